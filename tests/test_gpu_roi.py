"""ROI masks and GAME on the GPU (README, "ROI masks and GAME"): roi_weights_kernel bit for bit against the loop
reference of tests/roi_reference.py, the weighted instantiation of head_train_kernel against the unweighted one and the
staged fp32 reference, the count-metrics kernels against fp64, the native step with a 2-channel ground truth, and
evaluate_metrics through the GPU input pipeline.

Output buffers the tests allocate are pre-filled with NaN, so an element a kernel does not write shows.
"""
import copy
import math
import os

import numpy as np
import pytest
import torch

import elementwise_reference as R
import roi_reference as RR

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
NAN = float("nan")
_worst = {}          # (quantity, dtype) -> worst err / bound of the fractional-weight head runs of this session


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module: the worst err / bound per head quantity and dtype (shown with ``pytest -s``)."""
    yield
    for (q, dt), r in sorted(_worst.items()):
        print(f"\nROI HEAD fractional m {dt:<5s} {q:<5s} worst err/bound {r:.4f}", end="")
    print()


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require(), _ext


def _dt(dtype):
    from can_distributed_pytorch_amd.ops.conv import dt_code
    return dt_code(dtype)


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ----------------------------------------------------------------------------------------------------- weight kernel
def _rgba(h, w, seed, kind):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img[:, :, 3] = RR.make_mask(h, w, seed + 1, kind)
    return img


def _weights_of(packed):
    """(plane 0, plane 1 of the roi launch, the gt of the same pack without roi) on the host."""
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    x4, gt2 = preprocess_packed(packed, "cuda", roi=True)
    x4b, gt = preprocess_packed(packed, "cuda")
    torch.cuda.synchronize()
    assert tuple(gt2.shape) == (gt.shape[0], 2) + tuple(gt.shape[2:]) and gt2.dtype == torch.float32
    assert torch.equal(_bits(x4), _bits(x4b))                       # the image launch is what it was
    return gt2[:, 0].cpu(), gt2[:, 1].cpu(), gt[:, 0].cpu()


@pytest.mark.parametrize("kind", ["binary", "frac"])
@pytest.mark.parametrize("ch,cw,s", RR.SCALED_WINDOWS, ids=lambda v: str(v))
def test_weights_of_scaled_windows(ch, cw, s, kind):
    """A scaled-crop pack of one image, both flips: plane 1 is the reference bit for bit, plane 0 the pack's gt."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    sh, sw = RR.window_of(ch, cw, s)
    img = _rgba(sh + 5, sw + 9, 10 * ch + int(8 * s), kind)
    gts = torch.rand(2, 1, ch // 8, cw // 8, generator=torch.Generator().manual_seed(ch))
    wins = torch.tensor([[3, 7, 0, sh, sw], [3, 7, 1, sh, sw]], dtype=torch.int64)
    packed = PackedCollate(crop=(ch, cw), crop_scale=True)([(torch.from_numpy(img), gts, wins)])
    p0, p1, gt = _weights_of(packed)
    assert torch.equal(_bits(p0), _bits(gt)) and torch.equal(_bits(gt), _bits(gts[:, 0]))
    for k, flip in enumerate((False, True)):
        want = RR.roi_weights_ref(img[:, :, 3], 3, 7, sh, sw, ch // 8, cw // 8, flip)
        assert np.array_equal(p1[k].numpy().view(np.int32), want.view(np.int32)), (k, flip)


@pytest.mark.parametrize("kind", ["binary", "frac"])
@pytest.mark.parametrize("h0,w0,ch,cw", [(21, 45, 16, 24), (150, 280, 136, 264), RR.SMALL_IMAGE + RR.SMALL_CROP],
                         ids=["16x24", "136x264", "padded"])
def test_weights_of_unscaled_crops(h0, w0, ch, cw, kind):
    """An unscaled-crop pack, both flips; the last image is smaller than the crop: its padding cells are 0."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    img = _rgba(h0, w0, h0 + w0, kind)
    vh, vw = min(ch, h0 // 8 * 8), min(cw, w0 // 8 * 8)
    y0, x0 = h0 - vh, (w0 - vw) // 2
    gts = torch.rand(2, 1, ch // 8, cw // 8, generator=torch.Generator().manual_seed(ch))
    wins = torch.tensor([[y0, x0, 0], [y0, x0, 1]], dtype=torch.int64)
    packed = PackedCollate(crop=(ch, cw))([(torch.from_numpy(img), gts, wins)])
    p0, p1, gt = _weights_of(packed)
    assert torch.equal(_bits(p0), _bits(gt))
    for k, flip in enumerate((False, True)):
        want = RR.roi_weights_padded_ref(img[:, :, 3], y0, x0, ch, cw, 8, flip)
        assert np.array_equal(p1[k].numpy().view(np.int32), want.view(np.int32)), (k, flip)
        if (vh, vw) != (ch, cw):
            assert bool((p1[k][vh // 8:] == 0).all()) and bool((p1[k][:, vw // 8:] == 0).all())


@pytest.mark.parametrize("kind", ["binary", "frac", "ones"])
def test_weights_of_whole_images(kind):
    """An uncropped pack of two 37 x 53 images, one flipped: the window is the whole image, 4 x 6 cells."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    h0, w0 = RR.WHOLE_IMAGE
    imgs = [_rgba(h0, w0, 50 + k, kind) for k in range(2)]
    gts = torch.rand(2, 1, h0 // 8, w0 // 8, generator=torch.Generator().manual_seed(1))
    packed = PackedCollate()([(torch.from_numpy(imgs[k]), gts[k], bool(k)) for k in range(2)])
    p0, p1, gt = _weights_of(packed)
    assert torch.equal(_bits(p0), _bits(gt))
    for k in range(2):
        want = RR.roi_weights_ref(imgs[k][:, :, 3], 0, 0, h0, w0, h0 // 8, w0 // 8, bool(k))
        assert np.array_equal(p1[k].numpy().view(np.int32), want.view(np.int32))
        if kind == "ones":
            assert bool((p1[k] == 1).all())


SIZES = [(40, 56), (21, 45), (37, 53)]
CROP = (32, 40)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return RR.write_folder(str(tmp_path_factory.mktemp("roi")), SIZES, seed=3)


PACK_KINDS = [(dict(crop=CROP, crops_per_image=2), dict(crop=CROP)),
              (dict(crop=CROP, crops_per_image=2, gt_from_heads=True), dict(crop=CROP, gt_from_heads=True)),
              (dict(crop=CROP, crops_per_image=2, crop_scale=(0.5, 2.0), gt_from_heads=True),
               dict(crop=CROP, crop_scale=True, gt_from_heads=True)),
              (dict(crop=CROP, crops_per_image=2, crop_scale=(0.5, 2.0), photo_jitter=(0.2, 0.3, 1.5), gray_prob=0.5),
               dict(crop=CROP, crop_scale=True, photo=True)),
              (dict(crop=CROP, crops_per_image=2, gt_from_heads=True, gray_prob=0.5),
               dict(crop=CROP, gt_from_heads=True, photo=True))]


@pytest.mark.parametrize("kw,ckw", PACK_KINDS, ids=["crop", "crop+heads", "scaled+heads", "scaled+photo",
                                                    "crop+heads+photo"])
def test_dataset_packs_of_every_kind(folder, kw, ckw):
    """CrowdDataset(raw=True, roi=True) packs: plane 0 is the ground truth the pack gives without roi (rendered by
    gt_from_heads where the pack has heads), plane 1 the weights the CPU dataset computes for the same windows."""
    from can_distributed_pytorch_amd.data import CrowdDataset
    from can_distributed_pytorch_amd.data.dataset import crop_collate
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    img_root, gt_root = folder
    raw = CrowdDataset(img_root, gt_root, 8, phase="train", seed=5, raw=True, roi=True, **kw)
    cpu = CrowdDataset(img_root, gt_root, 8, phase="train", seed=5, roi=True, **kw)
    p0, p1, gt = _weights_of(PackedCollate(**ckw)([raw[i] for i in range(len(SIZES))]))
    _, want = crop_collate([cpu[i] for i in range(len(SIZES))])
    assert torch.equal(_bits(p0), _bits(gt))
    assert torch.equal(_bits(p1), _bits(want[:, 1]))
    if "gt_from_heads" in kw:
        assert float(p0.abs().sum()) > 0


def test_refusals(ext, folder):
    """A 3-channel pack is refused (-31) before any launch; a crop that is no multiple of d (-32) and a window that
    leaves its image or is empty (-33) have their own codes (the check reads host descriptors only)."""
    from can_distributed_pytorch_amd.data import CrowdDataset
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    C, _ = ext
    img_root, gt_root = folder
    rgb = CrowdDataset(img_root, gt_root, 8, phase="train", seed=5, raw=True, crop=CROP)
    packed = PackedCollate(crop=CROP)([rgb[0]])
    with pytest.raises(RuntimeError, match="-31"):
        preprocess_packed(packed, "cuda", roi=True)

    def check(rows, ch=32, cw=40, d=8, nbytes=1 << 20):
        desc = torch.tensor(rows, dtype=torch.int64)
        return C.roi_weights_check(desc.data_ptr(), desc.shape[0], nbytes, ch, cw, d)

    ok = [0, 64, 80, 4, 0, 5, 7, 1]
    assert check([ok]) == 0
    assert check([ok, [0, 64, 80, 3, 0, 5, 7, 1]]) == -31
    assert check([ok], ch=36) == -32 and check([ok], cw=44) == -32
    assert check([[0, 64, 80, 4, 0, 33, 7, 1]]) == -33                       # y0 + 32 > 64
    assert check([[0, 64, 80, 4, 0, 0, 0, (65 << 32) | 40]]) == -33          # taller than the image
    assert check([[0, 64, 80, 4, 0, 0, 0, (32 << 32) | 40]]) == 0
    assert check([[0, 64, 80, 4, 0, 0, 0, 40]]) == -33                       # sh == 0: an empty window
    assert check([[0, 64, 80, 4, 0, 0, 0, 0]], ch=64, cw=80) == 0            # a whole image
    assert check([[0, 64, 80, 4, 0, 0, 0, 0]], ch=32, cw=40) == -33          # a whole image of another size
    assert check([ok], nbytes=64 * 80 * 4 - 1) == -33                        # the image leaves the packed bytes


# ----------------------------------------------------------------------------------------------------- weighted head
def _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch=0, wv=0, wt=None, seed=0):
    C, X = ext
    P = y.shape[0]
    st = X.stream_ptr()
    et, part = _full((P,), NAN), _full((nblk, 66), NAN)
    dy = _full((P, 64), NAN, y.dtype)
    loss, nonfinite = _full((1,), NAN), _full((1,), NAN)
    if beta != 0.0:
        g = torch.Generator().manual_seed(seed + 77)
        dw, db = torch.randn(64, generator=g).cuda(), torch.randn(1, generator=g).cuda()
    else:
        dw, db = _full((64,), NAN), _full((1,), NAN)
    old = (dw.clone(), db.clone())
    ls = torch.tensor([lscale], dtype=torch.float32, device="cuda") if lscale is not None else None
    C.head_train(y.data_ptr(), w.data_ptr(), b.data_ptr(), gt.data_ptr(), et.data_ptr(), dy.data_ptr(),
                 part.data_ptr(), nblk, dw.data_ptr(), db.data_ptr(), loss.data_ptr(), P, gscale, beta,
                 ls.data_ptr() if ls is not None else 0, nonfinite.data_ptr(), _dt(y.dtype), st, pitch, wv,
                 *(() if wt is None else (wt.data_ptr(),)))
    torch.cuda.synchronize()
    return dict(et=et, dy=dy, dw=dw, db=db, loss=loss, nonfinite=nonfinite, part=part, old=old)


def _head_cases():
    """(P, nblk, pitch, wv, id): the plain cases, then the width-padded ones."""
    out = [(P, nblk, 0, 0, f"P={P} nblk={nblk}") for P, nblk in RR.WEIGHTED_HEAD_CASES]
    out += [(rows * pitch, math.ceil(rows * pitch / 32), pitch, wv, f"rows={rows} pitch={pitch} wv={wv}")
            for rows, pitch, wv in R.HEAD_PADDED]
    return out


def _head_inputs(P, dtype, pitch, wv, seed):
    y, w, b, gt = R.head_inputs(P, dtype, seed=seed, device="cuda")
    if pitch > wv:                                                 # padding columns: loud values that must not count
        pad = ~R.head_valid(P, pitch, wv, "cuda")
        y[pad] = 3.0
        gt[pad] = 1e6
    return y, w, b, gt


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk,pitch,wv,case", _head_cases(), ids=[c[4] for c in _head_cases()])
def test_weighted_head_with_unit_weight_is_the_unweighted_launch(ext, P, nblk, pitch, wv, case, dtype):
    """(a) m = 1: dm is d itself, so et, dy, dw, db and the loss equal the unweighted launch's bit for bit."""
    y, w, b, gt = _head_inputs(P, dtype, pitch, wv, 2000 + P + nblk)
    ones = torch.ones(P, device="cuda")
    for gscale, lscale, beta in R.HEAD_CONFIGS:
        a = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch, wv, seed=P)
        o = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch, wv, wt=ones, seed=P)
        for q in ("et", "dy", "dw", "db", "loss", "nonfinite", "part"):
            assert torch.equal(_bits(o[q]), _bits(a[q])), (case, q, gscale, lscale, beta)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk,pitch,wv,case", _head_cases(), ids=[c[4] for c in _head_cases()])
def test_weighted_head_with_binary_weight(ext, P, nblk, pitch, wv, case, dtype):
    """(b) a binary m equals the unweighted launch on gt' = where(m, gt, et), et from head_fwd (bitwise head_train's):
    a masked pixel has d = 0 there and dm = 0 here, so both add exact zeros.  dy as floats (a zero's sign may differ),
    dw, db and the loss with torch.equal; et is stored unweighted."""
    C, X = ext
    y, w, b, gt = _head_inputs(P, dtype, pitch, wv, 3000 + P + nblk)
    m = (torch.rand(P, generator=torch.Generator().manual_seed(P)) < 0.6).float().cuda()
    et = _full((P,), NAN)
    C.head_fwd(y.data_ptr(), w.data_ptr(), b.data_ptr(), et.data_ptr(), P, _dt(dtype), X.stream_ptr(), pitch, wv)
    gt2 = torch.where(m > 0, gt, et)
    for gscale, lscale, beta in R.HEAD_CONFIGS:
        a = _run_head(ext, y, w, b, gt2, nblk, gscale, lscale, beta, pitch, wv, seed=P)
        o = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch, wv, wt=m, seed=P)
        assert torch.equal(_bits(o["et"]), _bits(et)) and torch.equal(_bits(a["et"]), _bits(et))
        assert torch.equal(o["dy"].float(), a["dy"].float()), (case, gscale, lscale, beta)
        for q in ("dw", "db", "loss"):
            assert torch.equal(o[q], a[q]), (case, q, gscale, lscale, beta)
        assert o["nonfinite"].item() == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk,pitch,wv,case", _head_cases(), ids=[c[4] for c in _head_cases()])
def test_weighted_head_with_fractional_weight(ext, P, nblk, pitch, wv, case, dtype):
    """(c) a fractional m: dy bit for bit the staged fp32 reference (head_staged with the one extra product), dw, db
    and the loss within elementwise_reference.sum_ratio's bound 2 L 2^-24 sum|terms| on the staged fp32 values.
    Measured ratios: profiles/r20/roi_head_errors.txt."""
    y, w, b, gt = _head_inputs(P, dtype, pitch, wv, 4000 + P + nblk)
    m = torch.rand(P, generator=torch.Generator().manual_seed(P + 1)).cuda()
    m[::7] = 0.0
    m[3::11] = 1.0
    name = "bf16" if dtype == torch.bfloat16 else "fp16"
    failed = []
    for gscale, lscale, beta in R.HEAD_CONFIGS:
        o = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch, wv, wt=m, seed=P)
        st = RR.head_staged_weighted(o["et"], y, w, gt, m, gscale, lscale, pitch, wv)
        if not torch.equal(_bits(o["dy"]), _bits(st.dy)):
            failed.append(f"{case}: dy differs from the staged reference at "
                          f"{int((o['dy'].float() != st.dy.float()).sum())} elements")
        if not bool((o["dy"].float()[~st.valid] == 0).all() and (o["et"][~st.valid] == 0).all()):
            failed.append(f"{case}: et / dy not 0 at a padding pixel")
        for q, got, ref, mag, bt, old in (("dw", o["dw"], st.dw, st.dw_mag, beta, o["old"][0]),
                                          ("db", o["db"], st.db, st.db_mag, beta, o["old"][1]),
                                          ("loss", o["loss"], st.loss, st.loss_mag, 0.0, None)):
            ratio = R.sum_ratio(got, ref, mag, P, nblk, bt, old)
            print(f"ROI HEAD {case} {name} {q} gscale {gscale} lscale {lscale} beta {beta}: err/bound {ratio:.4f}")
            _worst[(q, name)] = max(_worst.get((q, name), 0.0), ratio)
            if not ratio <= 1.0:
                failed.append(f"{case} {q}: err / bound = {ratio:.4g} (gscale {gscale}, lscale {lscale}, beta {beta})")
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------- metrics kernel
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n,h,w", RR.METRIC_SHAPES)
def test_count_metrics_kernel(n, h, w, masked):
    from can_distributed_pytorch_amd.engine.metrics import count_metrics
    et, gt, m = RR.metric_inputs(n, h, w, seed=h * w + n, exact=True)
    terms = (m if masked else torch.ones_like(m)).double() * (et.double().abs() + gt.double().abs())
    assert float(terms.sum()) * 2.0 ** 10 < 2.0 ** 53            # every partial sum is exact in fp64, in any order
    gt_t = (torch.stack([gt, m], 1) if masked else gt[:, None]).cuda()
    ref, _ = RR.count_metrics_ref(et, gt, m if masked else None)
    got = count_metrics(et[:, None].cuda(), gt_t)
    again = count_metrics(et[:, None].cuda(), gt_t)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, 6)
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(got, again)
    et, gt, m = RR.metric_inputs(n, h, w, seed=9 + h, exact=False)
    gt_t = (torch.stack([gt, m], 1) if masked else gt[:, None]).cuda()
    ref, bound = RR.count_metrics_ref(et, gt, m if masked else None)
    got = count_metrics(et[:, None].cuda(), gt_t)
    again = count_metrics(et[:, None].cuda(), gt_t)
    torch.cuda.synchronize()
    err = (got.cpu() - ref).abs()
    print(f"COUNT METRICS n={n} {h}x{w} masked={masked}: worst err/bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert bool((err <= bound).all()), (err, bound)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))            # bitwise repeatable


# --------------------------------------------------------------------------------------------------------------- step
def _model(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    m = CANNet(backend="torch")
    for mod in m.modules():                           # He init so the signal survives 16 ReLU layers in a short test
        if isinstance(mod, torch.nn.Conv2d):
            fan_in = mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
            torch.nn.init.normal_(mod.weight, std=(2.0 / fan_in) ** 0.5)
            if mod.bias is not None:
                torch.nn.init.uniform_(mod.bias, -0.05, 0.05)
    m.exec_backend = "hip"
    return m.cuda()


def _stepper(model, **kw):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    kw.setdefault("graph", False)
    kw.setdefault("lr", 1e-6)
    return NativeStepper("cuda", model=copy.deepcopy(model), **kw)


def _batch(h, w, seed, n=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, 3, h, w, device="cuda", generator=g),
            torch.rand(n, 1, h // 8, w // 8, device="cuda", generator=g),
            torch.rand(n, 1, h // 8, w // 8, device="cuda", generator=g))


def _packs(ex):
    packs = [t for s in ex.front + ex.back for t in ex.packs[id(s.module.weight)] if t is not None]
    return packs + [t for sc in (1, 2, 3, 6) for t in ex.packs[id(ex.ctx2[sc].weight)]]


@pytest.mark.parametrize("h,w", [(64, 64), (72, 88)], ids=["64x64", "72x88"])
def test_step_with_unit_weight_is_the_plain_step(h, w):
    """m = 1: the masters, the momentum, the weight packs and the loss equal the 1-channel step's bit for bit (72 x 88
    is a width-padded map: both planes are padded to the pitch)."""
    model = _model(3)
    a, b = _stepper(model), _stepper(model)
    for i in range(2):
        x, gt, _ = _batch(h, w, 10 + i, n=2)
        la, lb = a.step(x, gt), b.step(x, torch.cat([gt, torch.ones_like(gt)], 1))
        assert float(la) == float(lb)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(_packs(a.ex), _packs(b.ex)))
    assert not torch.equal(a.arena.data, _stepper(model).arena.data)


def test_captured_step_with_a_mask_replays_the_eager_one():
    model = _model(4)
    a, b = _stepper(model, graph=False), _stepper(model, graph=True)
    for i in range(3):
        x, gt, m = _batch(64, 64, 20 + i)
        m = torch.where(m < 0.3, torch.zeros_like(m), m)
        la, lb = a.step(x, torch.cat([gt, m], 1)), b.step(x, torch.cat([gt, m], 1))
        assert float(la) == float(lb)
    torch.cuda.synchronize()
    assert b.graph_captures == 1
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)
    plain = _stepper(model)
    for i in range(3):
        x, gt, _ = _batch(64, 64, 20 + i)
        plain.step(x, gt)
    assert not torch.equal(a.arena.data, plain.arena.data)        # the mask took part


@pytest.mark.parametrize("h,w", [(64, 64), (72, 88)], ids=["64x64", "72x88"])
def test_zero_weight_gives_zero_gradient_into_the_backend(h, w):
    """m = 0 over the lower half of the map: d_b6 is exactly zero there, et is still stored, and the loss is the
    upper half's."""
    model = _model(5)
    st = _stepper(model)
    ex = st.ex
    x, gt, _ = _batch(h, w, 30, n=2)
    m = torch.ones_like(gt)
    half = gt.shape[2] // 2
    m[:, :, half:] = 0.0
    b6, _ = ex.forward_features(x, save=True)
    grads = [None] * ex.n_params
    grads[ex.head_w_index], grads[ex.head_b_index] = _full((1, 64, 1, 1), NAN), _full((1,), NAN)
    loss, et, d_b6 = ex.head_train(b6, torch.cat([gt, m], 1), grads)
    torch.cuda.synchronize()
    wv = gt.shape[3]
    assert tuple(et.shape) == tuple(gt.shape) and bool(torch.isfinite(et).all()) and float(et[:, :, half:].abs().sum()) > 0
    assert bool((d_b6[:, half:].float() == 0).all())
    assert float(d_b6[:, :half, :wv].float().abs().sum()) > 0
    want = ((et.double() - gt.double()) ** 2 * m.double()).sum().item()
    assert abs(float(loss) - want) <= 1e-4 * want
    with pytest.raises(ValueError):
        ex.head_train(b6, torch.cat([gt, m], 1).double(), grads)
    with pytest.raises(ValueError):
        ex.head_train(b6, torch.cat([gt, m, m], 1), grads)


# --------------------------------------------------------------------------------------------------------- evaluation
class _PoolModel(torch.nn.Module):
    """A stand-in network: 8 x 8 mean of the first input channel, recorded so that the CPU path sees the same map."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x4):
        et = torch.nn.functional.avg_pool2d(x4[..., 0].float()[:, None], 8)
        self.seen.append(et.cpu())
        return et


def test_evaluate_metrics_through_the_gpu_input_pipeline(folder):
    """evaluate_metrics over raw test items (GPU: the roi launch renders the weights, the kernels count) against the
    torch float64 definition on the CPU dataset's 2-channel ground truth of the same images, within the metrics bound
    summed over the images."""
    from can_distributed_pytorch_amd.data import CrowdDataset
    from can_distributed_pytorch_amd.engine.metrics import count_metrics_torch, evaluate_metrics
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    img_root, gt_root = folder
    raw = CrowdDataset(img_root, gt_root, 8, phase="test", raw=True, roi=True)
    cpu = CrowdDataset(img_root, gt_root, 8, phase="test", roi=True)
    loader = torch.utils.data.DataLoader(raw, batch_size=1, shuffle=False, collate_fn=PackedCollate())
    model = _PoolModel()
    got = evaluate_metrics(model, loader, torch.device("cuda"),
                           prep=lambda b: preprocess_packed(b, "cuda", roi=True))
    assert got["n"] == len(SIZES) and len(got["game"]) == 4 and len(model.seen) == len(SIZES)
    game, se, gb, sb = [0.0] * 4, 0.0, [0.0] * 4, 0.0
    for i, et in enumerate(model.seen):
        gt2 = cpu[i][1][None]
        cm = count_metrics_torch(et, gt2)[0]
        _, bound = RR.count_metrics_ref(et[:, 0], gt2[:, 0], gt2[:, 1])
        d = float(cm[0] - cm[1])
        se += d * d
        sb += 2 * abs(d) * float(bound[0, 0] + bound[0, 1]) + float(bound[0, 0] + bound[0, 1]) ** 2
        for lvl in range(4):
            game[lvl] += float(cm[2 + lvl])
            gb[lvl] += 2 * float(bound[0, 2 + lvl])                 # both paths are within the bound of the reference
    for lvl in range(4):
        assert abs(got["game"][lvl] - game[lvl]) <= gb[lvl] + 2.0 ** -50 * game[lvl], (lvl, got["game"], game)
    assert abs(got["se"] - se) <= 2 * sb + 2.0 ** -50 * se
    assert got["game"][0] <= got["game"][1] <= got["game"][2] <= got["game"][3]
