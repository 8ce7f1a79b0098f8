"""The numpy model of the fused optimizer-and-pack launches (tests/optpack_reference.py) against independent
yardsticks on the CPU: fma32 and the 16-bit roundings against exact rational arithmetic and numpy / torch conversions,
the pack layouts against ops.conv's pack functions, the Adam emulation against torch.optim, and the conditions the
GPU tests (tests/test_gpu_optpack_exact.py) rely on: per-launch coefficients that a last-bit difference in a device
double operation cannot change, and directed blocks that do separate "pack of the stored master" from "pack of the
exact update"."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import optpack_reference as R

F32 = np.float32


def _exact_fma(a, b, c):
    return np.array([R.round_fp32_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], dtype=F32)


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def test_round_fp32_exact_on_known_values():
    u = 2.0 ** -24
    assert R.round_fp32_exact(Fraction(1) + Fraction(u)) == F32(1.0)                       # tie -> even
    assert R.round_fp32_exact(Fraction(1) + Fraction(3 * u)) == F32(1.0 + 4 * u)           # tie -> even
    assert R.round_fp32_exact(Fraction(1) + Fraction(u) + Fraction(1, 2 ** 90)) == F32(1.0 + 2 * u)
    assert R.round_fp32_exact(Fraction(1) + Fraction(u) - Fraction(1, 2 ** 90)) == F32(1.0)
    assert R.round_fp32_exact(-Fraction(3, 2 ** 150)) == F32(-2.0 ** -148)                  # subnormal tie -> even
    assert R.round_fp32_exact(Fraction(1, 3)) == F32(1.0 / 3.0)
    rng = np.random.default_rng(0)
    x = rng.standard_normal(2000) * np.exp2(rng.integers(-140, 120, 2000))
    got = np.array([R.round_fp32_exact(Fraction(float(v))) for v in x], dtype=F32)
    assert np.array_equal(_bits(got), _bits(x.astype(F32)))


def test_fma32_directed_midpoints():
    """p = -+(2^-24 - 2^-64) * 2^k added to c with every small mantissa: the float64 sum is exactly an fp32 midpoint,
    the true sum is not.  Rounding the float64 sum (two roundings) gets a share of these wrong; fma32 none."""
    a, b, c = [], [], []
    for k in (-20, 0, 1, 37):
        for mant in range(0, 12):
            for sp in (1.0, -1.0):
                for sc in (1.0, -1.0):
                    a.append(sp * 2.0 ** -12 * (1 + 2.0 ** -20) * 2.0 ** k)
                    b.append(2.0 ** -12 * (1 - 2.0 ** -20))
                    c.append(sc * (1 + mant * 2.0 ** -23) * 2.0 ** k)
    a, b, c = (np.array(v, dtype=F32) for v in (a, b, c))
    assert np.array_equal(a.astype(np.float64), np.array(a, dtype=np.float64))
    want = _exact_fma(a, b, c)
    got = R.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    wrong = int((_bits(naive) != _bits(want)).sum())
    print(f"directed: {a.size} cases, float64-then-float32 wrong on {wrong}")
    assert wrong >= a.size // 8, wrong            # the cases do hit the hazard
    assert np.array_equal(_bits(got), _bits(want))


def test_fma32_random_triples():
    rng = np.random.default_rng(1)
    n = 4000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, n))).astype(F32)
    # a third: c cancels the product to within a few ulp (results far smaller than the operands)
    k = n // 3
    c[:k] = -(a[:k] * b[:k]) * (1 + rng.integers(-3, 4, k) * 2.0 ** -23).astype(F32)
    # a third: the product is around half an ulp of c
    c[k:2 * k] = (a[k:2 * k].astype(np.float64) * b[k:2 * k] * np.exp2(rng.integers(22, 27, k))).astype(F32)
    got = R.fma32(a, b, c)
    want = _exact_fma(a, b, c)
    assert np.array_equal(_bits(got), _bits(want))
    # scalars broadcast
    assert np.array_equal(_bits(R.fma32(F32(3.0), a, F32(-1.0))), _bits(_exact_fma(np.full(n, 3.0), a, np.full(n, -1.0))))


def _round16_inputs():
    rng = np.random.default_rng(2)
    x = [rng.standard_normal(20000) * np.exp2(rng.integers(-30, 18, 20000))]
    # every fp16 value, every midpoint between neighbours, and one fp32 ulp either side of each
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = ((h[:-1] + h[1:]) / 2).astype(F32)
    x += [h, mid, np.nextafter(mid, F32(np.inf)), np.nextafter(mid, F32(-np.inf)), [65504.0, 65519.9, 65520.0, 1e6]]
    # bf16 midpoints around one and in the small range
    for e in (-40, -14, 0, 7):
        m = (1 + (2 * np.arange(0, 64) + 1) * 2.0 ** -8) * 2.0 ** e
        x += [m, np.nextafter(m.astype(F32), F32(np.inf)), np.nextafter(m.astype(F32), F32(-np.inf))]
    x = np.concatenate([np.asarray(v, dtype=np.float64) for v in x]).astype(F32)
    return np.concatenate([x, -x, np.zeros(1, dtype=F32)])


def test_round_fp16_bits():
    x = _round16_inputs()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = R.round_fp16(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    t = torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, t)
    assert R.round_fp16(F32(1 + 2.0 ** -11)) == 0x3C00 and R.round_fp16(F32(1 + 3 * 2.0 ** -11)) == 0x3C02
    assert R.round_fp16(F32(2.0 ** -25)) == 0 and R.round_fp16(F32(3 * 2.0 ** -25)) == 2
    assert R.round_fp16(np.nextafter(F32(2.0 ** -25), F32(1))) == 1


def test_round_bf16_bits():
    x = _round16_inputs()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.round_bf16(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert R.round_bf16(F32(1 + 2.0 ** -8)) == 0x3F80 and R.round_bf16(F32(1 + 3 * 2.0 ** -8)) == 0x3F82


@pytest.mark.parametrize("dt,tdt", [(R.DT_F16, torch.float16), (R.DT_BF16, torch.bfloat16)])
def test_layouts_match_pack_functions(dt, tdt):
    from can_distributed_pytorch_amd.ops import conv
    g = torch.Generator().manual_seed(3)

    def bits(t):
        return t.contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)
    for Co, Ci, k in ((64, 64, 3), (40, 24, 3), (5, 7, 3), (33, 35, 1), (32, 32, 1)):
        w = torch.randn(Co, Ci, k, k, generator=g) * 0.3
        h = R.round16(w.numpy().reshape(-1), dt)
        for fn, ref in ((R.layout_fwd, conv.pack_weight_fwd), (R.layout_dgr, conv.pack_weight_dgrad)):
            dst, src = fn(Co, Ci, k * k)
            out = np.zeros(Co * Ci * k * k, dtype=np.uint16)
            out[dst] = h[src]
            assert np.array_equal(np.sort(dst), np.arange(dst.size))
            assert np.array_equal(out, bits(ref(w, tdt))), (fn.__name__, Co, Ci, k)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    dst, src = R.layout_first(64, 3, 9)
    out = np.zeros(64 * 64, dtype=np.uint16)
    out[dst] = R.round16(w.numpy().reshape(-1), dt)[src]
    assert np.array_equal(out, bits(conv.pack_weight_first(w, tdt)))
    # the interleaved context packs: W2cat[4 co + si] = W2_si[co], and its transpose
    ws = [torch.randn(32, 32, 1, 1, generator=g) for _ in range(4)]
    cat = torch.stack([x.reshape(32, 32) for x in ws], dim=1).reshape(128, 32)
    fwd2, dgr2 = np.zeros(4096, dtype=np.uint16), np.zeros(4096, dtype=np.uint16)
    for si, x in enumerate(ws):
        h = R.round16(x.numpy().reshape(-1), dt)
        d, s = R.layout_fwd2(32, 32, si)
        fwd2[d] = h[s]
        d, s = R.layout_dgr2(32, 32, si)
        dgr2[d] = h[s]
    assert np.array_equal(fwd2, bits(cat.to(tdt)))
    assert np.array_equal(dgr2, bits(cat.t().contiguous().to(tdt)))


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_emulation_close_to_torch(decoupled):
    """A sanity check, not a pin: torch orders the same operations differently (addcdiv, its own bias-correction
    arithmetic), so agreement is to a few fp32 ulp of max(|p|, lr) per step."""
    rng = np.random.default_rng(4)
    n, steps, lr, wd = 5000, 5, 1e-3, 1e-2
    p0 = (rng.standard_normal(n) * 0.3).astype(F32)
    gs = [rng.standard_normal(n).astype(F32) for _ in range(steps)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([tp], lr=lr, betas=(0.9, 0.999), eps=1e-8,
                                                                   weight_decay=wd)
    p, m, v = p0, np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    for t, g in enumerate(gs, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        c = R.adam_coef(t=t, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=wd, decoupled=decoupled, gscale=1.0)
        p, m, v = R.adam_step(c, p, g, m, v)
        err = np.abs(p.astype(np.float64) - tp.detach().numpy().astype(np.float64))
        tol = 8 * t * 2.0 ** -24 * np.maximum(np.abs(p), lr)
        assert np.all(err <= tol), (t, float((err / tol).max()))
    assert not np.array_equal(p, p0)


# The GPU tests preset t = 11 and n = 3 and take two steps; step 1 uses LR on the host, step 2 LR_DEV on the device.
GPU_T, GPU_EMA_N, LR_DEV, GMUL, GSCALE2 = 11, 3, 3e-3, 0.37, 0.01


def test_step2_scalars_tell_the_gmul_orders_apart():
    """gmul enters as one fp32 product with gscale.  With step 2's gscale (no power of two) multiplying it in per
    element, (g * gscale) * gmul, rounds differently on a good share of the gradients; with step 1's power of two the
    two orders are the same number, which is why step 2 has a gscale of its own."""
    g = R.initial_values()["g"]
    once = R.mul32(g, R.eff_gscale(GSCALE2, GMUL))
    per_element = R.mul32(R.mul32(g, F32(GSCALE2)), F32(GMUL))
    assert float((once != per_element).mean()) > 0.2
    assert np.array_equal(R.mul32(g, R.eff_gscale(R.GSCALE, GMUL)), R.mul32(R.mul32(g, F32(R.GSCALE)), F32(GMUL)))


def test_gpu_coefficients_survive_a_last_bit_difference():
    """Every per-launch double scalar the GPU tests' launches cast to fp32 keeps its fp32 value when moved by up to
    8 double ulps: however the device forms beta^t, lr / bc1, sqrt(bc2) or (1 + n) / (10 + n) in the last bit (a
    contracted multiply-subtract, a divide or square root one ulp off), the expectation is the same."""
    for t in (GPU_T + 1, GPU_T + 2):
        for lr in (R.LR, LR_DEV):
            for decoupled in (False, True):
                c = R.adam_coef(t=t, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=R.WD, decoupled=decoupled,
                                gscale=R.GSCALE)
                assert R.coef_is_robust(c["_step_size64"]), (t, lr)
                assert R.coef_is_robust(c["_bc2s64"]), t
                assert R.coef_is_robust(1.0 - float(F32(lr)) * float(F32(R.WD)))
    assert R.coef_is_robust(1.0 - 0.9) and R.coef_is_robust(1.0 - 0.999) and R.coef_is_robust(0.999)
    for n in (GPU_EMA_N, GPU_EMA_N + 1):
        w, w64 = R.ema_coef(n=n, decay=0.999, warmup=True)
        assert R.coef_is_robust(w64) and w == F32(1.0 - (1.0 + n) / (10.0 + n))
    assert not R.coef_is_robust(float(F32(1.0)) + 2.0 ** -24)        # an fp32 midpoint: the check can fail


def test_powi_and_coefficients():
    assert R.powi(0.9, 12) == 0.9 ** 12 or abs(R.powi(0.9, 12) - 0.9 ** 12) < 1e-15
    assert R.powi(0.5, 10) == 2.0 ** -10 and R.powi(3.0, 0) == 1.0
    c = R.adam_coef(t=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, decoupled=False, gscale=1.0)
    assert abs(float(c["step_size"]) - 1e-2) < 1e-8 and abs(float(c["bc2s"]) - np.sqrt(1e-3)) < 1e-8
    assert R.eff_gscale(0.25, 0.37) == F32(0.25) * F32(0.37)


@pytest.mark.parametrize("kind,block", [("sgd", "A"), ("sgd_wd", "B")])
def test_directed_blocks_separate_stored_from_folded(kind, block):
    """In the directed block of every packed row the update is far below half an fp32 ulp: the stored master keeps
    its midpoint value, and a pack rounded from the exact update differs from the pack of the stored master in the
    cases where the update points away from the even neighbour."""
    table = R.Table("aligned")
    vals = R.initial_values()
    idx = R.directed_index(table, block)
    assert idx.size == R.N_DIRECTED * len(table.packed)
    # (a gradient multiplier rescales g * gscale, so block B's cancellation against WD * p holds without one only)
    for kw in (dict(), dict(lr=LR_DEV, gmul=GMUL, gscale=GSCALE2) if block == "A" else dict(lr=LR_DEV)):
        new = R.apply_launch(vals, kind, **kw)
        p0, p1, buf = vals["w"][idx], new["w"][idx], new["m"][idx]
        assert np.array_equal(_bits(p0), _bits(p1))                  # stored master unchanged
        assert np.all(buf != 0) and np.all(np.abs(buf) < 2.0 ** -19)
        exact_side = np.nextafter(p0, np.where(buf < 0, F32(np.inf), F32(-np.inf)).astype(F32))   # p - lr * buf
        for dt, sel in ((R.DT_F16, slice(0, 8)), (R.DT_BF16, slice(8, 16))):
            stored = R.round16(p1, dt).reshape(-1, R.N_DIRECTED)[:, sel]
            folded = R.round16(exact_side, dt).reshape(-1, R.N_DIRECTED)[:, sel]
            assert np.all((stored != folded).sum(axis=1) == 4), (dt, (stored != folded).sum(axis=1))
    # the issue's own example: p = 1 + 2^-11, g * gscale = -2^-20 -> stored 0x3C00, folded 0x3C01
    k = idx[0]
    assert vals["w"][k] == F32(1 + 2.0 ** -11)
    assert R.round_fp16(vals["w"][k]) == 0x3C00
    assert R.round_fp16(np.nextafter(vals["w"][k], F32(2))) == 0x3C01


def test_subnormal_block_stays_fp16_subnormal():
    table = R.Table("aligned")
    vals = R.initial_values()
    idx = R.directed_index(table, "S")
    for kind, kw in (("sgd", {}), ("sgd_wd", {}), ("adam", dict(t=GPU_T)), ("adamw", dict(t=GPU_T))):
        new = R.apply_launch(vals, kind, ema=True, ema_n=GPU_EMA_N, **kw)
        h = R.round_fp16(new["w"][idx])
        frac = float(((h & 0x7C00) == 0).mean())
        assert frac > 0.9, (kind, frac)                              # fp16 packs subnormal (or zero)
        assert len(np.unique(h)) > idx.size // 4


@pytest.mark.parametrize("layout", ["aligned", "grad_off1", "one_slot_off1"])
def test_expected_buffers(layout):
    """The builder's expectation for whole buffers: only slots of the arenas the launch writes change, every written
    pack element is the rounding of the master at its source index, everything else keeps its prior bytes."""
    t = R.Table(layout)
    buf32, buf16 = t.initial()
    for kind, kw, writes in (("pack", {}, ""), ("swap", {}, "we"), ("sgd", {}, "wm"),
                             ("adamw", dict(t=GPU_T, ema=True, ema_n=GPU_EMA_N), "wmve")):
        out32, out16 = R.expected_buffers(t, buf32, buf16, R.DT_F16, kind, **kw)
        for a in R.ARENAS:
            same = np.array_equal(t.slots(out32, a), t.slots(buf32, a))
            assert same == (a not in writes), (kind, a)
        touched = np.zeros(t.total32, dtype=bool)
        for a in writes:
            touched[t.base[a] + t.slot_idx] = True
        assert np.array_equal(out32[~touched], buf32[~touched])
        w = out32.view(F32)
        written = np.zeros(t.total16, dtype=bool)
        written[t.pack_dst] = True
        assert np.all(out16[~written] == R.SENT16) and written.sum() == t.pack_dst.size
        assert np.array_equal(out16[t.pack_dst], R.round_fp16(w[t.base["w"] + t.pack_src]))
    # the first-layer pack: 27 of each row's 64 slots written; a null dgrad pack writes nothing
    e = next(r for r in t.packed if r.first)
    assert int(written[e.fwd:e.fwd + 64 * 64].sum()) == 64 * 27
    assert sum(r.has_dgr for r in t.packed) == len(t.packed) - 3


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_table_layout(layout):
    """The builder's own promises: slots and packs disjoint with sentinels between, the alignments each layout names,
    max_tiles as the executor's opt_prepare computes it."""
    t = R.Table(layout)
    buf32, buf16 = t.initial()
    used = np.zeros(t.total32, dtype=np.int32)
    for _, off, n in t.regions32():
        used[off:off + n] += 1
        assert used[off - 1] == 0 and off + n < t.total32
    assert used.max() == 1 and np.all((buf32 == R.SENT32) == (used == 0))
    used16 = np.zeros(t.total16, dtype=np.int32)
    for _, off, n in t.regions16():
        used16[off:off + n] += 1
        assert off >= R.GAP16 and off + n + R.GAP16 <= t.total16 + 8
    assert used16.max() == 1
    mod = {a: (t.base[a] + t.rows[0].off) % 4 for a in R.ARENAS}
    want = {"aligned": (0, 0, 0, 0, 0), "all_off1": (1, 1, 1, 1, 1), "grad_off1": (0, 1, 0, 0, 0),
            "mom_off1": (0, 0, 1, 0, 0), "mom2_off1": (0, 0, 0, 1, 0), "ema_off1": (0, 0, 0, 0, 1),
            "one_slot_off1": (1, 1, 1, 1, 1)}[layout]
    assert tuple(mod[a] for a in R.ARENAS) == want
    if layout == "one_slot_off1":
        assert all((t.base["w"] + r.off) % 4 == 0 for r in t.rows[1:])
    d = t.desc(4096, 8192)
    rows = d.tolist()
    assert t.max_tiles == max(((r[3] + 31) // 32) * ((r[4] + 31) // 32) if r[7] >= 0 else -(-r[11] // 4096)
                              for r in rows) == 4
    g = [r for r in rows if r[7] == 0 and (r[2] - 8192) % 16 == 8]
    assert len(g) == 1 and g[0][1] % 16 == 0
    assert all(r[1] % 16 == 0 and (r[2] == 0 or r is g[0] or r[2] % 16 == 0) for r in rows if r[7] == 0)
    assert sum(1 for r in rows if r[7] == 0 and r[2] == 0 and not r[6]) == 2      # the two null dgrad packs
    assert sorted(r[10] for r in rows if r[8]) == [0, 1, 2, 3]
    assert d.shape == (len(t.rows), R.K_PACK_ROW) and sum(r.n for r in t.rows) < 200_000
