"""The fused optimizer-and-pack launches (elementwise.hip pack_multi_kernel: C.pack_multi, C.opt_pack with and without
EMA, C.swap_pack) bit for bit against the numpy model of tests/optpack_reference.py, on descriptor tables
built by hand: no CANNet, no executor.

One table of about 150 k floats holds whole tiles (the float4 path, nine Adam-loop iterations per thread), the
interleaved context packs, partial tiles with channel counts that are and are not multiples of 8, the first-layer
layout, null dgrad packs on a whole and on a partial tile, a dgrad pack 8 bytes off 16-byte alignment, and mode -1
rows at every chunk boundary.  It is laid out seven ways (R.LAYOUTS): aligned, every arena one float past alignment,
each of the gradient / momentum / second-moment / EMA arenas alone 1 (mod 4) floats from the masters, and one master
slot 4 bytes off inside an aligned arena.  Every packed row starts with directed blocks (R.initial_values): masters on
a 16-bit midpoint with an update below half an fp32 ulp, and masters in the fp16 subnormal range.

Per launch kind, element type and layout:
  1. masters, momentum, second moment and EMA arena bit-equal to the emulation;
  2. the gradient arena untouched;
  3. every pack, the context packs included, bit-equal to the layout function applied to round16(master as stored);
  4. the sentinel words between slots, between packs and in the first-layer pack's unwritten positions unchanged;
  5. with flags[0] or flags[2] set nothing changes, no count advances, flags[3] latches only for flags[0];
  6. two swaps restore everything;
  7. a second step from the first step's result (learning rate from the device, a gradient multiplier) matches too.
     The kind "sgd_nogmul" is the plain SGD launch of the default training step: C.opt_pack with opt = OPT_SGD and no
     gradient multiplier on either step, so its step 2 takes the non-power-of-two gscale alone.
(1, 2 and 4 are one comparison of the whole fp32 buffer, 3 and 4 one of the whole pack buffer.)

Adam's p is held bit for bit like the rest: the kernel's divide and square root are the correctly rounded ones (HIP's
default, which adam1's comment promises), and tests/test_optpack_reference_cpu.py shows that the per-launch
coefficients of the step counts used here cannot depend on the last bit of a device double operation.
What the parent of this test's commit got wrong, and five mutants of the kernel it catches:
profiles/r19/optpack_mutants.txt."""
import functools

import numpy as np
import pytest
import torch

import optpack_reference as R

pytestmark = pytest.mark.gpu

T0, EMA_N0 = 11, 3                      # preset device counts (Adam steps / EMA updates applied so far)
LR_DEV, GMUL = 3e-3, 0.37               # step 2: learning rate read from the device, gradient multiplier,
GSCALE2 = 0.01                          #   and a gradient scale that is no power of two: (g * gscale) * gmul and
                                        #   g * (gscale * gmul) then round differently, only the second is right
BETAS, EPS, EMA_DECAY = (0.9, 0.999), 1e-8, 0.999
OPT_KINDS = ("sgd", "sgd_wd", "adam", "adamw")
KINDS = ("pack", "sgd_nogmul") + OPT_KINDS + tuple(k + "+ema" for k in OPT_KINDS) + ("swap",)
DTS = ((R.DT_F16, "fp16"), (R.DT_BF16, "bf16"))


def _C():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _table(layout):
    return R.Table(layout)


@functools.lru_cache(maxsize=None)
def _chain(kind):
    """Slot values before, after step 1 (host learning rate) and after step 2 (device learning rate, and a gradient
    multiplier where the entry point takes one): computed once, the same in every layout and element type."""
    base, _, ema = kind.partition("+")
    emu = "sgd" if base == "sgd_nogmul" else base
    v0 = R.initial_values()
    v1 = R.apply_launch(v0, emu, t=T0, ema=bool(ema), ema_n=EMA_N0, ema_decay=EMA_DECAY, betas=BETAS, eps=EPS)
    v2 = R.apply_launch(v1, emu, t=T0 + 1, ema=bool(ema), ema_n=EMA_N0 + 1, ema_decay=EMA_DECAY, betas=BETAS, eps=EPS,
                        lr=LR_DEV, gscale=GSCALE2, gmul=None if base == "sgd_nogmul" else GMUL)
    return v0, v1, v2


def _buf32(table, vals):
    buf = np.full(table.total32, R.SENT32, dtype=np.uint32)
    for a in R.ARENAS:
        table.put(buf, a, vals[a])
    return buf


class Dev:
    """The table's two buffers, its descriptor rows and the launch's device scalars on the GPU."""

    def __init__(self, table, dt):
        self.table, self.dt = table, dt
        buf32, buf16 = table.initial()
        self.init32, self.init16 = buf32, buf16
        self.d32 = torch.from_numpy(buf32.view(np.int32).copy()).cuda()
        self.d16 = torch.from_numpy(buf16.view(np.int16).copy()).cuda()
        assert self.d32.data_ptr() % 16 == 0 and self.d16.data_ptr() % 16 == 0
        self.desc = torch.from_numpy(table.desc(self.d32.data_ptr(), self.d16.data_ptr())).cuda()
        self.pdesc = torch.from_numpy(table.desc(self.d32.data_ptr(), self.d16.data_ptr(), packed_only=True)).cuda()
        self.t = torch.full((1,), T0, dtype=torch.int32, device="cuda")
        self.ema_t = torch.full((1,), EMA_N0, dtype=torch.int32, device="cuda")
        self.flags = torch.zeros(4, device="cuda")
        self.lr_dev = torch.full((1,), LR_DEV, device="cuda")
        self.gmul = torch.full((1,), GMUL, device="cuda")

    def get(self):
        torch.cuda.synchronize()
        return self.d32.cpu().numpy().view(np.uint32), self.d16.cpu().numpy().view(np.uint16)

    def counts(self):
        return int(self.t), int(self.ema_t)

    def launch(self, kind, step2=False):
        C, tb = _C(), self.table
        base, _, ema = kind.partition("+")
        lr_dev = self.lr_dev.data_ptr() if step2 else 0
        gscale = GSCALE2 if step2 else R.GSCALE
        if base == "pack":
            C.pack_multi(self.pdesc.data_ptr(), self.pdesc.shape[0], tb.pack_tiles, self.dt, _stream())
        elif base == "swap":
            C.swap_pack(self.desc.data_ptr(), self.desc.shape[0], tb.max_tiles, tb.eoff, self.dt, _stream())
        else:
            opt = {"sgd_nogmul": R.OPT_SGD, "sgd": R.OPT_SGD, "sgd_wd": R.OPT_SGD_WD, "adam": R.OPT_ADAM,
                   "adamw": R.OPT_ADAM}[base]
            wd = 0.0 if opt == R.OPT_SGD else R.WD
            kw = dict(eoff=tb.eoff, ema_decay=EMA_DECAY, ema_warmup=1, ema_t=self.ema_t.data_ptr()) if ema else {}
            C.opt_pack(self.desc.data_ptr(), self.desc.shape[0], tb.max_tiles, opt, tb.goff, tb.boff, tb.voff, R.LR,
                       R.MOMENTUM, BETAS[0], BETAS[1], EPS, wd, int(base == "adamw"), gscale,
                       self.t.data_ptr() if opt == R.OPT_ADAM else 0, self.flags.data_ptr(), lr_dev, self.dt,
                       _stream(), self.gmul.data_ptr() if step2 and base != "sgd_nogmul" else 0, **kw)


def _check(dev, want32, want16, what):
    got32, got16 = dev.get()
    rep = R.diff_report(dev.table, got32, want32, got16, want16)
    assert not rep, f"{what}:\n{rep}"


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("dt,dtname", DTS, ids=[n for _, n in DTS])
@pytest.mark.parametrize("kind", KINDS)
def test_launch_bit_exact(kind, dt, dtname, layout):
    table = _table(layout)
    dev = Dev(table, dt)
    base, _, ema = kind.partition("+")
    if base == "pack":
        want16 = table.packs_of(dev.init32, dev.init16, dt)
        for rep in ("first", "repeated"):
            dev.launch("pack")
            _check(dev, dev.init32, want16, f"pack_multi {rep}")
        # the masters moved: every pack follows
        v = dict(R.initial_values())
        v["w"] = v["e"]
        moved = _buf32(table, v)
        dev.d32.copy_(torch.from_numpy(moved.view(np.int32).copy()))
        dev.launch("pack")
        _check(dev, moved, table.packs_of(moved, want16, dt), "pack_multi of other masters")
        return
    if base == "swap":
        dev.launch("pack")
        p0 = table.packs_of(dev.init32, dev.init16, dt)
        swapped = _buf32(table, R.apply_launch(R.initial_values(), "swap"))
        dev.launch("swap")
        _check(dev, swapped, table.packs_of(swapped, p0, dt), "swap")
        dev.launch("swap")
        _check(dev, dev.init32, p0, "second swap")
        assert dev.counts() == (T0, EMA_N0)
        return
    v0, v1, v2 = _chain(kind)
    # 5. a skipped step changes nothing (the packs keep their prior bytes, here the sentinels)
    for idx in (0, 2):
        dev.flags.zero_()
        dev.flags[idx] = 1.0
        dev.launch(kind)
        _check(dev, dev.init32, dev.init16, f"skipped step, flags[{idx}]")
        assert dev.counts() == (T0, EMA_N0)
        assert dev.flags.tolist() == ([1.0, 0.0, 0.0, 1.0] if idx == 0 else [0.0, 0.0, 1.0, 0.0])
    dev.flags.zero_()
    adam = base in ("adam", "adamw")
    # 1. - 4. the step
    want32 = _buf32(table, v1)
    want16 = table.packs_of(want32, dev.init16, dt)
    dev.launch(kind)
    _check(dev, want32, want16, "step 1")
    assert dev.counts() == (T0 + adam, EMA_N0 + bool(ema))
    assert not np.array_equal(want32, dev.init32)
    # 7. a second step from the first step's result
    want32 = _buf32(table, v2)
    want16 = table.packs_of(want32, want16, dt)
    dev.launch(kind, step2=True)
    _check(dev, want32, want16, "step 2")
    assert dev.counts() == (T0 + 2 * adam, EMA_N0 + 2 * bool(ema))
    assert dev.flags.tolist() == [0.0] * 4


def test_repack_reproduces_the_optimizers_packs():
    """The invariant resume, swap_weights and refresh_packs rely on, stated directly: after an fp16 SGD step in the
    layout that sends every tile down the element-wise path, C.pack_multi from the stored masters rewrites every
    pack with the bytes the step wrote."""
    table = _table("all_off1")
    for kind in ("sgd_nogmul", "sgd+ema", "sgd_wd", "adam"):
        dev = Dev(table, R.DT_F16)
        dev.launch(kind)
        a32, a16 = dev.get()
        dev.launch("pack")
        b32, b16 = dev.get()
        assert np.array_equal(a32, b32)
        rep = R.diff_report(table, b32, a32, a16, b16)
        assert not rep, f"{kind}: the step's packs (got) differ from a re-pack of its masters (want):\n{rep}"
