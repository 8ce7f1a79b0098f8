"""An independent model of elementwise.hip's fused optimizer-and-pack launches (pack_multi_kernel), numpy only.

Everything here is written from the kernel's documented operation order, never from its code paths: one element-wise
function per step kind built on exactly rounded fp32 primitives, the 16-bit roundings as bit patterns, the pack layouts
as index arithmetic, and a builder that lays a descriptor table out in memory and says what every byte of every buffer
must hold after a launch.  tests/test_optpack_reference_cpu.py checks this model against exact rational arithmetic and
against torch on the CPU; tests/test_gpu_optpack_exact.py holds the kernel to it bit for bit.

The invariant the model states for every launch kind: a pack is the 16-bit round-to-nearest-even of the fp32 master
AS STORED, laid out by the functions below.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

F32 = np.float32
F64 = np.float64
TINY32 = float(np.finfo(np.float32).tiny)

K_PACK_ROW = 12          # {w, fwd, dgr, Co, Ci, taps, first, mode, fwd2, dgr2, si, n}
CHUNK = 4096             # elements per block of a mode -1 row
DT_BF16, DT_F16 = 0, 1
OPT_SGD, OPT_SGD_WD, OPT_ADAM = 1, 2, 3


# ------------------------------------------------------------------ exactly rounded fp32 primitives
def _f32(x):
    return np.asarray(x, dtype=F32)


def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, element-wise.

    The product of two fp32 values has at most 48 significant bits: exact in float64.  s = fl64(p + c) is rounded
    once more to fp32; the two roundings differ from the single one only when s lands exactly on an fp32 rounding
    midpoint while the true sum does not.  TwoSum gives the exact error term of s, whose sign then says on which side
    of the midpoint the true sum lies.  (No overflow handling: the callers stay far from the fp32 range limits.)"""
    a, b, c = np.broadcast_arrays(_f32(a), _f32(b), _f32(c))
    p = a.astype(F64) * b.astype(F64)
    cd = c.astype(F64)
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)               # p + cd == s + err exactly (Knuth)
    r = s.astype(F32)
    rd = r.astype(F64)
    off = np.flatnonzero((rd != s) & (err != 0.0) & np.isfinite(s))
    if off.size:
        r = r.copy()
        rf, sf, ef = r.reshape(-1), s.reshape(-1), err.reshape(-1)
        ri, si, ei = rf[off], sf[off], ef[off]
        other = np.nextafter(ri, np.where(si > ri.astype(F64), F32(np.inf), F32(-np.inf)).astype(F32))
        # s - r and other - s are exact: all three lie within one fp32 ulp of each other
        mid = (si - ri.astype(F64)) == (other.astype(F64) - si)
        lo, hi = np.minimum(ri, other), np.maximum(ri, other)
        rf[off] = np.where(mid, np.where(ei > 0.0, hi, lo), ri)
        r = rf.reshape(s.shape)
    return r


def mul32(a, b):
    return _f32(a) * _f32(b)


def add32(a, b):
    return _f32(a) + _f32(b)


def sub32(a, b):
    return _f32(a) - _f32(b)


def div32(a, b):
    return _f32(a) / _f32(b)


def sqrt32(a):
    return np.sqrt(_f32(a))


def round_fp32_exact(x: Fraction) -> np.float32:
    """round-to-nearest-even of a rational to fp32 (normal and subnormal range), in integer arithmetic: the yardstick
    fma32 is tested against."""
    if x == 0:
        return F32(0.0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()      # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)                                 # in units of the ulp at exponent e
    n, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and (n & 1)):
        n += 1
    return F32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


# ------------------------------------------------------------------ 16-bit roundings, as bit patterns
def round_bf16(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_fp16(x):
    """fp32 -> fp16 bits, round to nearest even, subnormals included, overflow to infinity (finite inputs); integer
    arithmetic on the fp32 bit pattern."""
    u = _f32(x).view(np.uint32).astype(np.int64)
    sign = ((u >> 16) & 0x8000)
    exp = ((u >> 23) & 0xFF) - 127
    man = (u & 0x7FFFFF) | np.where(((u >> 23) & 0xFF) != 0, 0x800000, 0)      # 24-bit significand
    # value = man * 2^(exp - 23); the fp16 grid at this exponent has spacing 2^(max(exp, -14) - 10)
    shift = np.clip(13 + np.maximum(-14 - exp, 0), 13, 40)          # bits dropped (>= 38: everything rounds to 0)
    keep = man >> shift
    rem = man & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    keep = keep + ((rem > half) | ((rem == half) & ((keep & 1) == 1)))
    # normal: keep in [2^10, 2^11], bits = (exp + 15 - 1) << 10 + keep carries the exponent; subnormal: bits = keep
    bits = np.where(exp >= -14, ((exp + 14) << 10) + keep, keep)
    bits = np.where(bits >= 0x7C00, 0x7C00, bits)                   # overflow -> inf
    bits = np.where((u & 0x7FFFFFFF) == 0, 0, bits)
    return (sign | bits).astype(np.uint16)


def round16(x, dt):
    return round_fp16(x) if dt == DT_F16 else round_bf16(x)


def bits16_to_f64(bits, dt):
    """The value of a 16-bit pattern (for error messages and the CPU tests)."""
    b = np.asarray(bits, dtype=np.uint16)
    if dt == DT_F16:
        return b.view(np.float16).astype(F64)
    return (b.astype(np.uint32) << 16).view(F32).astype(F64)


# ------------------------------------------------------------------ the step kinds, element-wise
def _normal(*xs):
    """Every fp32 intermediate is zero or normal, so fp32 denormal handling is no part of any expectation."""
    for x in xs:
        ax = np.abs(np.asarray(x, dtype=F64))
        assert not np.any((ax != 0) & (ax < TINY32)), "fp32 subnormal intermediate"
        assert np.all(np.isfinite(ax))
    return xs[0]


def eff_gscale(gscale, gmul=None):
    """gmul enters once, as one fp32 product with gscale."""
    return F32(gscale) if gmul is None else _normal(mul32(F32(gscale), F32(gmul)))


def sgd_step(p, g, buf, *, lr, momentum, gscale, wd=None):
    """torch.optim.SGD with momentum (dampening 0), coupled weight decay when wd is given: returns (p, buf)."""
    g1 = _normal(mul32(g, F32(gscale)))
    if wd is not None:
        g1 = _normal(fma32(F32(wd), p, g1))
    buf = _normal(fma32(F32(momentum), buf, g1))
    p = _normal(fma32(-F32(lr), buf, p))
    return p, buf


def powi(b: float, n: int) -> float:
    """b^n in double by repeated squaring (multiply into the result where the bit is set, then square)."""
    r = 1.0
    while n:
        if n & 1:
            r *= b
        n >>= 1
        b *= b
    return r


def adam_coef(*, t, lr, beta1, beta2, eps, wd, decoupled, gscale, gmul=None):
    """The per-launch scalars of the Adam step for the 1-based step t, formed in double and cast to fp32 once."""
    lr = float(F32(lr))
    wd = float(F32(wd))
    bc1 = 1.0 - powi(beta1, t)
    bc2 = 1.0 - powi(beta2, t)
    return dict(
        gscale=eff_gscale(gscale, gmul),
        cwd=F32(0.0) if decoupled else F32(wd),
        decay=F32(1.0 - lr * wd) if decoupled else F32(1.0),
        w1=F32(1.0 - beta1), w2=F32(1.0 - beta2), b2=F32(beta2),
        step_size=F32(lr / bc1), bc2s=F32(np.sqrt(F64(bc2))), eps=F32(eps),
        _step_size64=lr / bc1, _bc2s64=float(np.sqrt(F64(bc2))))


def adam_step(c, p, g, m, v):
    """torch.optim.Adam / AdamW, one element: returns (p, m, v)."""
    g = _normal(mul32(g, c["gscale"]))
    g = _normal(fma32(c["cwd"], p, g))
    p = _normal(mul32(p, c["decay"]))
    m = _normal(fma32(c["w1"], _normal(sub32(g, m)), m))
    v = _normal(fma32(_normal(mul32(c["w2"], g)), g, _normal(mul32(c["b2"], v))))
    denom = _normal(add32(_normal(div32(_normal(sqrt32(v)), c["bc2s"])), c["eps"]))
    p = _normal(fma32(-c["step_size"], _normal(div32(m, denom)), p))
    return p, m, v


def ema_coef(*, n, decay, warmup):
    """(w as fp32, 1 - d_n in double): d_n = min(decay, (1 + n) / (10 + n)) with warm-up, n updates applied so far."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
    return F32(1.0 - d), 1.0 - d


def ema_step(w, p_stored, e):
    """e += w (p - e) from the new master as stored: one fp32 subtraction, one fma."""
    return _normal(fma32(w, _normal(sub32(p_stored, e)), e))


def coef_is_robust(x64: float, ulps: int = 8) -> bool:
    """A per-launch double scalar whose fp32 cast survives a perturbation of up to ``ulps`` double ulps either way:
    a last-bit difference in how a device forms it (a contracted multiply-subtract, a divide or square root that is
    off by an ulp) then cannot change the fp32 coefficient the elements see."""
    want = F32(x64)
    lo = hi = F64(x64)
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        if F32(lo) != want or F32(hi) != want:
            return False
    return True


# ------------------------------------------------------------------ pack layouts, as index arithmetic
# Each returns (dst, src): pack.flat[dst] = round16(w.flat[src]) for a weight stored [Co][Ci][taps].
def _grid(Co, Ci, taps):
    i = np.arange(Co * Ci * taps, dtype=np.int64)
    return i, i // (Ci * taps), (i // taps) % Ci, i % taps


def layout_fwd(Co, Ci, taps):
    """fwd[co][tap][ci]"""
    src, co, ci, tap = _grid(Co, Ci, taps)
    return (co * taps + tap) * Ci + ci, src


def layout_dgr(Co, Ci, taps):
    """dgr[ci][taps - 1 - tap][co]"""
    src, co, ci, tap = _grid(Co, Ci, taps)
    return (ci * taps + (taps - 1 - tap)) * Co + co, src


def layout_first(Co, Ci, taps):
    """The first layer's fwd[co][64], k = tap * 4 + c; the other slots of a row are not written."""
    assert Ci <= 4 and taps * 4 <= 64
    src, co, ci, tap = _grid(Co, Ci, taps)
    return co * 64 + tap * 4 + ci, src


def layout_fwd2(Co, Ci, si):
    """The interleaved context pack fwd2[4 co + si][ci] of a 1x1 weight."""
    src, co, ci, _ = _grid(Co, Ci, 1)
    return (4 * co + si) * Ci + ci, src


def layout_dgr2(Co, Ci, si):
    """Its transpose dgr2[ci][4 co + si]."""
    src, co, ci, _ = _grid(Co, Ci, 1)
    return ci * (4 * Co) + 4 * co + si, src


# ------------------------------------------------------------------ the descriptor table
LAYOUTS = ("aligned", "all_off1", "grad_off1", "mom_off1", "mom2_off1", "ema_off1", "one_slot_off1")
ARENAS = ("w", "g", "m", "v", "e")
SENT32 = np.uint32(0xCAFEF00D)       # sentinel words of the fp32 buffer (a negative normal float)
SENT16 = np.uint16(0xA5C3)           # sentinel elements of the pack buffer
GAP32 = 8                            # sentinel floats between slots (and around arenas)
GAP16 = 136                          # sentinel elements between packs (> the widest row of any pack: 128)
WD = 5e-4                            # the weight decay every weight-decay launch uses (the directed block B needs it)
GSCALE = 2.0 ** -7
LR = 2.0 ** -10
MOMENTUM = 0.95
N_DIRECTED = 16


class Row:
    def __init__(self, name, Co=0, Ci=0, taps=0, first=0, n=None, dgr=True, dgr_off8=False, si=None):
        self.name, self.Co, self.Ci, self.taps, self.first = name, Co, Ci, taps, first
        self.mode = -1 if n is not None else 0
        self.n = n if n is not None else Co * Ci * taps
        self.has_dgr = dgr and not first and self.mode == 0
        self.dgr_off8, self.si = dgr_off8, si
        self.tiles = -(-self.n // CHUNK) if self.mode < 0 else (-(-Co // 32)) * (-(-Ci // 32))
        self.off = self.fwd = self.dgr = None


def table_rows():
    rows = [Row("a", 64, 64, 9)]
    rows += [Row(f"b{si}", 32, 32, 1, si=si) for si in range(4)]
    rows += [Row("c", 40, 24, 9), Row("d1", 33, 35, 1), Row("d2", 5, 7, 9), Row("e", 64, 3, 9, first=1),
             Row("f1", 64, 64, 9, dgr=False), Row("f2", 40, 24, 9, dgr=False), Row("g", 64, 64, 9, dgr_off8=True)]
    rows += [Row(f"h{n}", n=n) for n in (1, 255, 4095, 4096, 4097, 2 * 4096 + 3)]
    return rows


class Table:
    """One fp32 buffer holding five arenas (masters, gradients, momentum / first moment, second moment, EMA copy) with
    the same slot offsets in each, one 16-bit buffer holding every pack, and the descriptor rows that point into them.
    Both buffers are assumed to start 16-byte aligned.  Sentinels fill everything between slots and between packs."""

    def __init__(self, layout: str):
        assert layout in LAYOUTS
        self.layout = layout
        self.rows = table_rows()
        self.packed = [r for r in self.rows if r.mode == 0]
        # slots inside an arena: 16-byte aligned starts, sentinel gaps
        off = GAP32
        for r in self.rows:
            off = -(-off // 4) * 4
            r.off = off + (1 if (layout == "one_slot_off1" and r.name == "a") else 0)
            off = r.off + r.n + GAP32
        self.arena_len = -(-off // 4) * 4
        base = 4 + (1 if layout == "all_off1" else 0)
        shift = {"g": "grad_off1", "m": "mom_off1", "v": "mom2_off1", "e": "ema_off1"}
        self.base = {}
        for k, a in enumerate(ARENAS):
            self.base[a] = base + k * (self.arena_len + 4) + (1 if shift.get(a) == layout else 0)
        self.total32 = self.base["e"] + self.arena_len + 8
        self.goff, self.boff, self.voff, self.eoff = (self.base[a] - self.base["w"] for a in ("g", "m", "v", "e"))
        # packs: 16-byte aligned starts (row g's dgrad pack 8 bytes past one), sentinel gaps
        poff = GAP16

        def place(n, off8=False):
            nonlocal poff
            poff = -(-poff // 8) * 8 + (4 if off8 else 0)
            at = poff
            poff += n + GAP16
            return at
        for r in self.packed:
            r.fwd = place(r.Co * 64 if r.first else r.n)
            r.dgr = place(r.n, r.dgr_off8) if r.has_dgr else None
        self.ctx_Co = self.ctx_Ci = 32
        self.fwd2 = place(4 * 32 * 32)
        self.dgr2 = place(4 * 32 * 32)
        self.total16 = -(-poff // 8) * 8
        self.max_tiles = max(r.tiles for r in self.rows)
        self.pack_tiles = max(r.tiles for r in self.packed)
        # every element of every slot, as indices into an arena (concatenated over the rows, in row order)
        self.slot_idx = np.concatenate([np.arange(r.off, r.off + r.n, dtype=np.int64) for r in self.rows])
        self.slot_start = np.cumsum([0] + [r.n for r in self.rows])
        # every pack element the kernel writes: pack buffer index <- arena index
        dst, src = [], []
        for r in self.packed:
            d, s = (layout_first if r.first else layout_fwd)(r.Co, r.Ci, r.taps)
            dst.append(r.fwd + d), src.append(r.off + s)
            if r.has_dgr:
                d, s = layout_dgr(r.Co, r.Ci, r.taps)
                dst.append(r.dgr + d), src.append(r.off + s)
            if r.si is not None:
                d, s = layout_fwd2(r.Co, r.Ci, r.si)
                dst.append(self.fwd2 + d), src.append(r.off + s)
                d, s = layout_dgr2(r.Co, r.Ci, r.si)
                dst.append(self.dgr2 + d), src.append(r.off + s)
        self.pack_dst, self.pack_src = np.concatenate(dst), np.concatenate(src)
        assert np.unique(self.pack_dst).size == self.pack_dst.size
        assert self.pack_dst.min() >= GAP16 and self.pack_dst.max() < self.total16 - GAP16 + 8

    # -- descriptor rows for buffers at these addresses (bytes)
    def desc(self, ptr32: int, ptr16: int, packed_only: bool = False) -> np.ndarray:
        assert ptr32 % 16 == 0 and ptr16 % 16 == 0
        out = []
        for r in (self.packed if packed_only else self.rows):
            w = ptr32 + 4 * (self.base["w"] + r.off)
            if r.mode < 0:
                out.append([w, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0, r.n])
                continue
            ctx = r.si is not None
            out.append([w, ptr16 + 2 * r.fwd, ptr16 + 2 * r.dgr if r.has_dgr else 0, r.Co, r.Ci, r.taps, r.first, 0,
                        ptr16 + 2 * self.fwd2 if ctx else 0, ptr16 + 2 * self.dgr2 if ctx else 0, r.si if ctx else 0,
                        r.n])
        d = np.asarray(out, dtype=np.int64)
        assert d.shape[1] == K_PACK_ROW
        return d

    # -- slot values <-> buffers
    def slots(self, buf32: np.ndarray, arena: str) -> np.ndarray:
        return buf32.view(F32)[self.base[arena] + self.slot_idx]

    def put(self, buf32: np.ndarray, arena: str, values: np.ndarray):
        buf32.view(F32)[self.base[arena] + self.slot_idx] = values

    def row_slice(self, name: str) -> slice:
        k = [r.name for r in self.rows].index(name)
        return slice(int(self.slot_start[k]), int(self.slot_start[k + 1]))

    def packs_of(self, buf32: np.ndarray, prior16: np.ndarray, dt: int) -> np.ndarray:
        """The pack buffer after a launch that packs: every written element is the 16-bit rounding of the master as
        stored in ``buf32``; everything else keeps ``prior16``."""
        out = prior16.copy()
        out[self.pack_dst] = round16(buf32.view(F32)[self.base["w"] + self.pack_src], dt)
        return out

    # -- where a word / element of a buffer lies (for failure messages)
    def regions32(self):
        for a in ARENAS:
            for r in self.rows:
                yield f"{a}:{r.name}", self.base[a] + r.off, r.n

    def regions16(self):
        for r in self.packed:
            yield f"fwd:{r.name}", r.fwd, (r.Co * 64 if r.first else r.n)
            if r.has_dgr:
                yield f"dgr:{r.name}", r.dgr, r.n
        yield "fwd2", self.fwd2, 4096
        yield "dgr2", self.dgr2, 4096

    # -- initial contents
    def initial(self, seed: int = 0):
        """(fp32 buffer as uint32 words, pack buffer as uint16): sentinels everywhere, the slots filled with the
        values of ``initial_values`` (identical in every layout)."""
        vals = initial_values(seed)
        buf = np.full(self.total32, SENT32, dtype=np.uint32)
        for a in ARENAS:
            self.put(buf, a, vals[a])
        return buf, np.full(self.total16, SENT16, dtype=np.uint16)


_VALUES = {}


def directed_masters():
    """Masters exactly on a 16-bit rounding midpoint: fp16 (1 + 2^-11, lower neighbour even; 1 + 2^-10 + 2^-11, lower
    neighbour odd) and bf16 (1 + 2^-8; 1 + 2^-7 + 2^-8), both signs, each once for an update below and once for an
    update above."""
    mags = [1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11, 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8]
    p = np.array([s * m for m in mags for s in (1.0, -1.0) for _ in range(2)], dtype=F32)
    usign = np.array([1.0, -1.0] * 8, dtype=F32)          # sign of g * gscale
    assert p.size == N_DIRECTED
    return p, usign


def initial_values(seed: int = 0):
    """Slot values of the five arenas, concatenated over the table's rows.  Weights N(0, 0.3); in every packed row
    three directed blocks at the start of the slot:

    A  the master is on a 16-bit midpoint, momentum 0, g * gscale = -+2^-20: a plain SGD update of 2^-30, far below
       half an fp32 ulp, so the stored master keeps its value and the coherent pack is the midpoint's even neighbour,
       while a pack rounded from the exact update lands on the other side;
    B  the same under weight decay WD: g * gscale = -fl(WD p) -+ 2^-20, so g' = fma(WD, p, g * gscale) is again
       -+2^-20 up to a residue below 2^-34;
    S  masters between 2^-27 and 2^-14 (fp16 subnormals, the ties 2^-25 and 3 * 2^-25 among them) with small
       gradients, zero momentum and second moments near one, so they stay that small under every optimizer."""
    if seed in _VALUES:
        return _VALUES[seed]
    rows = table_rows()
    rng = np.random.default_rng(1234 + seed)
    n = sum(r.n for r in rows)
    v = {"w": (rng.standard_normal(n) * 0.3).astype(F32),
         "g": rng.standard_normal(n).astype(F32),
         "m": (rng.standard_normal(n) * 0.01).astype(F32),
         "v": (np.abs(rng.standard_normal(n)) * 1e-4 + 1e-8).astype(F32),
         "e": (rng.standard_normal(n) * 0.3).astype(F32)}
    pd, usign = directed_masters()
    start = 0
    for r in rows:
        if r.mode == 0:
            assert r.n >= 3 * N_DIRECTED + 32
            a = slice(start, start + N_DIRECTED)
            b = slice(start + N_DIRECTED, start + 2 * N_DIRECTED)
            s = slice(start + 2 * N_DIRECTED, start + 2 * N_DIRECTED + 32)
            for blk in (a, b):
                v["w"][blk] = pd
                v["m"][blk] = 0
            v["g"][a] = -usign * F32(2.0 ** -20 / GSCALE)
            v["g"][b] = (-mul32(F32(WD), pd) - usign * F32(2.0 ** -20)) / F32(GSCALE)
            sub = np.exp2(rng.uniform(-27, -14, 32)) * rng.choice([-1.0, 1.0], 32)
            sub[:4] = [2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25]
            v["w"][s] = sub.astype(F32)
            v["g"][s] = (rng.standard_normal(32) * 2.0 ** -12 / GSCALE).astype(F32)
            v["g"][s][:4] = 0
            v["m"][s] = 0
            v["v"][s] = rng.uniform(0.5, 2.0, 32).astype(F32)
            v["e"][s] = (np.exp2(rng.uniform(-27, -14, 32)) * rng.choice([-1.0, 1.0], 32)).astype(F32)
        start += r.n
    _VALUES[seed] = v
    return v


def directed_index(table: Table, block: str) -> np.ndarray:
    """Indices (into the concatenated slot values) of directed block 'A', 'B' or 'S' of every packed row."""
    k0, n = {"A": (0, N_DIRECTED), "B": (N_DIRECTED, N_DIRECTED), "S": (2 * N_DIRECTED, 32)}[block]
    out = []
    for r, st in zip(table.rows, table.slot_start):
        if r.mode == 0:
            out.append(np.arange(st + k0, st + k0 + n))
    return np.concatenate(out)


# ------------------------------------------------------------------ one launch on slot values
def apply_launch(vals: dict, kind: str, *, lr=LR, gscale=GSCALE, gmul=None, momentum=MOMENTUM, wd=WD,
                 betas=(0.9, 0.999), eps=1e-8, t=None, ema=False, ema_n=None, ema_decay=0.999, ema_warmup=True):
    """The arenas' slot values after one launch of ``kind`` ('pack', 'sgd', 'sgd_wd', 'adam', 'adamw', 'swap');
    ``vals`` is not modified.  t: Adam steps applied so far; ema_n: EMA updates applied so far."""
    out = dict(vals)
    if kind == "pack":
        return out
    if kind == "swap":
        out["w"], out["e"] = vals["e"], vals["w"]
        return out
    if kind in ("sgd", "sgd_wd"):
        out["w"], out["m"] = sgd_step(vals["w"], vals["g"], vals["m"], lr=lr, momentum=momentum,
                                      gscale=eff_gscale(gscale, gmul), wd=wd if kind == "sgd_wd" else None)
    elif kind in ("adam", "adamw"):
        c = adam_coef(t=t + 1, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, wd=wd, decoupled=kind == "adamw",
                      gscale=gscale, gmul=gmul)
        out["w"], out["m"], out["v"] = adam_step(c, vals["w"], vals["g"], vals["m"], vals["v"])
    else:
        raise ValueError(kind)
    if ema:
        w, _ = ema_coef(n=ema_n, decay=ema_decay, warmup=ema_warmup)
        out["e"] = ema_step(w, out["w"], vals["e"])
    return out


def expected_buffers(table: Table, buf32: np.ndarray, buf16: np.ndarray, dt: int, kind: str, **kw):
    """What both buffers must hold after one launch of ``kind`` on (buf32, buf16): every arena slot from the
    emulation, every pack from the master as stored, every other word unchanged."""
    vals = {a: table.slots(buf32, a) for a in ARENAS}
    new = apply_launch(vals, kind, **kw)
    out32 = buf32.copy()
    for a in ARENAS:
        if new[a] is not vals[a]:
            table.put(out32, a, new[a])
    return out32, table.packs_of(out32, buf16, dt)


def diff_report(table: Table, got32, want32, got16, want16, limit: int = 6) -> str:
    """'' when both buffers match bit for bit, else where they differ: mismatches per region, first few shown."""
    lines = []
    bad = np.flatnonzero(got32 != want32)
    if bad.size:
        seen = np.zeros(bad.size, dtype=bool)
        for name, off, n in table.regions32():
            m = (bad >= off) & (bad < off + n)
            seen |= m
            if m.any():
                i = bad[m][:limit]
                lines.append(f"{name}: {int(m.sum())} of {n} words differ, first at +{[int(k - off) for k in i]} got "
                             f"{[hex(int(x)) for x in got32[i]]} want {[hex(int(x)) for x in want32[i]]}")
        if (~seen).any():
            lines.append(f"fp32 sentinel words overwritten: {int((~seen).sum())}, first at {bad[~seen][:limit].tolist()}")
    bad = np.flatnonzero(got16 != want16)
    if bad.size:
        seen = np.zeros(bad.size, dtype=bool)
        for name, off, n in table.regions16():
            m = (bad >= off) & (bad < off + n)
            seen |= m
            if m.any():
                i = bad[m][:limit]
                lines.append(f"{name}: {int(m.sum())} of {n} pack elements differ, first at "
                             f"+{[int(k - off) for k in i]} got {[hex(int(x)) for x in got16[i]]} want "
                             f"{[hex(int(x)) for x in want16[i]]}")
        if (~seen).any():
            lines.append(f"pack sentinel elements overwritten: {int((~seen).sum())}, first at "
                         f"{bad[~seen][:limit].tolist()}")
    return "\n".join(lines)
