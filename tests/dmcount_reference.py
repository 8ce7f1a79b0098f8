"""The DM-Count loss of one sample in plain numpy, as the README's "DM-Count loss" note defines it, with the dense N x M
Gibbs kernel.  Every array and every scalar is of ``dtype``: float64 is the yardstick of tests/test_gpu_dmcount.py,
float32 shows the error an fp32 evaluation of the same recurrence has against it."""
import numpy as np

D8 = 8


def reference(et, pts, reg=10.0, iters=100, ot_weight=0.1, tv_weight=0.01, dtype=np.float64):
    """et [h, w], pts [N, 2] (x, y) in crop pixels -> dict: terms (L_c, L_ot, L_tv), L, g [h, w], K, u, v, a and the
    two sign arguments P - N and a - q / N (None for a sample that has the count term alone)."""
    f = dtype
    h, w = et.shape
    M, N = h * w, len(pts)
    et = et.astype(f).ravel()
    p = np.abs(et)
    P = p.sum(dtype=f)
    Lc, sc = np.abs(f(N) - P), np.sign(P - f(N))
    out = dict(terms=np.array([Lc, 0, 0], dtype=f), L=Lc, g=(np.sign(et) * sc).reshape(h, w), dPN=P - f(N), da=None)
    if N == 0 or P == 0:
        return out
    eps, tiny, den = f(reg), f(1e-16), f(1e-8)
    a, b = p / (P + den), np.full(N, f(1) / f(N))
    ii, jj = np.divmod(np.arange(M), w)
    z = pts.astype(f)
    s = f(2) / f(D8 * max(h, w))
    x, y = (D8 * jj + D8 // 2).astype(f), (D8 * ii + D8 // 2).astype(f)
    A = np.exp(-(((x[None, :] - z[:, :1]) * s) ** 2) / eps)                  # [N, M]: A_nj at cell m = (i, j)
    B = np.exp(-(((y[None, :] - z[:, 1:]) * s) ** 2) / eps)
    K = B * A
    u = np.full(M, f(1) / f(M))
    for _ in range(iters):
        v = b / (K @ u)
        u = a / (K.T @ v)
    beta, alpha = eps * np.log(u + tiny), eps * np.log(v + tiny)
    Lot = a @ beta + b @ alpha
    G = P / (P * P + den) * beta - (p @ beta) / (P * P + den)
    cj = np.clip(np.floor(z[:, 0] / f(D8)).astype(int), 0, w - 1)
    ci = np.clip(np.floor(z[:, 1] / f(D8)).astype(int), 0, h - 1)
    q = np.bincount(ci * w + cj, minlength=M).astype(f)
    da = a - q / f(N)
    r = np.sign(da)
    Ltv = f(N) * np.abs(da).sum(dtype=f)
    dtv = f(N) / (P + den) * (r - a @ r)
    g = np.sign(et) * (sc + f(ot_weight) * G + f(tv_weight) * dtv)
    out.update(terms=np.array([Lc, Lot, Ltv], dtype=f), L=Lc + f(ot_weight) * Lot + f(tv_weight) * Ltv,
               g=g.reshape(h, w), da=da, K=K, u=u, v=v, a=a, P=P, beta=beta, alpha=alpha)
    return out
