"""Float64 oracle of the L1 cost table and its gradient (aligner_amd/l1cost.py, csrc/l1cost.hip), the error bounds of an
fp32 evaluation, and the inputs the host and the GPU tests share.

Definition, on the fp32 input values in float64, with n = n[b], m = m[b] (clamped to N, M) and the band w:

    cell (i,j) of utterance b exists  iff  i < n, j < m, |i - j| <= w
    cost[b,i,j]    = scale sum_c |pred[b,c,i] - target[b,c,j]|       on existing cells
                   = +inf where i < n, j < m, |i - j| > w;  0 at or past n or m
    dpred[b,c,i]   =  g[b] scale sum_j G[b,i,j] sign(pred[b,c,i] - target[b,c,j])      over the existing cells of row i
    dtarget[b,c,j] = -g[b] scale sum_i G[b,i,j] sign(pred[b,c,i] - target[b,c,j])      over the existing cells of column j

sign(0) = 0.  G is read on existing cells only (the oracle replaces it by 0 elsewhere before it multiplies).

Error bounds, u = 2^-24, inputs exactly representable in fp32.  k roundings in a row give a factor within
gamma_k = k u / (1 - k u) of 1, and gamma_k <= (k + 1) u while k (k + 1) u <= 1, i.e. k <= 4095 (asserted below).

  cost.  Each |x - y| is one rounded subtraction (taking the magnitude is exact).  The C terms are added in fp32 in
  some order: a term passes through at most C - 1 additions, all of non-negative numbers, so nothing cancels.  scale
  is rounded to fp32 once and the product with it once.  That is 1 + (C - 1) + 2 = C + 2 roundings at most, the
  issue's constant:

      |cost - exact| <= (C + 2) u exact                                                                  (COST)

  As a first-order count this leaves out (C + 2)^2 u^2 / 2 of exact, 3e-6 of the bound at C = 129.  It is not needed:
  with scale = 1 (every case but `scaled`) the two last roundings do not happen and gamma_C <= (C + 1) u is inside the
  bound with a unit to spare, and for sums and inner products in any order Jeannerod & Rump (2013, "Improved error
  bounds for inner products in floating-point arithmetic") show that k u holds in place of gamma_k as it stands.  The
  host test evaluates the table in fp32 numpy, channels in order (the longest chain), and finds it inside the bound.

  gradient.  The terms +G, -G or 0 are exact (a selection, no product).  Over K existing cells a term passes through
  at most K - 1 additions of two non-zero partial sums in any order -- adding an exact 0 (a cell that does not exist,
  a tie, a lane or a row block without cells) does not round.  k = fl(fl(scale) g) is two roundings, fl(sum k) one:
  K + 2 roundings, and gamma_(K+2) <= (K + 3) u:

      |d - exact| <= (K + 3) u |scale g[b]| sum|G|      over the K existing cells of that row / column     (GRAD)

  and exactly 0 where the row / column has no existing cell.  Both constants come from the operation count, none from
  a run of the kernels.  The tests print observed / bound.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24


def _case(B, C, N, M, n=None, m=None, band=None, scale=1.0, row_scale=None, quantum=None, seed=0):
    return SimpleNamespace(B=B, C=C, N=N, M=M, n=n, m=m, band=band, scale=scale, row_scale=row_scale, quantum=quantum, seed=seed)


# The kernels' tiles: forward 16 rows x 64 columns a wave (64 rows a workgroup); dtarget 64 columns x 8 channels a wave,
# rows in steps of 8; dpred 8 rows x 8 channels a wave, columns in steps of 64.  Every edge is at a multiple of 8, 16 or
# 64, so the sizes below (65, 130, 63, 64, 33, 1; C = 1, 2, 3, 4, 7, 8, 80, 129) straddle them as they stand.
CASES = {
    "one": _case(1, 1, 1, 1, seed=1),
    "edges": _case(6, 3, 65, 130, n=(65, 64, 63, 1, 0, 33), m=(130, 128, 127, 1, 17, 0), seed=2),
    "channels80": _case(2, 80, 70, 90, seed=3),
    "channels129": _case(2, 129, 70, 90, seed=4),                       # 16 chunks of 8 channels and one of 1
    "tall": _case(2, 2, 1024, 40, n=(1024, 1000), m=(40, 33), seed=5),
    "band0": _case(4, 8, 130, 130, n=(130, 95, 130, 64), m=(130, 130, 120, 70), band=0, seed=6),
    "band30": _case(4, 8, 130, 130, n=(130, 95, 130, 64), m=(130, 130, 120, 70), band=30, seed=6),   # utterance 1: |n - m| = 35
    "ties": _case(2, 4, 40, 50, quantum=0.25, seed=7),
    "scaled": _case(3, 7, 70, 66, n=(70, 50, 69), m=(66, 66, 3), band=40, scale=1.0 / 80, row_scale=(0.0, -2.5, 1.0e4), seed=8),
}
CASE_NAMES = list(CASES)


def lengths(t, B, T):
    if t is None:
        return np.full(B, T, np.int64)
    return np.clip(np.asarray(t, np.int64).reshape(B), 0, T)


def exists(B, N, M, n=None, m=None, band=None):
    """bool [B,N,M]: the cells that exist; inside [B,N,M]: i < n and j < m (with or without the band)."""
    n, m = lengths(n, B, N), lengths(m, B, M)
    i, j = np.arange(N)[None, :, None], np.arange(M)[None, None, :]
    inside = (i < n[:, None, None]) & (j < m[:, None, None])
    ok = inside if band is None else inside & (np.abs(i - j) <= band)
    return ok, inside


def cost64(pred, target, n=None, m=None, band=None, scale=1.0):
    """cost [B,N,M] float64 with its fill values."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, inside = exists(B, N, M, n, m, band)
    d = np.abs(pred.astype(np.float64)[:, :, :, None] - target.astype(np.float64)[:, :, None, :]).sum(1) * float(scale)
    return np.where(ok, d, np.where(inside, np.inf, 0.0))


def grads64(G, pred, target, n=None, m=None, band=None, scale=1.0, row_scale=None):
    """(dpred [B,C,N], dtarget [B,C,M], bound_pred [B,1,N], bound_target [B,1,M]) in float64: the gradients and the
    bound GRAD of each element (0 where the row / column has no existing cell)."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, _ = exists(B, N, M, n, m, band)
    g = np.ones(B) if row_scale is None else np.asarray(row_scale, np.float64).reshape(B)
    Gz = np.where(ok, G.astype(np.float64), 0.0)
    s = np.sign(pred.astype(np.float64)[:, :, :, None] - target.astype(np.float64)[:, :, None, :])      # [B,C,N,M]
    k = (float(scale) * g)[:, None, None]
    dpred = k * (Gz[:, None] * s).sum(3)
    dtarget = -k * (Gz[:, None] * s).sum(2)
    absG = np.abs(Gz)
    Kr, Kc = ok.sum(2), ok.sum(1)                                       # existing cells per row, per column
    assert max(Kr.max(), Kc.max()) + 2 <= 4095
    bp = ((Kr + 3) * U * np.abs(k[:, :, 0]) * absG.sum(2))[:, None, :]
    bt = ((Kc + 3) * U * np.abs(k[:, :, 0]) * absG.sum(1))[:, None, :]
    return dpred, dtarget, bp, bt


def inputs(name):
    """(case, pred [B,C,N] fp32, target [B,C,M] fp32, G [B,N,M] fp32 with NaN at every cell that does not exist)."""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    pred = rng.uniform(-1.0, 1.0, (c.B, c.C, c.N))
    target = rng.uniform(-1.0, 1.0, (c.B, c.C, c.M))
    if c.quantum:
        pred, target = np.round(pred / c.quantum) * c.quantum, np.round(target / c.quantum) * c.quantum
    G = rng.normal(0.0, 1.0, (c.B, c.N, c.M)).astype(np.float32)
    ok, _ = exists(c.B, c.N, c.M, c.n, c.m, c.band)
    G[~ok] = np.nan
    return c, pred.astype(np.float32), target.astype(np.float32), G


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, pred, target, G, cost64, dpred64, dtarget64, bound_pred, bound_target), computed once per case."""
    c, pred, target, G = inputs(name)
    assert c.C + 1 <= 4095
    cost = cost64(pred, target, c.n, c.m, c.band, c.scale)
    dp, dt, bp, bt = grads64(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    for a in (pred, target, G, cost, dp, dt, bp, bt):
        a.setflags(write=False)
    return c, pred, target, G, cost, dp, dt, bp, bt


def tie_share(name):
    """Share of (i,j,c) with pred == target among the existing cells."""
    c, pred, target, *_ = reference(name)
    ok, _ = exists(c.B, c.N, c.M, c.n, c.m, c.band)
    tie = (pred[:, :, :, None] == target[:, :, None, :]) & ok[:, None]
    return tie.sum() / (ok.sum() * c.C)


def check_cost(name, got, what):
    """Largest |got - exact| / bound over the existing cells (printed); the fill values must be exact."""
    c, _, _, _, cost, *_ = reference(name)
    ok, inside = exists(c.B, c.N, c.M, c.n, c.m, c.band)
    got = np.asarray(got, np.float64)
    assert got.shape == cost.shape
    assert np.array_equal(got[~ok], cost[~ok]), f"{name}: a fill value of the {what} cost is not exactly +inf / 0"
    ratio = 0.0
    if ok.any():
        err, bound = np.abs(got[ok] - cost[ok]), (c.C + 2) * U * np.abs(cost[ok])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        ratio = float(r.max())
    print(f"{name} ({what}): cost error / bound {ratio:.3f} over {int(ok.sum())} cells, "
          f"{int((inside & ~ok).sum())} cells +inf, {int((~inside).sum())} cells 0")
    return ratio


def check_grads(name, dpred, dtarget, what, expect=None):
    """Largest |got - exact| / bound of each gradient (printed); exactly 0 where no cell exists.  expect: (dpred64,
    dtarget64, bound_pred, bound_target) in place of the case's own (the loss tests feed the GPU's E)."""
    c = CASES[name]
    dp, dt, bp, bt = expect if expect is not None else reference(name)[5:]
    out = []
    for label, got, want, bound in (("dpred", dpred, dp, bp), ("dtarget", dtarget, dt, bt)):
        if got is None:
            out.append(0.0)
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape
        bound = np.broadcast_to(bound, want.shape)
        none = bound == 0
        err = np.abs(got - want)
        assert not err[none].any() and not got[none].any(), f"{name}: {label} is not exactly 0 where no cell exists"
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        ratio = float(r.max()) if r.size else 0.0
        print(f"{name} ({what}): {label} error / bound {ratio:.3f}, largest |{label}| {np.abs(want).max() if want.size else 0:.3e}, "
              f"{int(none.sum())} of {none.size} elements without a cell")
        out.append(ratio)
    return tuple(out)


def cost32(pred, target, n=None, m=None, band=None, scale=1.0):
    """The cost in fp32 numpy, channels added in order (the order with the longest chain): what the bound must cover."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, inside = exists(B, N, M, n, m, band)
    acc = np.zeros((B, N, M), np.float32)
    for ch in range(C):
        acc = acc + np.abs(target[:, ch, None, :] - pred[:, ch, :, None])
    acc = acc * np.float32(scale)
    return np.where(ok, acc, np.where(inside, np.float32(np.inf), np.float32(0)))


def grads32(G, pred, target, n=None, m=None, band=None, scale=1.0, row_scale=None):
    """The gradients in fp32 numpy, cells added in index order."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, _ = exists(B, N, M, n, m, band)
    g = np.ones(B, np.float32) if row_scale is None else np.asarray(row_scale, np.float32).reshape(B)
    k = (np.float32(scale) * g)[:, None, None]
    Gz = np.where(ok, G, np.float32(0))[:, None]
    s = np.sign(pred[:, :, :, None] - target[:, :, None, :])
    term = (Gz * s).astype(np.float32)
    dp = np.zeros((B, C, N), np.float32)
    for j in range(M):
        dp = dp + term[:, :, :, j]
    dt = np.zeros((B, C, M), np.float32)
    for i in range(N):
        dt = dt + term[:, :, i, :]
    return dp * k, dt * -k
