"""Float64 oracle of the Euclidean cost tables and the squared cost's gradient (aligner_amd/l2cost.py; csrc/l1cost.hip
and csrc/banddtw.hip on the kinds of csrc/costkind.h), the error bounds of an fp32 evaluation, and the MCD-DTW mean.
The inputs are those of tests/l1cost_oracle.py (CASES, inputs(), exists(), lengths()): the tiles are the L1 kernels'.

Definition, on the fp32 input values in float64, with the existing cells of l1cost_oracle (i < n, j < m, |i - j| <= w):

    S[b,i,j]       = sum_c (pred[b,c,i] - target[b,c,j])^2
    squared cost   = scale S          root cost = scale sqrt(S)           on existing cells
                   = +inf where i < n, j < m, |i - j| > w;  0 at or past n or m
    dpred[b,c,i]   =  2 g[b] scale sum_j G[b,i,j] (pred[b,c,i] - target[b,c,j])      over the existing cells of row i
    dtarget[b,c,j] = -2 g[b] scale sum_i G[b,i,j] (pred[b,c,i] - target[b,c,j])      over the existing cells of column j

G is read on existing cells only.  The root has no gradient.

Error bounds, u = 2^-24, inputs exactly representable in fp32, no overflow or underflow.  k roundings in a row give a
factor within gamma_k = k u / (1 - k u) of 1, and gamma_k <= (k + 1) u while k (k + 1) u <= 1, i.e. k <= 4095 (asserted
where the bounds are built).  What is counted is the kernels' text: d = t - p; acc = fma(d, d, acc), channels in order.

  squared cost.  d_c = fl(t - p) carries one rounding and enters the term squared: two factors.  The product d_c d_c is
  exact inside the fused operation, whose result is rounded once; the term of channel c is inside the roundings of
  channels c .. C - 1, at most C of them.  All terms are non-negative, so the factors of the terms bound the factor of
  the sum.  scale is rounded to fp32 once and the product with it once.  2 + C + 2 = C + 4 roundings:

      |cost - exact| <= (C + 5) u exact                                                                  (SQUARED)

  root cost.  Before the root the sum is inside C + 2 roundings, a factor (1 + u)^(C + 2) at most; the square root of
  that factor is (1 + u)^((C + 2) / 2).  The root itself: one rounding when it is correctly rounded, which is what the
  compiled code shows (the hardware estimate followed by the two correction steps of the compiler's
  IEEE expansion); the bound allows two, so that it would also hold for a root a unit off.  scale and the product
  with it: two more.  C / 2 + 1 + 2 + 2 = C / 2 + 5 roundings, gamma <= (C / 2 + 6) u:

      |cost - exact| <= (C / 2 + 6) u exact                                                              (ROOT)

  gradient.  A term is fma(G, d, acc) with d = fl(p - t): one rounding in d, one in the term's own fused operation,
  and then at most K - 1 additions of two non-zero partial sums in any order over the K existing cells -- a cell that
  does not exist contributes fma(+0, d, acc) = acc exactly (G is masked to +0 there and d is finite), and a lane or a
  row block without cells an exact 0.  k = fl(fl(2 scale) g): 2 scale is exact once scale is rounded, so two roundings;
  the final product one.  1 + 1 + (K - 1) + 2 + 1 = K + 4 roundings; the terms have both signs, so the bound is on
  the sum of their magnitudes:

      |d - exact| <= (K + 5) u |2 scale g[b]| sum |G| |pred - target|     over the K existing cells      (GRAD)

  per element [B,C,N] / [B,C,M] (the magnitudes depend on the channel), and exactly 0 where the row / column has no
  existing cell.

  MCD.  mcd[b] = (1 / K) sum of the root cost (scale 10 sqrt(2) / ln 10) over the K cells of the path.  Each cell is
  inside ROOT; the K non-negative costs are added in fp32 in some order, a term passing through at most K - 1
  additions; K is exact in fp32 (K < 2^24) and the division rounds once.  C / 2 + 5 + (K - 1) + 1 roundings,
  gamma <= (C / 2 + 6 + K) u, inside the constant the tests use:

      |mcd - exact| <= (C / 2 + 6 + K + 2) u exact     on a fixed path                                   (MCD)

All constants come from the operation count, none from a run of the kernels.  The checks print observed / bound.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import l1cost_oracle as l1o
from l1cost_oracle import CASES, CASE_NAMES, U, exists, inputs, lengths  # noqa: F401

MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)


def cost_constant(C, squared):
    """The constant of SQUARED or ROOT, in units of u."""
    k = C + 4 if squared else C / 2 + 5
    assert k <= 4095
    return k + 1


def cost64(pred, target, n=None, m=None, band=None, scale=1.0, squared=True):
    """cost [B,N,M] float64 with its fill values."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, inside = exists(B, N, M, n, m, band)
    S = ((pred.astype(np.float64)[:, :, :, None] - target.astype(np.float64)[:, :, None, :]) ** 2).sum(1)
    d = (S if squared else np.sqrt(S)) * float(scale)
    return np.where(ok, d, np.where(inside, np.inf, 0.0))


def grads64(G, pred, target, n=None, m=None, band=None, scale=1.0, row_scale=None):
    """(dpred [B,C,N], dtarget [B,C,M], bound_pred [B,C,N], bound_target [B,C,M]) in float64: the gradients of the squared
    cost and the bound GRAD of each element (0 where the row / column has no existing cell)."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, _ = exists(B, N, M, n, m, band)
    g = np.ones(B) if row_scale is None else np.asarray(row_scale, np.float64).reshape(B)
    Gz = np.where(ok, G.astype(np.float64), 0.0)[:, None]                                                # [B,1,N,M]
    d = pred.astype(np.float64)[:, :, :, None] - target.astype(np.float64)[:, :, None, :]               # [B,C,N,M]
    k = (2.0 * float(scale) * g)[:, None, None]
    dpred = k * (Gz * d).sum(3)
    dtarget = -k * (Gz * d).sum(2)
    mag = np.abs(Gz) * np.abs(d)
    Kr, Kc = ok.sum(2), ok.sum(1)                                       # existing cells per row, per column
    assert max(Kr.max(), Kc.max()) + 4 <= 4095
    bp = (Kr[:, None, :] + 5) * U * np.abs(k) * mag.sum(3) * (Kr[:, None, :] > 0)
    bt = (Kc[:, None, :] + 5) * U * np.abs(k) * mag.sum(2) * (Kc[:, None, :] > 0)
    return dpred, dtarget, bp, bt


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, pred, target, G, squared cost64, root cost64, dpred64, dtarget64, bound_pred, bound_target), once per case;
    pred, target and G (NaN at every cell that does not exist) are l1cost_oracle's."""
    c, pred, target, G = l1o.reference(name)[:4]
    sq = cost64(pred, target, c.n, c.m, c.band, c.scale, True)
    rt = cost64(pred, target, c.n, c.m, c.band, c.scale, False)
    dp, dt, bp, bt = grads64(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    for a in (sq, rt, dp, dt, bp, bt):
        a.setflags(write=False)
    return c, pred, target, G, sq, rt, dp, dt, bp, bt


def cost_ratio(got, want, ok, C, squared):
    """Largest |got - want| / bound over the cells `ok`; the elements outside them must be equal exactly."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got[~ok], want[~ok]), "a fill value of the cost is not exact"
    if not ok.any():
        return 0.0
    err, bound = np.abs(got[ok] - want[ok]), cost_constant(C, squared) * U * np.abs(want[ok])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def check_cost(name, got, squared, what):
    """Largest |got - exact| / bound over the existing cells of a case (printed); the fill values must be exact."""
    c, _, _, _, sq, rt, *_ = reference(name)
    ok, inside = exists(c.B, c.N, c.M, c.n, c.m, c.band)
    ratio = cost_ratio(got, sq if squared else rt, ok, c.C, squared)
    print(f"{name} ({what}): {'squared' if squared else 'root'} cost error / bound {ratio:.3f} over {int(ok.sum())} cells, "
          f"{int((inside & ~ok).sum())} cells +inf, {int((~inside).sum())} cells 0")
    return ratio


def grad_ratios(name, dpred, dtarget, expect, what):
    """Largest |got - exact| / bound of each gradient against expect = (dpred64, dtarget64, bound_pred, bound_target)
    (printed); exactly 0 where no cell exists."""
    out = []
    for label, got, want, bound in (("dpred", dpred, expect[0], expect[2]), ("dtarget", dtarget, expect[1], expect[3])):
        if got is None:
            out.append(0.0)
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape == bound.shape
        none = bound == 0
        err = np.abs(got - want)
        # (bound 0 with cells: every |G| |d| of the row is 0, and then so is every term)
        assert not err[none].any() and not got[none].any(), f"{name}: {label} is not exactly 0 where it must be"
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        ratio = float(r.max()) if r.size else 0.0
        print(f"{name} ({what}): {label} error / bound {ratio:.3f}, largest |{label}| {np.abs(want).max() if want.size else 0:.3e}, "
              f"{int(none.sum())} of {none.size} elements with bound 0")
        out.append(ratio)
    return tuple(out)


def check_grads(name, dpred, dtarget, what, expect=None):
    return grad_ratios(name, dpred, dtarget, expect if expect is not None else reference(name)[6:], what)


def cost32(pred, target, n=None, m=None, band=None, scale=1.0, squared=True):
    """The cost in fp32 numpy, unfused, channels added in order: one rounding more per channel than the kernels."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, inside = exists(B, N, M, n, m, band)
    acc = np.zeros((B, N, M), np.float32)
    for ch in range(C):
        d = target[:, ch, None, :] - pred[:, ch, :, None]
        acc = acc + d * d
    acc = (acc if squared else np.sqrt(acc)) * np.float32(scale)
    return np.where(ok, acc, np.where(inside, np.float32(np.inf), np.float32(0)))


def grads32(G, pred, target, n=None, m=None, band=None, scale=1.0, row_scale=None):
    """The gradients in fp32 numpy, unfused, cells added in index order."""
    B, C, N = pred.shape
    M = target.shape[2]
    ok, _ = exists(B, N, M, n, m, band)
    g = np.ones(B, np.float32) if row_scale is None else np.asarray(row_scale, np.float32).reshape(B)
    k = ((np.float32(2) * np.float32(scale)) * g)[:, None, None]
    Gz = np.where(ok, G, np.float32(0))[:, None]
    term = (Gz * (pred[:, :, :, None] - target[:, :, None, :])).astype(np.float32)
    dp = np.zeros((B, C, N), np.float32)
    for j in range(M):
        dp = dp + term[:, :, :, j]
    dt = np.zeros((B, C, M), np.float32)
    for i in range(N):
        dt = dt + term[:, :, i, :]
    return dp * k, dt * -k


def mcd64(pred, target, path, length):
    """[B] float64: the mean of (10 sqrt 2 / ln 10) sqrt(sum_c d_c^2) over each utterance's path cells; +inf for a
    length of 0."""
    out = np.full(len(length), np.inf)
    for b, K in enumerate(np.asarray(length)):
        if K > 0:
            ij = np.asarray(path)[b, :K].astype(np.int64)
            d = pred[b].astype(np.float64)[:, ij[:, 0]] - target[b].astype(np.float64)[:, ij[:, 1]]
            out[b] = MCD_SCALE * np.sqrt((d * d).sum(0)).mean()
    return out


def mcd_constant(C, K):
    """The constant of MCD, in units of u."""
    assert C / 2 + 6 + K + 2 <= 4095
    return C / 2 + 6 + K + 2
