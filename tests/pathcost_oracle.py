"""Float64 oracle of the cost kinds along a warping path (aligner_amd/pathcost.py, csrc/pathcost.hip): pair costs, their
total and mean, the runs and the validity of a path, the three gradients along it, a float64 hard DTW of its own for
finite differences, the error bounds of the fp32 kernels, and the paths and inputs the host and the GPU tests share.

Definition, on the fp32 input values in float64, per utterance b with n = n[b], m = m[b] clamped to N, M, a path of
pairs (i_k, j_k), k < K = length[b], and d_k,c = pred[b,c,i_k] - target[b,c,j_k]:

    pair_cost[k]   = scale sum_c |d_k,c|   (l1)      scale sum_c d_k,c^2   (l2)      scale sqrt(sum_c d_k,c^2)   (l2root)
                   = +inf for a pair with i outside [0,n) or j outside [0,m);  0 for k >= K
    total          = sum of the K pair costs, +inf for K <= 0;   mean = total / K
    dpred[c,i]     =  factor sum over the pairs k of row i      of  w_k s(d_k,c)         pairs inside [0,n) x [0,m) only
    dtarget[c,j]   = -factor sum over the pairs k of column j   of  w_k s(d_k,c)
    l1: s = sign(d), factor = scale g     l2: s = d, factor = 2 scale g     l2root: s = d / dist_k, 0 where dist_k = 0,
                                                                            factor = scale g, dist_k = sqrt(sum_c d_k,c^2)

A path is valid iff 0 <= K <= L, every pair k < K lies in [0,N) x [0,M) and every step is (1,1), (1,0) or (0,1); one
that is not has no runs and no gradient.

Error bounds, u = 2^-24, inputs exactly representable in fp32, no overflow or underflow.  k roundings in a row give a
factor within gamma_k = k u / (1 - k u) of 1, and gamma_k <= (k + 1) u while k <= 4095 (asserted where the bounds are
built).  What is counted is the text of csrc/pathcost.hip.

  pair cost.  pc_pair_kernel is the cell's arithmetic of the table kernels (Kind::term over the channels in order from
  0, then Kind::finish), so it takes the cell's bounds: (C + 2) u relative for l1 (l1cost_oracle, COST) and
  l2cost_oracle.cost_constant(C, squared) u relative for the Euclidean kinds (SQUARED, ROOT).

  total and mean.  pc_total_kernel adds the K pair costs in fp32: strided partial sums, then a tree.  A term passes
  through at most K - 1 additions of two non-zero numbers (adding an exact 0 does not round).  With c the cell's count
  of roundings (l1: C + 2; squared: C + 4; root: C / 2 + 5) that is c + K - 1 roundings, and the mean's division one
  more (K < 2^24 is exact in fp32):

      |total - exact| <= (c + K) u sum |pair cost|          |mean - exact| <= (c + K + 1) u sum |pair cost| / K     (TOTAL)

  gradient over a run of R pairs, per element.  pc_run_kernel adds the run's terms in k order from 0 and multiplies the
  finished sum by the factor once; scale is rounded to fp32 once.
    l1      the terms +w, -w or 0 are selected, not computed: R - 1 additions; factor fl(fl(scale) g): 2; the product: 1.
            R + 2 roundings:    |d - exact| <= (R + 3) u |scale g| sum |w|                                      (GRAD1)
    l2      d = fl(p - t): 1; the term's own fma: 1; R - 1 later additions; factor fl(fl(2 scale) g), 2 scale exact: 2;
            the product: 1.  R + 4 roundings:    |d - exact| <= (R + 5) u |2 scale g| sum |w| |d|                 (GRAD2)
    l2root  the coefficient fl(w / dist): the sum under the root is inside C + 2 roundings and the root halves them,
            (C + 2) / 2; the root itself 2 (as ROOT allows; the compiled one needs 1); the division 1.  Then l2's
            arithmetic with the coefficient in place of w: d 1, the fma 1, R - 1 additions; factor fl(fl(scale) g): 2;
            the product: 1.  C / 2 + 4 + R + 4 = C / 2 + R + 8 roundings:
                                |d - exact| <= (C / 2 + R + 9) u |scale g| sum |w| |d| / dist                     (GRADR)
  and exactly 0 where the row or column has no pair inside the lengths, whatever g is.  All constants come from the
  operation count, none from a run of the kernels.  The checks print observed / bound.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import dtwpath_oracle as dpo
import l1cost_oracle as l1o
import l2cost_oracle as l2o
from l1cost_oracle import U, lengths  # noqa: F401

KINDS = ("l1", "l2", "l2root")


def cell_roundings(kind, C):
    """The cell's count of roundings (module text, TOTAL)."""
    return {"l1": C + 2, "l2": C + 4, "l2root": C / 2 + 5}[kind]


def pair_constant(kind, C):
    """The pair cost's constant in units of u: the cell's, from the table oracles."""
    return C + 2 if kind == "l1" else l2o.cost_constant(C, kind == "l2")


def table64(kind, pred, target, n=None, m=None, band=None, scale=1.0):
    """The kind's [B,N,M] float64 table of the table oracles."""
    if kind == "l1":
        return l1o.cost64(pred, target, n, m, band, scale)
    return l2o.cost64(pred, target, n, m, band, scale, squared=(kind == "l2"))


def table32(kind, pred, target, n=None, m=None, band=None, scale=1.0):
    """The same table in fp32 numpy: what a path is found on."""
    if kind == "l1":
        return l1o.cost32(pred, target, n, m, band, scale)
    return l2o.cost32(pred, target, n, m, band, scale, squared=(kind == "l2"))


def _diffs(pred, target, b, ij):
    """d [C,K] float64 of utterance b on the pairs ij [K,2]."""
    return pred[b].astype(np.float64)[:, ij[:, 0]] - target[b].astype(np.float64)[:, ij[:, 1]]


def _over_channels(term):
    """sum over axis 0, the channels added in order (as the table oracles' reduction over a non-contiguous axis does;
    numpy's own .sum(0) takes another order when fancy indexing has left axis 0 the contiguous one)."""
    acc = np.zeros(term.shape[1:])
    for t in term:
        acc = acc + t
    return acc


def _cost_of(kind, d, scale):
    if kind == "l1":
        return _over_channels(np.abs(d)) * float(scale)
    S = _over_channels(d * d)
    return (S if kind == "l2" else np.sqrt(S)) * float(scale)


def pair_cost64(pred, target, path, length, n=None, m=None, kind="l1", scale=1.0):
    """(pair_cost [B,L], total [B], mean [B]) in float64.  A length outside [0,L] is clamped for the pair costs."""
    B, C, N = pred.shape
    M = target.shape[2]
    path = np.asarray(path)
    L = path.shape[1]
    ns, ms = lengths(n, B, N), lengths(m, B, M)
    pair = np.zeros((B, L))
    total, mean = np.full(B, np.inf), np.full(B, np.inf)
    for b in range(B):
        K = int(np.clip(length[b], 0, L))
        if K == 0:
            continue
        ij = path[b, :K].astype(np.int64)
        inside = (ij[:, 0] >= 0) & (ij[:, 0] < ns[b]) & (ij[:, 1] >= 0) & (ij[:, 1] < ms[b])
        pair[b, :K] = np.inf
        if inside.any():
            pair[b, :K][inside] = _cost_of(kind, _diffs(pred, target, b, ij[inside]), scale)
        total[b] = pair[b, :K].sum()
        mean[b] = total[b] / K
    return pair, total, mean


def runs64(path, length, N, M):
    """(row_start [B,N], row_count [B,N], col_start [B,M], col_count [B,M], valid [B]) int32 of the definition."""
    path = np.asarray(path)
    B, L, _ = path.shape
    rs, rc = np.full((B, N), -1, np.int32), np.zeros((B, N), np.int32)
    cs, cc = np.full((B, M), -1, np.int32), np.zeros((B, M), np.int32)
    valid = np.zeros(B, np.int32)
    for b in range(B):
        K = int(length[b])
        if not 0 <= K <= L:
            continue
        ij = path[b, :K].astype(np.int64)
        if not ((ij[:, 0] >= 0) & (ij[:, 0] < N) & (ij[:, 1] >= 0) & (ij[:, 1] < M)).all():
            continue
        if not all(tuple(s) in ((1, 1), (1, 0), (0, 1)) for s in np.diff(ij, axis=0)):
            continue
        valid[b] = 1
        for k, (i, j) in enumerate(ij):
            if rc[b, i] == 0:
                rs[b, i] = k
            if cc[b, j] == 0:
                cs[b, j] = k
            rc[b, i] += 1
            cc[b, j] += 1
    return rs, rc, cs, cc, valid


def grads64(pair_weight, pred, target, path, length, n=None, m=None, kind="l1", scale=1.0, row_scale=None):
    """(dpred [B,C,N], dtarget [B,C,M], bound_pred, bound_target) in float64: the gradients along the path and the bound
    GRAD1 / GRAD2 / GRADR of each element (0 where the row / column has no pair inside the lengths)."""
    B, C, N = pred.shape
    M = target.shape[2]
    path = np.asarray(path)
    ns, ms = lengths(n, B, N), lengths(m, B, M)
    g = np.ones(B) if row_scale is None else np.asarray(row_scale, np.float64).reshape(B)
    valid = runs64(path, length, N, M)[4]
    dp, dt = np.zeros((B, C, N)), np.zeros((B, C, M))
    bp, bt = np.zeros((B, C, N)), np.zeros((B, C, M))
    for b in range(B):
        K = int(length[b])
        if not valid[b] or K == 0:
            continue
        ij = path[b, :K].astype(np.int64)
        w = np.ones(K) if pair_weight is None else np.asarray(pair_weight)[b, :K].astype(np.float64)
        inside = (ij[:, 0] < ns[b]) & (ij[:, 1] < ms[b])
        ij, w = ij[inside], w[inside]
        d = _diffs(pred, target, b, ij)                                     # [C,K']
        if kind == "l1":
            s, factor, mag = np.sign(d), float(scale) * g[b], np.broadcast_to(np.abs(w), d.shape)
        elif kind == "l2":
            s, factor, mag = d, 2.0 * float(scale) * g[b], np.abs(w) * np.abs(d)
        else:
            dist = np.sqrt(_over_channels(d * d))
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.where(dist > 0, d / dist, 0.0)
            factor, mag = float(scale) * g[b], np.abs(w) * np.abs(s)
        term = w * s
        R_row, R_col = np.bincount(ij[:, 0], minlength=N), np.bincount(ij[:, 1], minlength=M)
        extra = {"l1": 3, "l2": 5, "l2root": C / 2 + 9}[kind]
        assert max(R_row.max(initial=0), R_col.max(initial=0)) + extra <= 4095
        for c in range(C):
            dp[b, c] = factor * np.bincount(ij[:, 0], weights=term[c], minlength=N)
            dt[b, c] = -factor * np.bincount(ij[:, 1], weights=term[c], minlength=M)
            bp[b, c] = (R_row + extra) * U * abs(factor) * np.bincount(ij[:, 0], weights=mag[c], minlength=N) * (R_row > 0)
            bt[b, c] = (R_col + extra) * U * abs(factor) * np.bincount(ij[:, 1], weights=mag[c], minlength=M) * (R_col > 0)
        if not np.isfinite(factor):                                          # (a NaN row_scale beside pairs: not a test input)
            raise ValueError("row_scale must be finite where the utterance has pairs")
    return dp, dt, bp, bt


def total_ratios(kind, C, pair64, length, total, mean, what):
    """Largest |got - exact| / bound of total and mean (either may be None) against TOTAL (printed); +inf where the
    oracle has +inf."""
    worst = [0.0, 0.0]
    B, L = pair64.shape
    for b in range(B):
        K = int(np.clip(length[b], 0, L))
        exact = pair64[b, :K].sum() if K > 0 else np.inf
        if not np.isfinite(exact):
            assert (total is None or total[b] == np.inf) and (mean is None or mean[b] == np.inf), (what, b)
            continue
        c = cell_roundings(kind, C)
        assert c + K <= 4095
        mag = np.abs(pair64[b, :K]).sum()
        for x, (got, want, bound) in enumerate(((None if total is None else total[b], exact, (c + K) * U * mag),
                                                (None if mean is None else mean[b], exact / K, (c + K + 1) * U * mag / K))):
            if got is None:
                continue
            err = abs(float(got) - want)
            worst[x] = max(worst[x], 0.0 if err == 0 else err / bound)
    print(f"{what}: total error / bound {worst[0]:.3f}, mean error / bound {worst[1]:.3f}")
    return tuple(worst)


# ----------------------------------------------------------------------------------------------------------------------
# a float64 hard DTW of its own (dtwpath_oracle.dtw64 rounds its costs to fp32 first: no use for a finite difference)

def dtw_value64(pred, target, kind="l1", scale=1.0, p=0.0, w=None):
    """(value, cells) of one utterance pred [C,N], target [C,M]: dtwpath_oracle._table's recurrence and tie rule on the
    float64 costs."""
    d = pred.astype(np.float64)[:, :, None] - target.astype(np.float64)[:, None, :]
    D = _cost_of(kind, d.reshape(d.shape[0], -1), scale).reshape(d.shape[1], d.shape[2])
    R, K = dpo._table(D, p, w, np.float64)
    return float(R[-1, -1]), dpo._backtrack(K, *D.shape)


# ----------------------------------------------------------------------------------------------------------------------
# hand-made paths

def _as_path(cells, L):
    out = np.full((L, 2), -1, np.int32)
    out[:len(cells)] = cells
    return out


def hand_paths(N, M, L=None):
    """(names, path [P,L,2], length [P], valid [P]) on an N x M table: four warping paths with the longest possible runs,
    then the invalid ones.  N, M >= 4."""
    L = N + M - 1 if L is None else L
    diag = [(k, k) for k in range(min(N, M))]
    ell = [(0, j) for j in range(M)] + [(i, M - 1) for i in range(1, N)]
    stair, i, j = [(0, 0)], 0, 0
    while i + 1 < N or j + 1 < M:
        if (len(stair) % 2 == 1 and j + 1 < M) or i + 1 >= N:
            j += 1
        else:
            i += 1
        stair.append((i, j))
    back = diag[:3] + [(1, 2)] + diag[3:]
    jump = diag[:2] + [(3, 2)] + diag[4:]
    at_n = [(i, 0) for i in range(N)] + [(N, 0)]
    negative = [(0, 0), (-1, 1), (0, 2)]
    named = [("diagonal", diag, len(diag), 1), ("l_shaped", ell, len(ell), 1), ("staircase", stair, len(stair), 1),
             ("single_cell", [(0, 0)], 1, 1),
             ("backward_step", back, len(back), 0), ("step_2_1", jump, len(jump), 0), ("index_equal_n", at_n, len(at_n), 0),
             ("negative_index", negative, 3, 0), ("length_past_l", diag, L + 1, 0), ("length_negative", diag, -1, 0)]
    assert all(len(cells) <= L for _, cells, _, _ in named)
    return ([name for name, *_ in named], np.stack([_as_path(cells, L) for _, cells, _, _ in named]),
            np.array([k for *_, k, _ in named], np.int32), np.array([v for *_, v in named], np.int32))


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests: pred / target of l1cost_oracle.CASES and two cases more, paths from the CPU oracle on the
# fp32 costs of `path_kind` (any warping path is a legal input: the kernels do not know optimality)

CASE_NAMES = ["one", "edges", "channels80", "channels129", "tall", "band30", "ties", "scaled", "identical", "long_band"]
PENALTY = 0.05


def _base(name):
    """(case, pred, target) -- l1cost_oracle's, or the two added cases."""
    if name in l1o.CASES:
        c, pred, target, _ = l1o.inputs(name)
        return c, pred, target
    if name == "identical":
        c = l1o._case(2, 4, 70, 70, seed=21)
        pred = np.random.default_rng(c.seed).uniform(-1.0, 1.0, (c.B, c.C, c.N)).astype(np.float32)
        return c, pred, pred.copy()
    assert name == "long_band"
    c = l1o._case(2, 2, 1500, 1490, band=5, n=(1495, 1488), m=(1490, 1490), seed=22)      # (|n - m| <= w)
    rng = np.random.default_rng(c.seed)
    pred = rng.uniform(-1.0, 1.0, (c.B, c.C, c.N)).astype(np.float32)
    target = rng.uniform(-1.0, 1.0, (c.B, c.C, c.M)).astype(np.float32)
    return c, pred, target


def banded(c):
    """The path buffer of this case is the band call's (L = 2 N + w - 1)."""
    return c.N > 1024


@functools.lru_cache(maxsize=None)
def reference(name):
    """SimpleNamespace(c, pred, target, path [B,L,2], length [B], weight [B,L] with NaN at every k >= length), once per
    case and never modified.  The path is dtwpath_oracle's on the fp32 L1 table with the case's band and PENALTY."""
    c, pred, target = _base(name)
    L = 2 * c.N + c.band - 1 if banded(c) else c.N + c.M - 1
    cost = table32("l1", pred, target, c.n, c.m, c.band, c.scale)
    _, path, length = dpo.dtw_path32(cost, c.n, c.m, PENALTY, c.band, L)
    weight = np.random.default_rng(c.seed + 1000).normal(0.0, 1.0, (c.B, L)).astype(np.float32)
    weight[np.arange(L)[None, :] >= length[:, None]] = np.nan
    for a in (pred, target, path, length, weight):
        a.setflags(write=False)
    return SimpleNamespace(c=c, pred=pred, target=target, path=path, length=length, weight=weight, L=L)


@functools.lru_cache(maxsize=None)
def hand_reference():
    """The hand-made paths in `edges`' shapes: utterance p takes pred / target of edges' utterance p % B, full lengths."""
    c, pred, target = _base("edges")
    names, path, length, valid = hand_paths(c.N, c.M)
    pick = np.arange(len(names)) % c.B
    L = path.shape[1]
    weight = np.random.default_rng(77).normal(0.0, 1.0, (len(names), L)).astype(np.float32)
    weight[np.arange(L)[None, :] >= length[:, None]] = np.nan
    out = SimpleNamespace(c=SimpleNamespace(B=len(names), C=c.C, N=c.N, M=c.M, n=None, m=None, band=None, scale=1.0, row_scale=None),
                          names=names, pred=np.ascontiguousarray(pred[pick]), target=np.ascontiguousarray(target[pick]),
                          path=path, length=length, valid=valid, weight=weight, L=L)
    for a in (out.pred, out.target, out.path, out.length, out.valid, out.weight):
        a.setflags(write=False)
    return out


def grad_ratios(label, dpred, dtarget, expect, what):
    """l2cost_oracle.grad_ratios: largest |got - exact| / bound (printed), exactly 0 where the bound is 0."""
    return l2o.grad_ratios(label, dpred, dtarget, expect, what)
