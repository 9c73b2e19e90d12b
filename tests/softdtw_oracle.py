"""Float64 oracle of Soft-DTW (aligner_amd/softdtw.py, csrc/softdtw.hip), an np.float32 restatement of the kernels'
arithmetic, the error bounds of such an evaluation, and the inputs the host and the GPU tests share.

Definition, per utterance with D = cost[:n,:m] (on the fp32 input values, in float64), gamma > 0, penalty p >= 0, band w:

    softmin_g(a,b,c) = -gamma log(exp(-a/gamma) + exp(-b/gamma) + exp(-c/gamma))
    R[i,j] = D[i,j] + softmin_g(R[i-1,j-1], R[i-1,j] + p, R[i,j-1] + p)      R[-1,-1] = 0, every other border cell +inf
    value  = R[n-1,m-1]         E = d value / d D       cell (i,j) exists iff |i - j| <= w; a +inf cost forbids a cell

E is computed "pushed": E[n-1,m-1] = 1 and, from the last anti-diagonal to the first, cell (i,j) hands
E[i,j] w_k / (wa + wb + wc), w_k = exp((mn - pred_k) / gamma), to its three predecessors.  With exact R this is the
gradient (the weights are the softmin's partial derivatives; test_softdtw_host.py checks it against autograd and against
central differences).

Error bounds of an fp32 evaluation in the kernels' form: base-2 logs, x' = x log2(e) / gamma, u = 2^-24, exp2 / log2 /
rcp good to 1 ulp = 2 u.  L = n + m bounds the cells of a path.

  One cell of the forward table, in scaled units.  d' = fl(fl(d) scale), scale itself rounded: 2 u |d'|.  The penalised
  operands fl(pred' + pen'), pen' rounded: 2 u (|pred'| + pen'); a softmin moves by at most the largest move of an operand
  (its partial derivatives are a probability vector), so the two count once: 2 u P', P = the largest |pred| + p among the
  cell's finite operands.  The differences mn - x_k: u |mn - x_k| each, entering log2(s) with weight w_k / s, and
  t 2^-t <= 0.531, one of the three differences is 0 and s >= 1: 1.07 u.  exp2: 2 u of each term, 2 u of s, 2.89 u of
  log2 s.  The two additions: another 2.89 u.  log2 itself: 2 u of a result <= log2 3: 3.17 u.  mn - log2 s: u |sm'|,
  d' + sm': u |R'|.  In natural units (x = x' gamma ln 2; 10.02 ln 2 < 7):

      cell = u (2 |D| + 2 P + |sm| + |R|) + 7 u gamma   <=   u (A + 7 gamma),   A = max over the cells that exist

  value.  An error of the operands passes through a softmin undiminished at most, so the table's error at a cell is at most
  the cell errors along the longest chain to it; the final fl(fin * unscale), unscale rounded: 2 u |value|.

      |value - exact| <= L u (A + 7 gamma) + 2 u |value|                                             (VALUE)

  The host test asserts A <= 5 max|R| + 2 p on every input, so that this stays below 8 L u (max|R| + gamma).

  E, the forward table's share.  The computed table is the exact table of costs moved by at most `cell` each.  E[i,j] is
  the probability that a path drawn with probability ~ exp(-cost / gamma) passes (i,j); moving every path's cost by at most
  d = L cell / gamma turns a probability P into P a / (P a + (1 - P) b), a, b in [e^-d, e^d], which is off by at most
  tanh(d / 2) <= d / 2:  L u (A / (2 gamma) + 3.5).

  E, the backward sweep's share.  A weight 2^(mn - x_k): the operand's 2 u P', the difference's u |mn - x_k| <= u G', G the
  largest gap between two finite operands of a cell: the exponent is off by u (2 P + G) / gamma =: r in natural units, the
  weight by a factor e^+-r, its share w_k / s by e^+-2r.  On top exp2 2 u in w_k and in s, the two additions 2 u, rcp 2 u,
  the two products 2 u, and the two additions that collect a cell's inflow 2 u: 12 u.  A path's probability is a product
  of at most L shares, E a sum of path probabilities:

      |E - exact| <= L u (A / (2 gamma) + 3.5)  +  expm1(L u (2 H / gamma + 12)),   H = max (2 P + G)     (GRAD)

  Both constants come from the operation count above, none from a run of the kernels.  The tests print observed / bound.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
BIG = np.float32(1e30)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def _lengths(t, B, T):
    if t is None:
        return np.full(B, T, np.int64)
    return np.minimum(np.asarray(t, np.int64).reshape(B), T)


def _diag(s, n, m):
    i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
    return i, s - i


def _exists(D, band):
    n, m = D.shape
    i, j = np.mgrid[0:n, 0:m]
    ok = D != np.inf
    if band is not None:
        ok &= np.abs(i - j) <= band
    return ok


def table64(D, gamma, p, band):
    """(R padded by one border row and column, sm) of one utterance in float64; +inf where a cell does not exist."""
    n, m = D.shape
    D = np.where(_exists(D, band), D.astype(np.float64), np.inf)
    R = np.full((n + 1, m + 1), np.inf)
    R[0, 0] = 0.0
    SM = np.full((n, m), np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(n + m - 1):
            i, j = _diag(s, n, m)
            a, b, c = R[i, j], R[i, j + 1] + p, R[i + 1, j] + p
            mn = np.minimum(np.minimum(a, b), c)
            fin = np.isfinite(mn)
            mz = np.where(fin, mn, 0.0)
            sm = mz - gamma * np.log(np.exp((mz - a) / gamma) + np.exp((mz - b) / gamma) + np.exp((mz - c) / gamma))
            sm = np.where(fin, sm, np.inf)
            SM[i, j] = sm
            R[i + 1, j + 1] = D[i, j] + sm
    return R, SM


def push64(R, gamma, p):
    """E of one utterance from its padded table, pushed; zeros without a finite value."""
    n, m = R.shape[0] - 1, R.shape[1] - 1
    E = np.zeros((n + 1, m + 1))
    if not np.isfinite(R[n, m]):
        return E[1:, 1:]
    E[n, m] = 1.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(n + m - 2, -1, -1):
            i, j = _diag(s, n, m)
            a, b, c = R[i, j], R[i, j + 1] + p, R[i + 1, j] + p
            mn = np.minimum(np.minimum(a, b), c)
            fin = np.isfinite(mn) & np.isfinite(R[i + 1, j + 1])
            mz = np.where(fin, mn, 0.0)
            wa, wb, wc = (np.where(fin, np.exp((mz - x) / gamma), 0.0) for x in (a, b, c))
            q = np.where(fin, E[i + 1, j + 1], 0.0) / np.where(fin, wa + wb + wc, 1.0)
            E[i, j] += q * wa
            E[i, j + 1] += q * wb
            E[i + 1, j] += q * wc
    return E[1:, 1:]


def soft_dtw64(cost, n=None, m=None, gamma=1.0, p=0.0, band=None):
    """The oracle: value [B] and E [B,N,M] in float64, and per utterance the magnitudes the bounds are made of."""
    cost = np.asarray(cost)
    B, N, M = cost.shape
    ns, ms = _lengths(n, B, N), _lengths(m, B, M)
    value = np.full(B, np.inf)
    E = np.zeros((B, N, M))
    stats = []
    for b in range(B):
        nb, mb = int(ns[b]), int(ms[b])
        st = SimpleNamespace(n=nb, m=mb, L=max(nb + mb, 2), A=0.0, H=0.0, maxR=0.0, feasible=False)
        stats.append(st)
        if nb < 1 or mb < 1:
            continue
        D = cost[b, :nb, :mb]
        R, SM = table64(D, gamma, p, band)
        value[b] = R[nb, mb]
        st.feasible = bool(np.isfinite(value[b]))
        if not st.feasible:
            continue
        E[b, :nb, :mb] = push64(R, gamma, p)
        Rin = R[1:, 1:]
        ok = np.isfinite(Rin)
        preds = np.stack([R[:-1, :-1], R[:-1, 1:] + p, R[1:, :-1] + p])
        pf = np.isfinite(preds)
        P = np.max(np.where(pf, np.abs(preds), 0.0), axis=0)
        hi = np.max(np.where(pf, preds, -np.inf), axis=0)
        lo = np.min(np.where(pf, preds, np.inf), axis=0)
        G = np.where(pf.any(axis=0), hi - lo, 0.0)
        Dd = np.where(ok, np.abs(D.astype(np.float64)), 0.0)
        st.A = float(np.max(np.where(ok, 2 * Dd + 2 * P + np.abs(np.where(ok, SM, 0.0)) + np.abs(np.where(ok, Rin, 0.0)), 0.0)))
        st.H = float(np.max(np.where(ok, 2 * P + G, 0.0)))
        st.maxR = float(np.max(np.abs(Rin[ok])))
    return value, E, stats


def value_bound(st, value, gamma):
    return st.L * U * (st.A + 7.0 * gamma) + 2.0 * U * abs(value)


def value_cap(st, gamma):
    return 8.0 * st.L * U * (st.maxR + gamma)


def grad_bound(st, gamma):
    return st.L * U * (st.A / (2.0 * gamma) + 3.5) + math.expm1(st.L * U * (2.0 * st.H / gamma + 12.0))


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in np.float32: base 2, the finite sentinel, the same order of operations

def soft_dtw32(cost, n=None, m=None, gamma=1.0, p=0.0, band=None, sabotage=None):
    """value [B] fp32 and E [B,N,M] fp32 as csrc/softdtw.hip computes them (numpy's exp2 / log2 in place of the
    hardware's).  sabotage: None, "no_penalty", "band_plus_one", "gamma_doubled" or "swap_weights" -- the wrong kernels
    the bounds must catch."""
    f = np.float32
    cost = np.asarray(cost, np.float32)
    B, N, M = cost.shape
    ns, ms = _lengths(n, B, N), _lengths(m, B, M)
    if sabotage == "gamma_doubled":
        gamma = 2.0 * gamma
    if sabotage == "band_plus_one" and band is not None:
        band = band + 1
    scale = f(LOG2E / gamma)
    pen = f(0.0) if sabotage == "no_penalty" else f(min(p * (LOG2E / gamma), 1e30))
    unscale = f(gamma * LN2)
    value = np.full(B, np.inf, np.float32)
    E = np.zeros((B, N, M), np.float32)
    for b in range(B):
        nb, mb = int(ns[b]), int(ms[b])
        if nb < 1 or mb < 1 or (band is not None and abs(nb - mb) > band):
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d = np.minimum(np.maximum(cost[b, :nb, :mb] * scale, -BIG), BIG).astype(f)
        i, j = np.mgrid[0:nb, 0:mb]
        exists = np.ones((nb, mb), bool) if band is None else (np.abs(i - j) <= band)
        R = np.full((nb + 1, mb + 1), BIG, f)
        R[0, 0] = 0.0
        for s in range(nb + mb - 1):
            i, j = _diag(s, nb, mb)
            a, bb, c = R[i, j], R[i, j + 1] + pen, R[i + 1, j] + pen
            mn = np.minimum(np.minimum(a, bb), c)
            ssum = (np.exp2(mn - a) + np.exp2(mn - bb)) + np.exp2(mn - c)
            cur = d[i, j] + (mn - np.log2(ssum))
            cur = np.minimum(np.maximum(cur, -BIG), BIG)
            R[i + 1, j + 1] = np.where(exists[i, j], cur, BIG)
        fin = R[nb, mb]
        if not fin < f(0.5) * BIG:
            continue
        value[b] = fin * unscale
        CL = np.zeros((nb + 2, mb + 2), f)          # flow into a cell from (i,j+1), from (i+1,j), from (i+1,j+1)
        CU = np.zeros((nb + 2, mb + 2), f)
        CD = np.zeros((nb + 2, mb + 2), f)
        Eb = np.zeros((nb, mb), f)
        for s in range(nb + mb - 2, -1, -1):
            i, j = _diag(s, nb, mb)
            a, bb, c = R[i, j], R[i, j + 1] + pen, R[i + 1, j] + pen
            mn = np.minimum(np.minimum(a, bb), c)
            wa, wb, wc = np.exp2(mn - a), np.exp2(mn - bb), np.exp2(mn - c)
            inv = f(1.0) / ((wa + wb) + wc)
            e = CL[i + 1, j + 1] + (CU[i + 1, j + 1] + CD[i + 1, j + 1])
            e = np.where((i == nb - 1) & (j == mb - 1), f(1.0), e)
            e = np.where(exists[i, j], e, f(0.0)).astype(f)
            Eb[i, j] = e
            q = e * inv
            if sabotage == "swap_weights":
                wa, wb = wb, wa
            CD[i, j] = q * wa
            CU[i, j + 1] = q * wb
            CL[i + 1, j] = q * wc
        E[b, :nb, :mb] = Eb
    return value, E


# ----------------------------------------------------------------------------------------------------------------------
# the textbook backward, E[i,j] = sum over successors of E[succ] exp((R[succ] - R[i,j] - D[succ] - pen) / gamma), and the
# pushed one, in a given precision on a plain natural-log table: the measurement behind the kernels' choice

def both_backward_forms(D, gamma, dtype):
    """(value, E textbook, E pushed) of one block without band or penalty, every operation in `dtype`."""
    f = dtype
    D = np.asarray(D, f)
    g = f(gamma)
    n, m = D.shape
    inf = f(np.inf)
    R = np.full((n + 2, m + 2), inf, f)
    R[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(n + m - 1):
            i, j = _diag(s, n, m)
            a, b, c = R[i, j], R[i, j + 1], R[i + 1, j]
            mn = np.minimum(np.minimum(a, b), c)
            R[i + 1, j + 1] = D[i, j] + (mn - g * np.log(np.exp((mn - a) / g) + np.exp((mn - b) / g) + np.exp((mn - c) / g)))
        Dp = np.zeros((n + 2, m + 2), f)
        Dp[1:n + 1, 1:m + 1] = D
        Rt = R.copy()
        Rt[n + 1, :] = -inf
        Rt[:, m + 1] = -inf
        Rt[n + 1, m + 1] = R[n, m]
        Et = np.zeros((n + 2, m + 2), f)
        Et[n + 1, m + 1] = 1
        for s in range(n + m - 2, -1, -1):
            i, j = _diag(s, n, m)
            i, j = i + 1, j + 1
            tot = np.zeros(len(i), f)
            for di, dj in ((1, 1), (1, 0), (0, 1)):
                w = np.exp((Rt[i + di, j + dj] - Rt[i, j] - Dp[i + di, j + dj]) / g)
                tot = tot + Et[i + di, j + dj] * np.where(np.isfinite(w), w, f(0))
            Et[i, j] = tot
        Ep = np.zeros((n + 1, m + 1), f)
        Ep[n, m] = 1
        for s in range(n + m - 2, -1, -1):
            i, j = _diag(s, n, m)
            a, b, c = R[i, j], R[i, j + 1], R[i + 1, j]
            mn = np.minimum(np.minimum(a, b), c)
            wa, wb, wc = np.exp((mn - a) / g), np.exp((mn - b) / g), np.exp((mn - c) / g)
            q = Ep[i + 1, j + 1] / (wa + wb + wc)
            Ep[i, j] += q * wa
            Ep[i, j + 1] += q * wb
            Ep[i + 1, j] += q * wc
    return R[n, m], Et[1:n + 1, 1:m + 1], Ep[1:, 1:]


# ----------------------------------------------------------------------------------------------------------------------
# inputs

def uniform_cost(B, N, M, seed):
    """costs uniform in [0, 2]"""
    return np.random.default_rng(seed).uniform(0.0, 2.0, (B, N, M)).astype(np.float32)


def l1_cost(B, N, M, seed, amp=1.0, channels=8):
    """mean |x_i - y_j| over the channels of two random sequences with entries in [0, amp]"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, amp, (B, N, 1, channels))
    y = rng.uniform(0.0, amp, (B, 1, M, channels))
    return np.abs(x - y).mean(axis=3).astype(np.float32)


def _case(name, B, N, M, gamma=1.0, p=0.0, band=None, n=None, m=None, kind="uniform", amp=1.0, blocks=()):
    return SimpleNamespace(name=name, B=B, N=N, M=M, gamma=gamma, p=p, band=band, n=n, m=m, kind=kind, amp=amp, blocks=blocks)


# the smallest shapes at which each mechanism of the kernels can break: rows across the wave (64) and lane edges, columns
# across the tile (16) edges, the largest text, ragged lengths, band and penalty, forbidden blocks.  gamma = 0.1 only
# where n + m <= 230 and on the small-amplitude L1 costs: that is what keeps GRAD at or below 0.05 (asserted on the host).
CASES = (
    [_case(f"rows{N}", 2, N, 40) for N in (1, 2, 63, 64, 65, 127, 129)]
    + [_case(f"cols{M}", 2, 65, M) for M in (1, 15, 16, 17, 33, 130)]
    + [_case("rows65_sharp", 2, 65, 40, gamma=0.1, kind="l1", amp=0.5),
       _case("cols130_sharp", 2, 65, 130, gamma=0.1, p=0.05, kind="l1", amp=0.5),
       _case("rows129_l1", 2, 129, 40, kind="l1", amp=1.0, p=0.2),
       _case("largest_text", 2, 1024, 24, kind="l1", amp=0.25),
       _case("ragged", 6, 65, 130, p=0.3, n=(65, 1, 65, 1, 64, 33), m=(130, 130, 1, 1, 17, 129)),
       _case("band_p0", 4, 100, 127, band=30, p=0.0, n=(97, 60, 90, 100), m=(127, 95, 119, 71)),
       _case("band_p05", 4, 100, 127, band=30, p=0.5, n=(97, 60, 90, 100), m=(127, 95, 119, 71)),
       # utterance 0: a forbidden block with a way round it; utterance 1: two forbidden rows, no path
       _case("forbidden", 2, 33, 40, blocks=((0, slice(10, 20), slice(5, 30)), (1, slice(10, 12), slice(0, 40))))]
)
CASE_NAMES = [c.name for c in CASES]


def case_cost(c):
    seed = sum(ord(ch) for ch in c.name) * 7919 + c.N * 31 + c.M
    cost = uniform_cost(c.B, c.N, c.M, seed) if c.kind == "uniform" else l1_cost(c.B, c.N, c.M, seed, c.amp)
    for b, rows, cols in c.blocks:
        cost[b, rows, cols] = np.inf
    return cost


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, cost, value64, E64, stats) of a named case, computed once per process and never modified."""
    c = CASES[CASE_NAMES.index(name)]
    cost = case_cost(c)
    value, E, stats = soft_dtw64(cost, c.n, c.m, c.gamma, c.p, c.band)
    for a in (cost, value, E):
        a.setflags(write=False)
    return c, cost, value, E, stats


def check(name, got_value, got_E, what):
    """Compare fp32 results with the reference inside VALUE and GRAD; prints observed / bound and returns the two largest
    ratios.  Infeasible utterances must be +inf with an all-zero E."""
    c, cost, value, E, stats = reference(name)
    got_value = np.asarray(got_value, np.float64)
    got_E = np.asarray(got_E, np.float64)
    rv = rg = 0.0
    for b, st in enumerate(stats):
        if not st.feasible:
            assert got_value[b] == np.inf, (name, b, got_value[b])
            assert not got_E[b].any(), (name, b)
            continue
        bv, bg = value_bound(st, value[b], c.gamma), grad_bound(st, c.gamma)
        ev = abs(got_value[b] - value[b])
        eg = float(np.max(np.abs(got_E[b] - E[b])))
        rv, rg = max(rv, ev / bv), max(rg, eg / bg)
        print(f"{what} {name}[{b}] n={st.n} m={st.m}: value err {ev:.3e} / bound {bv:.3e} = {ev / bv:.4f};  "
              f"E err {eg:.3e} / bound {bg:.3e} = {eg / bg:.5f}")
    return rv, rg
