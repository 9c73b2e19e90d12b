"""Oracle, checker and cases of the hard-DTW tests (aligner_amd/dtwpath.py, csrc/dtwpath.hip).

Definition, per utterance with n, m clamped to the table, a warp penalty p >= 0 and an optional band w; cell (i,j)
exists iff i < n, j < m and |i - j| <= w:

    a = R[i-1,j-1]   b = R[i-1,j] + p   c = R[i,j-1] + p                 R[-1,-1] = 0, every other border cell +inf
    best = a, k = 0;  b < best: best = b, k = 1;  c < best: best = c, k = 2            (strict: diagonal, row, column)
    R[i,j] = best + cost[i,j], or +inf if the cell does not exist, the cost is +inf or NaN, or best is +inf
    value = R[n-1,m-1]; the path follows k from (n-1,m-1) to (0,0) and is reported ascending

dtw_path32() is that in np.float32, anti-diagonal by anti-diagonal over the cells that exist: two IEEE additions and two
comparisons per cell, which is all the kernels do, so the GPU must return its bits.  dtw64() is the same recurrence and
tie rule in float64 on the float32 costs; it is used for bounds only.

The float32 value of a fixed path is its costs and penalties added one at a time, at most 2 K <= 2 (n + m - 1)
additions whose partial sums are at most S = sum |cost| + p K in magnitude: off by at most (n + m) 2^-23 S.  Rounding
is monotone, so the float32 DP returns the smallest float32 path value; comparing it with the float64 optimum through
both optimal paths gives, for costs that are not negative (S of the float64 path is then at most S of the float32 one),

    |value32 - value64| <= (n + m) 2^-23 (sum of |cost| on the path + p K)                              (VALUE)

The dense cases straddle the dense kernel's 16-step tile, its 64-row wave, the ring hand-off between waves and the row
limit; the band cases are banddtw_oracle.CASES (its docstring says which edges of the band kernel they straddle), once
with their uniform costs and once with the costs rounded to integers, where every comparison ties somewhere.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import banddtw_oracle as bo
import softdtw_oracle as orc


def _table(D, p, w, f):
    """(R padded by a border row and column, decisions) of one utterance's block D [n,m], every operation in dtype f."""
    n, m = D.shape
    inf = f(np.inf)
    p = f(p)
    R = np.full((n + 1, m + 1), inf, f)
    R[0, 0] = 0
    K = np.zeros((n, m), np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(n + m - 1):
            lo, hi = max(0, s - m + 1), min(n - 1, s)
            if w is not None:                                    # |2 i - s| <= w
                lo, hi = max(lo, (s - w + 1) // 2), min(hi, (s + w) // 2)
            if lo > hi:
                continue
            i = np.arange(lo, hi + 1)
            j = s - i
            a, b, c = R[i, j], R[i, j + 1] + p, R[i + 1, j] + p
            best, k = a.copy(), np.zeros(len(i), np.int8)
            t = b < best
            best[t], k[t] = b[t], 1
            t = c < best
            best[t], k[t] = c[t], 2
            d = D[i, j]
            ok = (d < inf) & (best < inf)                        # (false for a NaN cost)
            R[i + 1, j + 1] = np.where(ok, best + d, inf)
            K[i, j] = k
    return R, K


def _backtrack(K, n, m):
    i, j, cells = n - 1, m - 1, []
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            return cells[::-1]
        k = K[i, j]
        i, j = i - (k != 2), j - (k != 1)
        assert i >= 0 and j >= 0


def _dtw(cost, n, m, p, w, L, f):
    cost = np.asarray(cost)
    B, N, M = cost.shape
    ns, ms = orc._lengths(n, B, N), orc._lengths(m, B, M)
    L = N + M - 1 if L is None else L
    value = np.full(B, np.inf, f)
    path = np.full((B, L, 2), -1, np.int32)
    length = np.zeros(B, np.int32)
    for b in range(B):
        nb, mb = int(ns[b]), int(ms[b])
        if nb < 1 or mb < 1 or (w is not None and abs(nb - mb) > w):
            continue
        R, K = _table(cost[b, :nb, :mb].astype(f), p, w, f)
        value[b] = R[nb, mb]
        if value[b] == np.inf:
            continue
        cells = _backtrack(K, nb, mb)
        length[b] = len(cells)
        path[b, :len(cells)] = cells
    return value, path, length


def dtw_path32(cost, n=None, m=None, p=0.0, w=None, L=None):
    """(value [B] float32, path [B,L,2] int32, length [B] int32) of the definition in np.float32; L: the path buffer's
    length (None: N + M - 1)."""
    return _dtw(np.asarray(cost, np.float32), n, m, p, w, L, np.float32)


def dtw64(cost, n=None, m=None, p=0.0, w=None, L=None):
    """The same recurrence and tie rule in float64 on the float32 costs."""
    return _dtw(np.asarray(cost, np.float32), n, m, p, w, L, np.float64)


def check_path(path, length, n, m, w, cost=None):
    """One utterance's reported path is a warping path: from (0,0) to (n-1,m-1) by steps (1,1), (1,0), (0,1), inside the
    band, through no forbidden cell, max(n,m) <= K <= n+m-1, and exactly -1 past K."""
    K = int(length)
    path = np.asarray(path)
    assert max(n, m) <= K <= n + m - 1, (K, n, m)
    assert (path[K:] == -1).all()
    cells = path[:K].astype(np.int64)
    assert tuple(cells[0]) == (0, 0) and tuple(cells[-1]) == (n - 1, m - 1), (cells[0], cells[-1])
    steps = np.diff(cells, axis=0)
    assert all(tuple(s) in ((1, 1), (1, 0), (0, 1)) for s in steps)
    if w is not None:
        assert (np.abs(cells[:, 0] - cells[:, 1]) <= w).all()
    if cost is not None:
        on = np.asarray(cost)[cells[:, 0], cells[:, 1]]
        assert not (np.isnan(on) | (on == np.inf)).any()


def path_sums(cost, path, length, p):
    """(float64 value of the path: its costs plus p per stall; S = sum |cost| + p K of VALUE)"""
    cells = np.asarray(path)[:int(length)].astype(np.int64)
    on = np.asarray(cost)[cells[:, 0], cells[:, 1]].astype(np.float64)
    stalls = int((np.diff(cells, axis=0).sum(axis=1) == 1).sum())
    return float(on.sum() + p * stalls), float(np.abs(on).sum() + p * len(cells))


def value_bound(n, m, S):
    return (n + m) * 2.0 ** -23 * S


def path32(cells, D, p):
    """The float32 value of a path as the recurrence adds it up: the penalty first, then the cost, cell by cell."""
    f = np.float32
    r = f(D[cells[0]])
    for (i0, j0), (i, j) in zip(cells[:-1], cells[1:]):
        if (i - i0) + (j - j0) == 1:
            r = f(r + f(p))
        r = f(r + f(D[i, j]))
    return r


def all_paths(n, m, w=None):
    """Every warping path of an n x m table inside the band, as lists of cells."""
    out = []

    def walk(i, j, cells):
        if w is not None and abs(i - j) > w:
            return
        cells = cells + [(i, j)]
        if i == n - 1 and j == m - 1:
            out.append(cells)
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, cells)
        if i + 1 < n:
            walk(i + 1, j, cells)
        if j + 1 < m:
            walk(i, j + 1, cells)

    walk(0, 0, [])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# cases

def _dense(name, B, N, M, w=None, p=0.0, n=None, m=None, kind="uniform", blocks=()):
    return SimpleNamespace(name=name, B=B, N=N, M=M, w=w, p=p, n=n, m=m, kind=kind, blocks=blocks, L=N + M - 1)


def _blocks(name):
    return bo.CASES[bo.CASE_NAMES.index(name)].blocks


DENSE_CASES = [
    _dense("d1x1", 2, 1, 1),
    _dense("d1x40", 2, 1, 40),
    _dense("d40x1", 2, 40, 1),
    _dense("d16x17", 2, 16, 17),
    _dense("d65x80", 2, 65, 80),
    _dense("d130x70_p", 2, 130, 70, p=0.3),
    _dense("d64x64_w0", 2, 64, 64, w=0),
    # utterance 0: |n - m| = 31 > w; utterance 1: a length of 1
    _dense("d100x127_w30", 2, 100, 127, w=30, n=(100, 1), m=(69, 20)),
    _dense("d100x127_w30_ragged", 6, 100, 127, w=30, p=0.3, n=(97, 1, 100, 1, 60, 100), m=(127, 20, 71, 1, 95, 69)),
    _dense("d1024x1030_w40", 1, 1024, 1030, w=40),
    _dense("forbidden", 2, 33, 40, blocks=_blocks("forbidden")),
    _dense("forbidden_round", 2, 33, 40, blocks=_blocks("forbidden_round")),
    # ties: every comparison ties somewhere and the tie rule decides the path
    _dense("zeros", 2, 20, 33, kind="zeros", n=(20, 7), m=(33, 33)),
    _dense("ints65x80", 2, 65, 80, kind="ints"),
    _dense("ints130x70", 2, 130, 70, kind="ints"),
]
# banddtw_oracle.CASES in band storage, with their uniform costs and with the costs rounded to integers
BAND_CASES = [SimpleNamespace(name=f"band_{c.name}{suffix}", B=c.B, N=c.N, M=c.M, w=c.w, p=c.p, n=c.n, m=bo.m_of(c), kind=kind,
                              blocks=c.blocks, L=2 * c.N + c.w - 1, source=c)
              for c in bo.CASES for kind, suffix in (("band", ""), ("band_rounded", "_int"))]
CASES = {c.name: c for c in DENSE_CASES + BAND_CASES}
DENSE_NAMES = [c.name for c in DENSE_CASES]
BAND_NAMES = [c.name for c in BAND_CASES]


def case_cost(c):
    """The costs of a case on the whole [B,N,M] table."""
    if c.kind in ("band", "band_rounded"):
        raw = bo.raw_cost(c.source)
        return np.rint(raw) if c.kind == "band_rounded" else raw
    rng = np.random.default_rng(sum(ord(ch) for ch in c.name) * 7919 + c.N * 31 + c.M)
    if c.kind == "uniform":
        cost = rng.uniform(0.0, 2.0, (c.B, c.N, c.M)).astype(np.float32)
    elif c.kind == "ints":
        cost = rng.integers(0, 4, (c.B, c.N, c.M)).astype(np.float32)
    else:
        cost = np.zeros((c.B, c.N, c.M), np.float32)
    for b, rows, cols in c.blocks:
        cost[b, rows, cols] = np.inf
    return cost


def lengths_of(c):
    return orc._lengths(c.n, c.B, c.N), orc._lengths(c.m, c.B, c.M)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, cost [B,N,M], value32, path32 [B,L,2], length32) of a named case, computed once per process and never
    modified.  L is the dense call's N + M - 1, or the band call's 2 N + w - 1 for a band case."""
    c = CASES[name]
    cost = case_cost(c)
    value, path, length = dtw_path32(cost, c.n, c.m, c.p, c.w, c.L)
    for a in (cost, value, path, length):
        a.setflags(write=False)
    return c, cost, value, path, length
