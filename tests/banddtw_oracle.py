"""Cases and helpers of the band-storage Soft-DTW tests (aligner_amd/banddtw.py, csrc/banddtw.hip).  Nothing is derived
here: the references are the float64 oracles of softdtw_oracle.py (on the dense image of the band, +inf outside it) and
l1cost_oracle.py, and the bounds are theirs -- the band kernels run softdtw_cell.h's per-cell arithmetic, the one those
bounds were derived from.

Band storage of bandwidth w: xb[b,i,d] is cell (i, j = i + d - w), W = 2 w + 1.

The DP kernels stage tiles of 32 anti-diagonals (steps s = i + j); lane l owns band columns (d + (w & 1)) >> 1 = l and,
for w > 63, 64 + l.  So the edges are: the last step n + m - 2 at 30, 31, 32, 63, 64 (the `steps*` cases), w = 63 / 64
(64 and 65 cells on an anti-diagonal: one column per lane / two), odd and even w, a band wider than the table, and a
table past the dense kernel's 1024 rows.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import softdtw_oracle as orc


def _case(name, N, M, w, B=2, gamma=1.0, p=0.0, n=None, m=None, hi=2.0, kind="uniform", amp=1.0, blocks=()):
    return SimpleNamespace(name=name, B=B, N=N, M=M, w=w, gamma=gamma, p=p, n=n, m=m, hi=hi, kind=kind, amp=amp, blocks=blocks)


CASES = [
    _case("w0", 40, 40, 0),
    _case("w1", 40, 41, 1, p=0.3),
    _case("w31", 100, 110, 31),
    _case("w32", 100, 110, 32),
    _case("w63", 150, 170, 63),
    _case("w64", 150, 170, 64),
    _case("w127", 270, 300, 127, p=0.1, hi=2.5),
    _case("wide", 5, 3, 127),
    _case("sharp", 65, 80, 20, gamma=0.1, p=0.05, kind="l1", amp=0.5),
    _case("ragged", 100, 127, 30, B=6, p=0.3, n=(97, 1, 100, 1, 60, 100), m=(127, 20, 71, 1, 95, 69)),
    # the dense case of that name: inside w = 12 its block (utterance 0) spans the band and its rows (utterance 1) cut
    # every path, so neither has an alignment; forbidden_round: a block with a way round it inside the band
    _case("forbidden", 33, 40, 12, blocks=((0, slice(10, 20), slice(5, 30)), (1, slice(10, 12), slice(0, 40)))),
    _case("forbidden_round", 33, 40, 12, blocks=((0, slice(10, 15), slice(8, 21)), (1, slice(10, 12), slice(0, 40)))),
    _case("past1024", 1100, 1096, 8, p=0.1, n=(1100, 1031), m=(1096, 1024), hi=2.45),
    # the last anti-diagonal n + m - 2 around the kernels' 32-step tiles
    _case("steps30", 16, 16, 3),
    _case("steps31", 17, 16, 3, p=0.2),
    _case("steps32", 17, 17, 4),
    _case("steps63", 33, 32, 3),
    _case("steps64", 33, 33, 5, p=0.2),
]
CASE_NAMES = [c.name for c in CASES]
DENSE_NAMES = [c.name for c in CASES if c.N <= 1024]


def m_of(c):
    """The column lengths as the band calls need them: band storage does not know M, so None means N there."""
    return tuple(c.m) if c.m is not None else (c.M,) * c.B


def band_mask(N, M, w):
    i, j = np.mgrid[0:N, 0:M]
    return np.abs(i - j) <= w


def to_band(x, w, fill=0.0):
    """numpy dense [B,N,M] -> band [B,N,2w+1]"""
    B, N, M = x.shape
    out = np.full((B, N, 2 * w + 1), fill, x.dtype)
    i = np.arange(N)[:, None]
    j = i + np.arange(2 * w + 1)[None, :] - w
    ok = (j >= 0) & (j < M)
    out[:, ok] = x[:, np.broadcast_to(i, j.shape)[ok], j[ok]]
    return out


def to_dense(xb, M, fill=0.0):
    """numpy band [B,N,W] -> dense [B,N,M]"""
    B, N, W = xb.shape
    w = (W - 1) // 2
    out = np.full((B, N, M), fill, xb.dtype)
    i = np.arange(N)[:, None]
    j = i + np.arange(W)[None, :] - w
    ok = (j >= 0) & (j < M)
    out[:, np.broadcast_to(i, j.shape)[ok], j[ok]] = xb[:, ok]
    return out


def exists_band(c):
    """bool [B,N,W]: the elements of band storage whose cell exists."""
    ns, ms = orc._lengths(c.n, c.B, c.N), orc._lengths(c.m, c.B, c.M)
    i = np.arange(c.N)[None, :, None]
    j = i + np.arange(2 * c.w + 1)[None, None, :] - c.w
    return (i < ns[:, None, None]) & (j >= 0) & (j < ms[:, None, None])


def raw_cost(c):
    """The costs of a case on the whole [B,N,M] table, finite but for the forbidden blocks."""
    seed = sum(ord(ch) for ch in c.name) * 7919 + c.N * 31 + c.M
    if c.kind == "uniform":
        cost = np.random.default_rng(seed).uniform(0.0, c.hi, (c.B, c.N, c.M)).astype(np.float32)
    else:
        cost = orc.l1_cost(c.B, c.N, c.M, seed, c.amp)
    for b, rows, cols in c.blocks:
        cost[b, rows, cols] = np.inf
    return cost


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, raw cost, dense image with +inf outside the band, cost in band storage, value64, E64 dense, stats),
    computed once per process and never modified."""
    c = CASES[CASE_NAMES.index(name)]
    raw = raw_cost(c)
    dense = np.where(band_mask(c.N, c.M, c.w)[None], raw, np.float32(np.inf))
    band = to_band(raw, c.w)
    value, E, stats = orc.soft_dtw64(dense, c.n, c.m, c.gamma, c.p, c.w)
    for a in (raw, dense, band, value, E):
        a.setflags(write=False)
    return c, raw, dense, band, value, E, stats


def check(name, got_value, got_E, what):
    """softdtw_oracle.check() on a band case: fp32 value [B] and dense E [B,N,M] inside VALUE and GRAD; prints
    observed / bound and returns the two largest ratios."""
    c, _, _, _, value, E, stats = reference(name)
    got_value = np.asarray(got_value, np.float64)
    got_E = np.asarray(got_E, np.float64)
    rv = rg = 0.0
    for b, st in enumerate(stats):
        if not st.feasible:
            assert got_value[b] == np.inf, (name, b, got_value[b])
            assert not got_E[b].any(), (name, b)
            continue
        bv, bg = orc.value_bound(st, value[b], c.gamma), orc.grad_bound(st, c.gamma)
        ev = abs(got_value[b] - value[b])
        eg = float(np.max(np.abs(got_E[b] - E[b])))
        rv, rg = max(rv, ev / bv), max(rg, eg / bg)
        print(f"{what} {name}[{b}] n={st.n} m={st.m} w={c.w}: value err {ev:.3e} / bound {bv:.3e} = {ev / bv:.4f};  "
              f"E err {eg:.3e} / bound {bg:.3e} = {eg / bg:.5f}")
    return rv, rg
