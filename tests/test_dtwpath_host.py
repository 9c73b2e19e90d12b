"""The hard-DTW oracle of tests/dtwpath_oracle.py checked on the host -- against brute force over every warping path,
against the float64 Soft-DTW oracle at a small gamma, float32 against float64 -- and the parts of aligner_amd/dtwpath.py
that need no GPU: path_to_dense, the argument checks, empty shapes, the C ABI's new symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

import banddtw_oracle as bo
import dtwpath_oracle as dpo
import softdtw_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [n for n in dpo.DENSE_NAMES + dpo.BAND_NAMES if dpo.CASES[n].N <= 130]


@pytest.mark.parametrize("kind", ["ints", "uniform"])
@pytest.mark.parametrize("w,p", [(None, 0.0), (None, 0.3), (1, 0.0), (2, 0.7)])
def test_oracle_is_the_minimum_over_all_warping_paths(kind, w, p):
    """Every shape with N, M <= 5, three seeds: the oracle's value is the smallest float32 path value (rounding is
    monotone, so the float32 DP returns exactly that), its path is a warping path with that value, and among the
    minimisers it is the one the tie rule picks when walked back from the end."""
    shapes = 0
    for N in range(1, 6):
        for M in range(1, 6):
            paths = dpo.all_paths(N, M, w)
            for seed in range(3):
                rng = np.random.default_rng(1000 * N + 10 * M + seed)
                D = (rng.integers(0, 4, (N, M)) if kind == "ints" else rng.uniform(0, 2, (N, M))).astype(np.float32)
                value, path, length = dpo.dtw_path32(D[None], None, None, p, w)
                if not paths:
                    assert w is not None and abs(N - M) > w
                    assert value[0] == np.inf and length[0] == 0 and (path == -1).all()
                    continue
                costs = [dpo.path32(c, D, p) for c in paths]
                assert value[0] == min(costs)
                dpo.check_path(path[0], length[0], N, M, w, D)
                mine = [tuple(x) for x in path[0, :length[0]]]
                assert mine in paths and dpo.path32(mine, D, p) == value[0]
                v64, p64, k64 = dpo.dtw64(D[None], None, None, p, w)
                assert abs(v64[0] - min(dpo.path_sums(D, np.array(c), len(c), p)[0] for c in paths)) <= 1e-12
                shapes += 1
    assert shapes >= 3 * (25 if w is None else 9)


def test_ties_prefer_the_diagonal_then_the_row_then_the_column():
    """All-zero costs: every path ties.  Walked back from the end the rule takes diagonals first, so the stalls are at
    the start: along the column axis for n < m, along the row axis for n > m."""
    for n, m in ((3, 7), (7, 3), (4, 4)):
        value, path, length = dpo.dtw_path32(np.zeros((1, n, m), np.float32))
        cells = [tuple(x) for x in path[0, :length[0]]]
        stall = [(0, j) for j in range(m - n)] if n < m else [(i, 0) for i in range(n - m)]
        d = max(n, m) - min(n, m)
        assert value[0] == 0 and length[0] == max(n, m)
        assert cells == stall + [(max(n - m, 0) + k, max(m - n, 0) + k) for k in range(min(n, m))], (cells, d)
    # b against c: at (1,1) a = 5, b = R[0,1] = 4 and c = R[1,0] = 4 tie below it, and the move that advances the row
    # (from (0,1)) wins
    value, path, length = dpo.dtw_path32(np.array([[[5, -1], [-1, 0]]], np.float32))
    assert value[0] == 4 and [tuple(x) for x in path[0, :length[0]]] == [(0, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("name", SMALL)
def test_soft_dtw_at_a_small_gamma_brackets_the_hard_value(name):
    """softmin lies in [min - gamma ln 3, min] and at most n + m - 1 cells are on a path:
    hard - gamma ln 3 (n + m - 1) <= soft_dtw64(gamma) <= hard, with 1e-9 relative slack for float64."""
    c, cost, *_ = dpo.reference(name)
    gamma = 1e-2
    hard, _, length = dpo.dtw64(cost, c.n, c.m, c.p, c.w)
    dense = cost if c.w is None else np.where(bo.band_mask(c.N, c.M, c.w)[None], cost, np.float32(np.inf))
    soft, _, stats = orc.soft_dtw64(dense, c.n, c.m, gamma, c.p, c.w)
    ns, ms = dpo.lengths_of(c)
    for b in range(c.B):
        assert (hard[b] == np.inf) == (soft[b] == np.inf) == (not stats[b].feasible)
        if hard[b] == np.inf:
            continue
        slack = 1e-9 * max(1.0, abs(hard[b]))
        lower = hard[b] - gamma * math.log(3.0) * (int(ns[b]) + int(ms[b]) - 1)
        print(f"{name}[{b}]: hard {hard[b]:.6f}, soft {soft[b]:.6f}, lower bound {lower:.6f}")
        assert lower - slack <= soft[b] <= hard[b] + slack


@pytest.mark.parametrize("name", dpo.DENSE_NAMES + dpo.BAND_NAMES)
def test_float32_value_against_float64_inside_the_bound(name):
    """VALUE of the oracle's docstring; the float32 path is a warping path whose float64 sum is inside it as well."""
    c, cost, value, path, length = dpo.reference(name)
    v64, p64, k64 = dpo.dtw64(cost, c.n, c.m, c.p, c.w, c.L)
    ns, ms = dpo.lengths_of(c)
    worst = 0.0
    for b in range(c.B):
        assert (value[b] == np.inf) == (v64[b] == np.inf)
        if value[b] == np.inf:
            assert length[b] == 0 and (path[b] == -1).all()
            continue
        n, m = int(ns[b]), int(ms[b])
        dpo.check_path(path[b], length[b], n, m, c.w, cost[b])
        total, S = dpo.path_sums(cost[b], path[b], length[b], c.p)
        bound = dpo.value_bound(n, m, S)
        err = abs(float(value[b]) - v64[b])
        worst = max(worst, err / bound if bound else float(err > 0))
        print(f"{name}[{b}] n={n} m={m} K={length[b]}: |value32 - value64| {err:.3e} / bound {bound:.3e}")
        assert err <= bound and abs(float(value[b]) - total) <= bound and total >= v64[b] - 1e-9 * max(1.0, abs(v64[b]))
    print(f"{name}: largest observed / bound {worst:.4f}")


def test_the_cases_cover_the_kernels_edges():
    shapes = {(c.B, c.N, c.M, c.w) for c in dpo.DENSE_CASES}
    for want in ((2, 1, 1, None), (2, 1, 40, None), (2, 40, 1, None), (2, 16, 17, None), (2, 65, 80, None), (2, 130, 70, None),
                 (2, 64, 64, 0), (2, 100, 127, 30), (1, 1024, 1030, 40), (2, 33, 40, None)):
        assert want in shapes, want
    assert len(dpo.BAND_NAMES) == 2 * len(bo.CASES)
    c, cost, value, path, length = dpo.reference("d100x127_w30")
    assert value[0] == np.inf and length[0] == 0 and length[1] == 20          # |n - m| > w; a length of 1
    c, cost, value, path, length = dpo.reference("forbidden")
    assert np.isinf(cost).any() and np.isfinite(value[0]) and value[1] == np.inf
    for name in ("ints65x80", "ints130x70", "zeros"):
        assert set(np.unique(dpo.reference(name)[1])) <= {0.0, 1.0, 2.0, 3.0}


def test_path_to_dense_round_trips():
    import aligner_amd
    for name in ("d16x17", "d100x127_w30_ragged", "zeros"):
        c, cost, value, path, length = dpo.reference(name)
        dense = aligner_amd.path_to_dense(torch.from_numpy(path.copy()), torch.from_numpy(length.copy()), c.N, c.M)
        assert dense.shape == (c.B, c.N, c.M) and dense.dtype == torch.float32
        for b in range(c.B):
            cells = torch.nonzero(dense[b]).numpy()                          # row-major: ascending along a warping path
            assert np.array_equal(cells, path[b, :length[b]]) and set(np.unique(dense[b].numpy())) <= {0.0, 1.0}
            assert dense[b].sum() == length[b]
    with pytest.raises(ValueError, match="B,L,2"):
        aligner_amd.path_to_dense(torch.zeros(2, 5, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 3, 3)
    with pytest.raises(ValueError, match="one entry per utterance"):
        aligner_amd.path_to_dense(torch.zeros(2, 5, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 3, 3)


def test_argument_checks():
    import aligner_amd
    c = torch.zeros(2, 3, 4)
    for bad in (dict(warp_penalty=-1.0), dict(warp_penalty=float("inf")), dict(warp_penalty=float("nan")), dict(bandwidth=-1)):
        with pytest.raises(ValueError):
            aligner_amd.dtw_path(c, **bad)
    with pytest.raises(ValueError, match="B,N,M"):
        aligner_amd.dtw_path(c[0])
    with pytest.raises(ValueError, match="floating"):
        aligner_amd.dtw_path(c.long())
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.dtw_path(c)
    cb = torch.zeros(2, 3, 5)
    for bad in (dict(warp_penalty=-1.0), dict(warp_penalty=float("inf"))):
        with pytest.raises(ValueError):
            aligner_amd.dtw_path_banded(cb, **bad)
    with pytest.raises(ValueError, match="odd"):
        aligner_amd.dtw_path_banded(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="B,N,W"):
        aligner_amd.dtw_path_banded(cb[0])
    with pytest.raises(ValueError, match="at most 127"):
        aligner_amd.dtw_path_banded(torch.zeros(1, 3, 257))
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.dtw_path_banded(cb)
    pred, target = torch.zeros(2, 4, 6), torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.dtw_path_l1(pred, target, bandwidth=2)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.dtw_path_l1(pred, target)
    with pytest.raises(ValueError, match="disagree"):
        aligner_amd.dtw_path_l1(pred, target[:, :3])


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is a GPU tensor: empty shapes return before anything looks closer."""
    is_cuda = property(lambda self: True)


def test_empty_shapes_return_without_a_library_load(monkeypatch):
    import aligner_amd
    from aligner_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_gpu", no_load)
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        r = aligner_amd.dtw_path(torch.zeros(shape).as_subclass(_OnGpu))
        assert torch.isinf(r.value).all() and r.value.shape == (shape[0],) and not r.length.any()
        assert r.path.shape == (shape[0], max(shape[1] + shape[2] - 1, 0), 2) and (r.path == -1).all()
        assert aligner_amd.dtw_path(torch.zeros(shape).as_subclass(_OnGpu), want_path=False).path is None
    for shape in ((0, 3, 5), (2, 0, 5)):
        r = aligner_amd.dtw_path_banded(torch.zeros(shape).as_subclass(_OnGpu))
        assert torch.isinf(r.value).all() and not r.length.any() and r.path.shape == (shape[0], 2 * shape[1] + 1, 2)


def test_the_new_symbols_are_declared_and_bound(built_lib):
    from aligner_amd import _lib
    with open(os.path.join(ROOT, "include", "aligner_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("aligner_dtw_path_workspace_bytes", "aligner_dtw_path_f32", "aligner_dtw_path_banded_workspace_bytes",
                 "aligner_dtw_path_banded_f32"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(built_lib, name)
    assert "#define ALIGNER_ABI_VERSION 5" in header and built_lib.aligner_abi_version() == 5
    # validated before any HIP call
    assert built_lib.aligner_dtw_path_workspace_bytes(2, 100, 100) == 20224
    assert built_lib.aligner_dtw_path_workspace_bytes(2, 1025, 100) == 0
    assert built_lib.aligner_dtw_path_banded_workspace_bytes(2, 5000, 60) == 2 * 5000 * 121 + (-2 * 5000 * 121) % 256
    assert built_lib.aligner_dtw_path_banded_workspace_bytes(2, 100, 128) == 0
    assert built_lib.aligner_dtw_path_f32(None, None, None, 0.0, -1, None, None, None, None, 0, 1, 4, 4, None) == _lib.EINVAL
    assert built_lib.aligner_dtw_path_banded_f32(1, None, None, 0.0, 200, 1, None, None, None, 0, 1, 4, None) == _lib.EDOM
