"""Host-side checks of the cost kinds along a path (no GPU): the oracle's along-path gradient is the derivative of its own
float64 hard-DTW value (central differences, the path unchanged by every perturbation); the oracle's runs on hand-made
paths, valid and not; its pair costs against the table oracles on the paths of dtwpath_oracle.dtw64; the wrappers'
argument checks before a library load, and the C entry points' before a device is looked for."""
import numpy as np
import pytest
import torch

import dtwpath_oracle as dpo
import pathcost_oracle as orc

C, N, M, SCALE, H = 3, 12, 15, 0.5, 1e-6


@pytest.mark.parametrize("penalty, band", [(0.0, None), (0.3, 5)])
@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("seed", range(20))
def test_gradient_is_the_finite_difference_of_the_dtw_value(seed, kind, penalty, band):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-1, 1, (C, N)).astype(np.float32).astype(np.float64)
    target = rng.uniform(-1, 1, (C, M)).astype(np.float32).astype(np.float64)
    value, cells = orc.dtw_value64(pred, target, kind, SCALE, penalty, band)
    path = np.array(cells, np.int32)[None]
    length = np.array([len(cells)], np.int32)
    dp, dt, _, _ = orc.grads64(None, pred[None], target[None], path, length, kind=kind, scale=SCALE)
    worst = 0.0
    for x, grad in ((pred, dp[0]), (target, dt[0])):
        for idx in np.ndindex(*x.shape):
            keep = x[idx]
            vals = []
            for sign in (1.0, -1.0):
                x[idx] = keep + sign * H
                v, moved = orc.dtw_value64(pred, target, kind, SCALE, penalty, band)
                assert moved == cells, (seed, kind, penalty, band, idx)     # no perturbed evaluation changes the path
                vals.append(v)
            x[idx] = keep
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * H) - grad[idx]))
    print(f"seed {seed} {kind} p={penalty} w={band}: value {value:.6f}, K = {len(cells)}, max |fd - grad| {worst:.2e}")
    assert worst <= 1e-7


def test_oracle_runs_on_hand_made_paths():
    Nn, Mm = 9, 14
    names, path, length, valid = orc.hand_paths(Nn, Mm)
    rs, rc, cs, cc, ok = orc.runs64(path, length, Nn, Mm)
    assert np.array_equal(ok, valid) and ok.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    at = {name: k for k, name in enumerate(names)}
    b = at["diagonal"]
    assert rs[b].tolist() == list(range(Nn)) and rc[b].tolist() == [1] * Nn
    assert cs[b].tolist() == list(range(Nn)) + [-1] * (Mm - Nn) and cc[b].tolist() == [1] * Nn + [0] * (Mm - Nn)
    b = at["l_shaped"]                       # row 0 across all M columns, then the last column down all N rows
    assert length[b] == Nn + Mm - 1
    assert rs[b].tolist() == [0] + list(range(Mm, Mm + Nn - 1)) and rc[b].tolist() == [Mm] + [1] * (Nn - 1)
    assert cs[b].tolist() == list(range(Mm)) and cc[b].tolist() == [1] * (Mm - 1) + [Nn]
    b = at["staircase"]
    assert length[b] == Nn + Mm - 1 and rc[b].sum() == length[b] and cc[b].sum() == length[b]
    assert rc[b, :Nn - 1].tolist() == [2] * (Nn - 1) and (rs[b, 1:] == rs[b, :-1] + rc[b, :-1]).all()
    assert (cs[b, 1:] == cs[b, :-1] + cc[b, :-1]).all() and rs[b, 0] == 0 and cs[b, 0] == 0
    b = at["single_cell"]
    assert rs[b, 0] == 0 and rc[b, 0] == 1 and cs[b, 0] == 0 and cc[b, 0] == 1 and rc[b].sum() == 1 and (rs[b, 1:] == -1).all()
    for name in names[4:]:                   # the invalid ones: no runs at all
        b = at[name]
        assert not rc[b].any() and not cc[b].any() and (rs[b] == -1).all() and (cs[b] == -1).all(), name
    # a 1 x 1 table
    one = orc.runs64(np.zeros((1, 1, 2), np.int32), np.array([1], np.int32), 1, 1)
    assert [a.tolist() for a in one] == [[[0]], [[1]], [[0]], [[1]], [1]]
    # an invalid path has no gradient either
    pred, target = np.ones((len(names), 2, Nn), np.float32), np.zeros((len(names), 2, Mm), np.float32)
    for kind in orc.KINDS:
        dp, dt, bp, bt = orc.grads64(None, pred, target, path, length, kind=kind)
        assert not dp[4:].any() and not dt[4:].any() and not bp[4:].any() and not bt[4:].any()
        assert dp[:4].any() and dt[:4].any()


@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name", ["edges", "band30", "scaled", "ties"])
def test_oracle_pair_cost_is_the_table_at_the_pairs(name, kind):
    c, pred, target = orc._base(name)
    table = orc.table64(kind, pred, target, c.n, c.m, c.band, c.scale)
    _, path, length = dpo.dtw64(orc.table32(kind, pred, target, c.n, c.m, c.band, c.scale), c.n, c.m, 0.05, c.band)
    pair, total, mean = orc.pair_cost64(pred, target, path, length, c.n, c.m, kind, c.scale)
    assert (length > 0).any()
    for b in range(c.B):
        K = int(length[b])
        ij = path[b, :K].astype(np.int64)
        assert np.array_equal(pair[b, :K], table[b, ij[:, 0], ij[:, 1]]) and not pair[b, K:].any()
        if K:
            assert total[b] == pair[b, :K].sum() and mean[b] == total[b] / K and np.isfinite(total[b])
        else:
            assert total[b] == np.inf and mean[b] == np.inf
    # a pair outside the lengths costs +inf, and so does its utterance
    ns = orc.lengths(c.n, c.B, c.N)
    b = int(np.argmax(length > 0))
    bad = path.copy()
    bad[b, 0, 0] = ns[b]
    pair, total, _ = orc.pair_cost64(pred, target, bad, length, c.n, c.m, kind, c.scale)
    assert pair[b, 0] == np.inf and total[b] == np.inf


def _loads(monkeypatch):
    from aligner_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_gpu", no_load)


def test_wrappers_reject_before_a_library_load(monkeypatch):
    import aligner_amd
    _loads(monkeypatch)
    p, t = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
    path, length = torch.zeros(2, 8, 2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    calls = [
        lambda: aligner_amd.path_cost(p[0], t, path, length),                                   # wrong ranks
        lambda: aligner_amd.path_cost(p, t[0], path, length),
        lambda: aligner_amd.path_cost(p, torch.zeros(2, 4, 5), path, length),                   # unequal C
        lambda: aligner_amd.path_cost(p, t, path[:, :, :1], length),                            # path not [B,L,2]
        lambda: aligner_amd.path_cost(p, t, path[0], length),
        lambda: aligner_amd.path_cost(p, t, path.float(), length),
        lambda: aligner_amd.path_cost(p, t, path[:1], length[:1]),                              # another batch size
        lambda: aligner_amd.path_cost(p, t, path, length[:1]),
        lambda: aligner_amd.path_cost(p, t, path, length, kind="cosine"),                       # an unknown kind
        lambda: aligner_amd.path_cost(p, t, path, length, scale=float("nan")),
        lambda: aligner_amd.path_cost(p, t, path, length),                                      # CPU tensors
        lambda: aligner_amd.path_cost_backward(None, p, t, path, length, kind="l3"),
        lambda: aligner_amd.path_cost_backward(torch.zeros(2, 7), p, t, path, length),          # pair_weight not [B,L]
        lambda: aligner_amd.path_cost_backward(None, p, t, path, length, row_scale=torch.zeros(3)),
        lambda: aligner_amd.path_cost_backward(None, p, t, path, length),                       # CPU tensors
        lambda: aligner_amd.path_runs(path[:, :, :1], length, 4, 5),
        lambda: aligner_amd.path_runs(path, length[:1], 4, 5),
        lambda: aligner_amd.path_runs(path, length, -1, 5),
        lambda: aligner_amd.path_runs(path, length, 4, 5),                                      # a CPU tensor
        lambda: aligner_amd.dtw_l1_loss(p[0], t),
        lambda: aligner_amd.dtw_l1_loss(p, torch.zeros(2, 4, 5)),
        lambda: aligner_amd.dtw_l1_loss(p, t, normalize="frames"),                              # an unknown normalize
        lambda: aligner_amd.dtw_l2_loss(p, t, reduction="median"),
        lambda: aligner_amd.dtw_l2_loss(p, t, warp_penalty=-1.0),
        lambda: aligner_amd.dtw_l2_loss(p, t, bandwidth=-3),
        lambda: aligner_amd.dtw_l1_loss(p, t),                                                  # CPU tensors
        lambda: aligner_amd.mcd_dtw_loss(p, t),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")


def test_c_entry_points_validate_before_any_hip_call(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = torch.zeros(4096, dtype=torch.float32)
    x = buf.data_ptr()
    ok = dict(B=1, C=2, N=4, M=5, L=8)

    def runs(path=x, length=x, outs=(x, x, x, x, x), **kw):
        s = dict(ok, **kw)
        return lib.aligner_path_runs(path, length, *outs, s["B"], s["L"], s["N"], s["M"], None)

    def cost(pred=x, target=x, path=x, length=x, pair=x, total=x, kind=0, scale=1.0, **kw):
        s = dict(ok, **kw)
        return lib.aligner_path_cost_f32(pred, target, path, length, None, None, kind, scale, pair, total,
                                         s["B"], s["C"], s["N"], s["M"], s["L"], None)

    def back(pred=x, target=x, path=x, length=x, dpred=x, dtarget=x, ws=x, ws_bytes=1 << 14, kind=0, scale=1.0, **kw):
        s = dict(ok, **kw)
        return lib.aligner_path_cost_backward_f32(None, pred, target, path, length, None, None, kind, scale, None, dpred,
                                                  dtarget, ws, ws_bytes, s["B"], s["C"], s["N"], s["M"], s["L"], None)

    shapes = tuple({k: 0} for k in ok)
    for kw in (dict(path=None), dict(length=None)) + tuple(dict(outs=(x,) * k + (None,) + (x,) * (4 - k)) for k in range(5)):
        assert runs(**kw) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    for kw in (dict(B=0), dict(L=0), dict(N=0), dict(M=0)):
        assert runs(**kw) == _lib.EINVAL, kw
    assert runs(B=65536) == _lib.EDOM and runs(L=1 << 24) == _lib.EDOM
    for kw in (dict(pred=None), dict(target=None), dict(path=None), dict(length=None), dict(pair=None)):
        assert cost(**kw) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    for kw in shapes + (dict(kind=3), dict(kind=-1), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert cost(**kw) == _lib.EINVAL, kw
    for kw in (dict(B=65536), dict(C=4097), dict(L=1 << 24)):
        assert cost(**kw) == _lib.EDOM, kw
    for kw in (dict(pred=None), dict(target=None), dict(path=None), dict(length=None), dict(ws=None), dict(dpred=None, dtarget=None)):
        assert back(**kw) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    for kw in shapes + (dict(kind=3), dict(scale=float("nan"))):
        assert back(**kw) == _lib.EINVAL, kw
    for kw in (dict(B=65536), dict(C=4097), dict(L=1 << 24)):
        assert back(**kw) == _lib.EDOM, kw
    assert back(ws_bytes=16) == _lib.ENOSPC
    # the workspace: the runs, and the root kind's coefficients; 0 outside the domain
    nbytes = lib.aligner_path_cost_backward_workspace_bytes
    assert nbytes(0, 3, 4, 5, 8) == 4 * (2 * 3 * 4 + 2 * 3 * 5 + 3) == nbytes(1, 3, 4, 5, 8)
    assert nbytes(2, 3, 4, 5, 8) == nbytes(0, 3, 4, 5, 8) + 4 * 3 * 8
    assert nbytes(3, 3, 4, 5, 8) == 0 and nbytes(0, 65536, 4, 5, 8) == 0 and nbytes(0, 3, 4, 5, 1 << 24) == 0


def test_empty_shapes_need_no_library(monkeypatch):
    """Empty shapes return before the library is looked for -- on any device, the answers are plain torch."""
    import aligner_amd
    from aligner_amd import pathcost
    _loads(monkeypatch)
    monkeypatch.setattr(pathcost, "one_gpu", lambda named, names: named[0][0].device)
    p, t = torch.zeros(2, 3, 0), torch.zeros(2, 3, 5)
    path, length = torch.full((2, 4, 2), -1, dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)
    pair, total = aligner_amd.path_cost(p, t, path, length)
    assert pair.tolist() == [[0.0] * 4, [float("inf")] * 2 + [0.0] * 2] and torch.isinf(total).all()
    dp, dt = aligner_amd.path_cost_backward(None, p, t, path, length, kind="l2root")
    assert tuple(dp.shape) == (2, 3, 0) and tuple(dt.shape) == (2, 3, 5) and not dt.any()
    assert aligner_amd.path_cost_backward(None, p, t, path, length, want=(False, False)) == (None, None)
