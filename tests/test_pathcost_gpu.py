"""path_cost() / path_runs() / path_cost_backward() and the hard-DTW losses on the GPU against the float64 oracle
(tests/pathcost_oracle.py) inside its derived bounds: pair costs pinned bit for bit to the GPU's own cost tables, runs
exact, gradients of all three kinds with and without weights, the composed path of the parent
(path_to_dense + l*_cost_backward) beside them, determinism, a NaN that stays in its utterance, stores inside their
buffers, and the autograd face.  pair_weight carries a NaN at every k >= length.  Every comparison prints
observed / bound."""
import functools

import numpy as np
import pytest
import torch

import l1cost_oracle as l1o
import l2cost_oracle as l2o
import pathcost_oracle as orc

pytestmark = pytest.mark.gpu

KIND_ARGS = {"l1": ("l1", None), "l2": ("l2", True), "l2root": ("l2", False)}      # kind -> (table family, squared)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(x, dev, dtype=None):
    return None if x is None else torch.tensor(np.asarray(x), dtype=dtype).to(dev)


def _i32(x, dev):
    return _t(x, dev, torch.int32)


def _f32(x, dev):
    return _t(x, dev, torch.float32)


def _ref(name):
    return orc.hand_reference() if name == "hand" else orc.reference(name)


def _operands(name, dev):
    r = _ref(name)
    return (r, _t(r.pred, dev), _t(r.target, dev), _t(r.path, dev), _t(r.length, dev), _i32(r.c.n, dev), _i32(r.c.m, dev),
            _t(r.weight, dev))


def _row_scale(r):
    """The case's own row_scale (`scaled`: 0, a negative, 1e4), or one with both signs; NaN where there is no alignment."""
    rs = np.asarray(r.c.row_scale, np.float32) if r.c.row_scale is not None else np.linspace(-1.5, 2.0, r.c.B).astype(np.float32)
    valid = orc.runs64(r.path, r.length, r.c.N, r.c.M)[4]
    rs = rs.copy()
    rs[(valid == 0) | (r.length <= 0)] = np.nan
    return rs


@functools.lru_cache(maxsize=None)
def _run(name, kind):
    """One GPU run per (case, kind), shared by the tests: (pair, total, dpred, dtarget with weights, dpred, dtarget
    without) as numpy arrays; row_scale is _row_scale()."""
    import aligner_amd
    dev = torch.device("cuda:0")
    r, pred, target, path, length, n, m, weight = _operands(name, dev)
    rs = _f32(_row_scale(r), dev)
    pair, total = aligner_amd.path_cost(pred, target, path, length, n, m, kind, r.c.scale)
    gw = aligner_amd.path_cost_backward(weight, pred, target, path, length, n, m, kind, r.c.scale, rs)
    g1 = aligner_amd.path_cost_backward(None, pred, target, path, length, n, m, kind, r.c.scale, rs)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (pair, total, *gw, *g1))


def _table(kind, pred, target, n, m, band, scale, banded):
    import aligner_amd
    family, squared = KIND_ARGS[kind]
    if family == "l1":
        return aligner_amd.l1_cost_banded(pred, target, n, m, band, scale) if banded else aligner_amd.l1_cost(pred, target, n, m, band, scale)
    if banded:
        return aligner_amd.l2_cost_banded(pred, target, n, m, band, scale, squared=squared)
    return aligner_amd.l2_cost(pred, target, n, m, band, scale, squared=squared)


def _gather(table, path, length, band=None):
    """table[b, i_k, j_k] (band storage: [b, i_k, j_k - i_k + w]) for k < length, 0 beyond."""
    B, L = path.shape[:2]
    on = torch.arange(L, device=path.device).view(1, L) < length.view(B, 1)
    ij = path.long().clamp(min=0)
    i, j = ij[..., 0], ij[..., 1]
    col = j if band is None else j - i + band
    at = table[torch.arange(B, device=path.device).view(B, 1), i, col]
    return torch.where(on, at, torch.zeros_like(at))


# ---- 1. pair costs pinned to the table ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_pair_costs_are_the_tables_cells_and_inside_the_bounds(dev, name, kind):
    import aligner_amd
    r, pred, target, path, length, n, m, _ = _operands(name, dev)
    c = r.c
    pair, total = _run(name, kind)[:2]
    assert pair.shape == (c.B, r.L) and total.shape == (c.B,)
    got = torch.tensor(pair).to(dev)
    if orc.banded(c):
        # band storage, its dense image, and the path of the banded DP on the GPU's own costs
        table = _table(kind, pred, target, n, m, c.band, c.scale, True)
        assert torch.equal(got.view(torch.int32), _gather(table, path, length, c.band).view(torch.int32))
        image = aligner_amd.dense_to_band(_table(kind, pred, target, n, m, c.band, c.scale, False), c.band)
        assert torch.equal(got.view(torch.int32), _gather(image, path, length, c.band).view(torch.int32))
        dp = aligner_amd.dtw_path_banded(table, n, m, orc.PENALTY)
        assert tuple(dp.path.shape) == (c.B, r.L, 2) and int(dp.length.min()) >= min(c.n)
        own, _ = aligner_amd.path_cost(pred, target, dp.path, dp.length, n, m, kind, c.scale)
        assert torch.equal(own.view(torch.int32), _gather(table, dp.path, dp.length, c.band).view(torch.int32))
    else:
        table = _table(kind, pred, target, n, m, c.band, c.scale, False)
        assert torch.equal(got.view(torch.int32), _gather(table, path, length).view(torch.int32))
    pair64, total64, mean64 = orc.pair_cost64(r.pred, r.target, r.path, r.length, c.n, c.m, kind, c.scale)
    on = np.arange(r.L)[None, :] < r.length[:, None]
    assert not pair[~on].any() and np.isfinite(pair[on]).all()                    # exactly 0 past the length
    err, bound = np.abs(pair[on] - pair64[on]), orc.pair_constant(kind, c.C) * orc.U * np.abs(pair64[on])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.where(err == 0, 0.0, err / bound).max()) if on.any() else 0.0
    print(f"{name} {kind}: pair cost error / bound {ratio:.3f} over {int(on.sum())} pairs")
    assert ratio <= 1.0
    mean = (torch.tensor(total) / torch.tensor(r.length).clamp(min=1).float()).numpy()
    rt, rm = orc.total_ratios(kind, c.C, pair64, r.length, total, mean, f"{name} {kind}")
    assert rt <= 1.0 and rm <= 1.0
    assert (total[r.length <= 0] == np.inf).all() and np.isfinite(total[r.length > 0]).all()


@pytest.mark.parametrize("kind", orc.KINDS)
def test_a_pair_outside_the_lengths_costs_inf_and_so_does_its_total(dev, kind):
    import aligner_amd
    r, pred, target, path, length, n, m, _ = _operands("edges", dev)
    pair0, total0 = _run("edges", kind)[:2]
    ns, ms = orc.lengths(r.c.n, r.c.B, r.c.N), orc.lengths(r.c.m, r.c.B, r.c.M)
    bad = path.clone()
    bad[1, 3, 0] = int(ns[1])                # i == n[1] = 64 < N: inside the tensor, outside the utterance
    bad[2, 5, 1] = int(ms[2])                # j == m[2]
    bad[0, 7, 0] = -1
    bad[3, 0, 1] = r.c.M + 5                 # outside the tensor: nothing is read
    pair, total = aligner_amd.path_cost(pred, target, bad, length, n, m, kind, r.c.scale)
    pair, total = pair.cpu().numpy(), total.cpu().numpy()
    want = pair0.copy()
    for b, k in ((1, 3), (2, 5), (0, 7), (3, 0)):
        want[b, k] = np.inf
    assert np.array_equal(pair, want)
    assert (total[:4] == np.inf).all() and np.array_equal(total[4:], total0[4:])
    # a length past the buffer is clamped, one below 0 counts as 0
    odd = length.clone()
    odd[0], odd[1] = r.L + 7, -3
    pair, total = aligner_amd.path_cost(pred, target, path, odd, n, m, kind, r.c.scale)
    assert np.array_equal(pair[0, :int(length[0])].cpu().numpy(), pair0[0, :int(length[0])]) and bool(torch.isinf(pair[0, int(length[0]):]).all())
    assert not pair[1].any() and torch.isinf(total[:2]).all()
    assert np.array_equal(pair[2:].cpu().numpy(), pair0[2:]) and np.array_equal(total[2:].cpu().numpy(), total0[2:])


# ---- 2. path_runs exact ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", orc.CASE_NAMES + ["hand"])
def test_runs_are_the_oracles(dev, name):
    import aligner_amd
    r, _, _, path, length, *_ = _operands(name, dev)
    got = aligner_amd.path_runs(path, length, r.c.N, r.c.M)
    want = orc.runs64(r.path, r.length, r.c.N, r.c.M)
    for label, g, w in zip(got._fields, got, want):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (name, label)
    if name == "hand":
        assert want[4].tolist() == r.valid.tolist() and 0 < want[4].sum() < len(want[4])
        assert int(got.row_count.max()) == r.c.M and int(got.col_count.max()) == r.c.N         # the longest possible runs
    else:
        assert want[4].all() and np.array_equal(want[1].sum(1), np.maximum(r.length, 0))


def test_runs_of_invalid_paths_between_valid_neighbours(dev):
    """Each invalid hand-made path in turn between two copies of a valid one: the neighbours keep their runs."""
    import aligner_amd
    r = orc.hand_reference()
    good = r.names.index("staircase")
    for bad in np.nonzero(r.valid == 0)[0]:
        pick = [good, int(bad), good]
        got = aligner_amd.path_runs(_t(r.path[pick], dev), _t(r.length[pick], dev), r.c.N, r.c.M)
        want = orc.runs64(r.path[pick], r.length[pick], r.c.N, r.c.M)
        assert want[4].tolist() == [1, 0, 1]
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w), r.names[bad]


# ---- 3. path_cost_backward inside the bounds -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name", orc.CASE_NAMES + ["hand"])
def test_gradients_inside_the_bounds(dev, name, kind):
    r = _ref(name)
    c = r.c
    rs = _row_scale(r)
    out = _run(name, kind)
    ns, ms = orc.lengths(c.n, c.B, c.N), orc.lengths(c.m, c.B, c.M)
    for what, weight, (dpred, dtarget) in (("weights", r.weight, out[2:4]), ("unit weights", None, out[4:6])):
        expect = orc.grads64(weight, r.pred, r.target, r.path, r.length, c.n, c.m, kind, c.scale, rs)
        rp, rt = orc.grad_ratios(f"{name} {kind}", dpred, dtarget, expect, what)       # (asserts the exact zeros)
        assert rp <= 1.0 and rt <= 1.0
        assert np.isfinite(dpred).all() and np.isfinite(dtarget).all()                 # none of the NaNs came through
        for b in range(c.B):
            assert not dpred[b, :, ns[b]:].any() and not dtarget[b, :, ms[b]:].any()
            if np.isnan(rs[b]):                                                        # no alignment, a NaN row_scale
                assert not dpred[b].any() and not dtarget[b].any()
    if name in ("hand", "band30", "edges", "scaled"):        # (these have utterances without an alignment)
        assert np.isnan(rs).any()
    if kind == "l1":
        # unit weights: the sum of the signs is an integer, exact in any order, and the product rounds once
        sp, st, _, _ = orc.grads64(None, r.pred, r.target, r.path, r.length, c.n, c.m, "l1", 1.0, None)
        k = (np.float32(c.scale) * np.nan_to_num(rs))[:, None, None]
        assert np.array_equal(out[4], k * sp.astype(np.float32)) and np.array_equal(out[5], k * st.astype(np.float32))
    if name == "identical":                  # d = 0 on every pair and channel, and dist = 0: exactly 0, and finite
        assert not any(x.any() for x in out[2:6])


# ---- 4. against the composed path of the parent ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("name", ["edges", "band30", "scaled", "ties"])
def test_composed_path_and_this_one_both_inside_their_bounds(dev, name, kind):
    """path_to_dense() + l*_cost_backward() and path_cost_backward() against the same float64 gradient, each inside its
    own bound; not bit for bit, the orders of summation differ."""
    import aligner_amd
    r, pred, target, path, length, n, m, _ = _operands(name, dev)
    c = r.c
    rs = np.nan_to_num(_row_scale(r))
    E = aligner_amd.path_to_dense(path, length, c.N, c.M)
    back = aligner_amd.l1_cost_backward if kind == "l1" else aligner_amd.l2_cost_backward
    dp, dt = back(E, pred, target, n, m, None, c.scale, _f32(rs, dev))
    table = l1o if kind == "l1" else l2o
    theirs = table.grads64(E.cpu().numpy(), r.pred, r.target, c.n, c.m, None, c.scale, rs)
    rp, rt = l2o.grad_ratios(f"{name} {kind}", dp.cpu().numpy(), dt.cpu().numpy(),
                             tuple(np.broadcast_to(a, theirs[0].shape if k % 2 == 0 else theirs[1].shape) for k, a in enumerate(theirs)),
                             "composed")
    assert rp <= 1.0 and rt <= 1.0
    mine = orc.grads64(None, r.pred, r.target, r.path, r.length, c.n, c.m, kind, c.scale, rs)
    assert np.allclose(mine[0], theirs[0], rtol=1e-12, atol=1e-12) and np.allclose(mine[1], theirs[1], rtol=1e-12, atol=1e-12)
    g = aligner_amd.path_cost_backward(None, pred, target, path, length, n, m, kind, c.scale, _f32(rs, dev))
    rp, rt = orc.grad_ratios(f"{name} {kind}", g[0].cpu().numpy(), g[1].cpu().numpy(), mine, "along the path")
    assert rp <= 1.0 and rt <= 1.0


# ---- 5. determinism and independence ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name", ["edges", "tall", "hand"])
def test_two_calls_give_the_same_bits_and_each_gradient_alone_too(dev, name, kind):
    import aligner_amd
    r, pred, target, path, length, n, m, weight = _operands(name, dev)
    rs = _f32(_row_scale(r), dev)
    pair0, total0, dpred0, dtarget0 = _run(name, kind)[:4]
    pair, total = aligner_amd.path_cost(pred, target, path, length, n, m, kind, r.c.scale)
    assert np.array_equal(pair.cpu().numpy(), pair0) and np.array_equal(total.cpu().numpy(), total0)
    dpred, dtarget = aligner_amd.path_cost_backward(weight, pred, target, path, length, n, m, kind, r.c.scale, rs)
    assert np.array_equal(dpred.cpu().numpy(), dpred0) and np.array_equal(dtarget.cpu().numpy(), dtarget0)
    only_p, none = aligner_amd.path_cost_backward(weight, pred, target, path, length, n, m, kind, r.c.scale, rs, want=(True, False))
    assert none is None and np.array_equal(only_p.cpu().numpy(), dpred0)
    none, only_t = aligner_amd.path_cost_backward(weight, pred, target, path, length, n, m, kind, r.c.scale, rs, want=(False, True))
    assert none is None and np.array_equal(only_t.cpu().numpy(), dtarget0)


@pytest.mark.parametrize("kind", orc.KINDS)
def test_nan_stays_in_its_utterance(dev, kind):
    import aligner_amd
    r, pred, target, path, length, n, m, weight = _operands("edges", dev)
    rs = _f32(_row_scale(r), dev)
    pair0, total0, dpred0, dtarget0 = _run("edges", kind)[:4]
    bad = pred.clone()
    bad[1, 0, 5] = float("nan")
    bad[1, 2, 63] = float("nan")
    pair, total = aligner_amd.path_cost(bad, target, path, length, n, m, kind, r.c.scale)
    dpred, dtarget = aligner_amd.path_cost_backward(weight, bad, target, path, length, n, m, kind, r.c.scale, rs)
    assert torch.isnan(pair[1]).any() and torch.isnan(total[1])
    for b in (0, 2, 3, 4, 5):
        assert np.array_equal(pair[b].cpu().numpy(), pair0[b]) and total[b].item() == total0[b]
        assert np.array_equal(dpred[b].cpu().numpy(), dpred0[b]) and np.array_equal(dtarget[b].cpu().numpy(), dtarget0[b])
    # NaN in the padding past n[b] / m[b] reaches nothing
    ns, ms = orc.lengths(r.c.n, r.c.B, r.c.N), orc.lengths(r.c.m, r.c.B, r.c.M)
    pad_p, pad_t = pred.clone(), target.clone()
    for b in range(r.c.B):
        pad_p[b, :, ns[b]:] = float("nan")
        pad_t[b, :, ms[b]:] = float("nan")
    pair, total = aligner_amd.path_cost(pad_p, pad_t, path, length, n, m, kind, r.c.scale)
    dpred, dtarget = aligner_amd.path_cost_backward(weight, pad_p, pad_t, path, length, n, m, kind, r.c.scale, rs)
    assert np.array_equal(pair.cpu().numpy(), pair0) and np.array_equal(total.cpu().numpy(), total0)
    assert np.array_equal(dpred.cpu().numpy(), dpred0) and np.array_equal(dtarget.cpu().numpy(), dtarget0)


# ---- 6. stores inside their buffers ----------------------------------------------------------------------------------

FENCE = 1024                                                   # elements of canary on either side
CANARY = 0x7FC0BEEF                                            # (a NaN as a float)


def _fenced(count, dev):
    buf = torch.full((FENCE + count + FENCE,), CANARY, dtype=torch.int32, device=dev)
    return buf, buf[FENCE:FENCE + count]


def _intact(buf, count):
    return bool((buf[:FENCE] == CANARY).all()) and bool((buf[FENCE + count:] == CANARY).all())


@pytest.mark.parametrize("name", ["one", "channels129", "hand", "scaled"])
def test_stores_stay_inside_their_buffers(dev, name):
    """Every output and the workspace carved out of canary-filled allocations, the C ABI called on the interior
    pointers (hand: L = 194, N = 65, M = 130, the invalid paths among them): the canaries are intact, every element is
    written and the results are the wrappers'."""
    import aligner_amd
    from aligner_amd import _lib
    lib = _lib.load()
    r, pred, target, path, length, n, m, weight = _operands(name, dev)
    c = r.c
    B, C, N, M, L = c.B, c.C, c.N, c.M, r.L
    rs = _f32(_row_scale(r), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()                              # noqa: E731
    runs = [_fenced(count, dev) for count in (B * N, B * N, B * M, B * M, B)]
    _lib.check(lib.aligner_path_runs(path.data_ptr(), length.data_ptr(), *(v.data_ptr() for _, v in runs), B, L, N, M, stream))
    torch.cuda.synchronize()
    want = aligner_amd.path_runs(path, length, N, M)
    for (buf, view), w in zip(runs, want):
        assert _intact(buf, view.numel()) and torch.equal(view, w.reshape(-1)) and not bool((view == CANARY).any())
    for kind, code in (("l1", _lib.COST_L1), ("l2", _lib.COST_L2), ("l2root", _lib.COST_L2_ROOT)):
        pbuf, pair = _fenced(B * L, dev)
        tbuf, total = _fenced(B, dev)
        dbuf, dpred = _fenced(B * C * N, dev)
        ebuf, dtarget = _fenced(B * C * M, dev)
        nbytes = lib.aligner_path_cost_backward_workspace_bytes(code, B, N, M, L)
        assert nbytes > 0 and nbytes % 4 == 0
        wbuf, ws = _fenced(nbytes // 4, dev)
        _lib.check(lib.aligner_path_cost_f32(pred.data_ptr(), target.data_ptr(), path.data_ptr(), length.data_ptr(), ptr(n), ptr(m),
                                             code, c.scale, pair.data_ptr(), total.data_ptr(), B, C, N, M, L, stream))
        _lib.check(lib.aligner_path_cost_backward_f32(weight.data_ptr(), pred.data_ptr(), target.data_ptr(), path.data_ptr(),
                                                      length.data_ptr(), ptr(n), ptr(m), code, c.scale, rs.data_ptr(),
                                                      dpred.data_ptr(), dtarget.data_ptr(), ws.data_ptr(), nbytes,
                                                      B, C, N, M, L, stream))
        torch.cuda.synchronize()
        for buf, view in ((pbuf, pair), (tbuf, total), (dbuf, dpred), (ebuf, dtarget), (wbuf, ws)):
            assert _intact(buf, view.numel()), kind
        pair0, total0, dpred0, dtarget0 = _run(name, kind)[:4]
        for view, w in ((pair, pair0), (total, total0), (dpred, dpred0), (dtarget, dtarget0)):
            assert np.array_equal(view.view(torch.float32).cpu().numpy(), w.reshape(-1), equal_nan=True), kind
            assert not bool((view == CANARY).any()), kind


# ---- 7. the losses ---------------------------------------------------------------------------------------------------

def _loss(kind):
    import aligner_amd
    family, squared = KIND_ARGS[kind]
    if family == "l1":
        return aligner_amd.dtw_l1_loss, aligner_amd.dtw_path_l1, {}
    return aligner_amd.dtw_l2_loss, aligner_amd.dtw_path_l2, {"squared": squared}


# (edges without a band runs dense and with w = 127 in band storage; band30 with w = 30 in band storage and with w = 200,
# which band storage does not take, dense: utterance 1 of band30 has |n - m| = 35)
@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name, w", [("edges", None), ("edges", 127), ("band30", 30), ("band30", 200)])
def test_loss_value_is_dtw_paths_and_its_gradient_is_path_cost_backwards(dev, name, w, kind):
    import aligner_amd
    r, pred, target, _, _, n, m, _ = _operands(name, dev)
    c = r.c
    loss, find, extra = _loss(kind)
    p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
    value = loss(p, t, n, m, orc.PENALTY, w, 0.5, reduction="none", **extra)
    dp = find(pred, target, n, m, orc.PENALTY, w, 0.5, **extra)
    assert torch.equal(value.detach().view(torch.int32), dp.value.view(torch.int32))
    assert tuple(dp.path.shape) == (c.B, 2 * c.N + w - 1 if w is not None and w <= 127 else c.N + c.M - 1, 2)
    up = torch.tensor(np.linspace(-1.5, 2.0, c.B).astype(np.float32)).to(dev)
    value.backward(up)
    dpred, dtarget = aligner_amd.path_cost_backward(None, pred, target, dp.path, dp.length, n, m, kind, 0.5, up)
    assert torch.equal(p.grad.view(torch.int32), dpred.view(torch.int32)) and torch.equal(t.grad.view(torch.int32), dtarget.view(torch.int32))
    none = dp.length == 0
    assert bool(none.any()) == (w != 200) and bool((~none).any()) and torch.isinf(value[none]).all() and torch.isfinite(value[~none]).all()
    assert not p.grad[none].any() and not t.grad[none].any() and p.grad[~none].any() and t.grad[~none].any()
    # what the node keeps: pred, target, the path and its length -- no cost table
    fresh = loss(pred.clone().requires_grad_(), target, n, m, orc.PENALTY, w, 0.5, reduction="none", **extra)
    saved = fresh.grad_fn.saved_tensors
    assert [tuple(s.shape) for s in saved] == [tuple(pred.shape), tuple(target.shape), tuple(dp.path.shape), (c.B,)]


@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("name, w", [("edges", None), ("band30", 30), ("scaled", 40)])
def test_loss_normalized_by_the_path_is_the_oracles_mean(dev, name, w, kind):
    import aligner_amd
    r, pred, target, _, _, n, m, _ = _operands(name, dev)
    c = r.c
    loss, find, extra = _loss(kind)
    p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
    value = loss(p, t, n, m, orc.PENALTY, w, 0.5, normalize="path", reduction="none", **extra)
    dp = find(pred, target, n, m, orc.PENALTY, w, 0.5, **extra)
    path, length = dp.path.cpu().numpy(), dp.length.cpu().numpy()
    pair64, _, mean64 = orc.pair_cost64(r.pred, r.target, path, length, c.n, c.m, kind, 0.5)
    got = value.detach().cpu().numpy()
    _, rm = orc.total_ratios(kind, c.C, pair64, length, None, got, f"{name} w={w} {kind} loss")
    assert rm <= 1.0 and (got[length == 0] == np.inf).all() and np.isfinite(got[length > 0]).all()
    # the gradient: path_cost_backward with row_scale = g / length, bit for bit, and inside the bound
    up = np.linspace(-1.5, 2.0, c.B).astype(np.float32)
    value.backward(torch.tensor(up).to(dev))
    g = torch.tensor(up).to(dev) / dp.length.clamp(min=1).float()
    dpred, dtarget = aligner_amd.path_cost_backward(None, pred, target, dp.path, dp.length, n, m, kind, 0.5, g)
    assert torch.equal(p.grad, dpred) and torch.equal(t.grad, dtarget)
    expect = orc.grads64(None, r.pred, r.target, path, length, c.n, c.m, kind, 0.5, np.where(length > 0, g.cpu().numpy(), np.nan))
    rp, rt = orc.grad_ratios(f"{name} {kind}", p.grad.cpu().numpy(), t.grad.cpu().numpy(), expect, "loss by path")
    assert rp <= 1.0 and rt <= 1.0


@pytest.mark.parametrize("name, w", [("edges", None), ("edges", 127), ("band30", 30), ("scaled", 40)])
def test_mcd_loss_and_mcd_dtw_inside_the_mcd_bound(dev, name, w):
    import aligner_amd
    r, pred, target, _, _, n, m, _ = _operands(name, dev)
    c = r.c
    value = aligner_amd.mcd_dtw_loss(pred, target, n, m, orc.PENALTY, w, reduction="none")
    mcd, dp = aligner_amd.mcd_dtw(pred, target, n, m, orc.PENALTY, w)
    path, length = dp.path.cpu().numpy(), dp.length.cpu().numpy()
    want = l2o.mcd64(r.pred, r.target, path, length)
    assert (length == 0).any() and (length > 0).any()
    for label, got in (("mcd_dtw_loss", value.cpu().numpy().astype(np.float64)), ("mcd_dtw", mcd.cpu().numpy().astype(np.float64))):
        assert (got[length == 0] == np.inf).all()
        for b in np.nonzero(length)[0]:
            bound = l2o.mcd_constant(c.C, int(length[b])) * l2o.U * want[b]
            print(f"{name} w={w} [{b}] {label}: K = {length[b]}, {got[b]:.4f} dB, error / bound {abs(got[b] - want[b]) / bound:.3f}")
            assert abs(got[b] - want[b]) <= bound


def test_loss_without_an_alignment_zero_infinity_half_precision_and_no_gradient(dev):
    import aligner_amd
    r, pred, target, _, _, n, m, _ = _operands("band30", dev)              # utterance 1: |n - m| = 35 > 30
    for loss in (aligner_amd.dtw_l1_loss, aligner_amd.dtw_l2_loss, aligner_amd.mcd_dtw_loss):
        kw = {} if loss is aligner_amd.mcd_dtw_loss else {"normalize": "path"}
        p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
        value = loss(p, t, n, m, 0.05, 30, reduction="none", **kw)
        assert torch.isinf(value[1]) and torch.isfinite(value[[0, 2, 3]]).all()
        assert torch.isinf(loss(p, t, n, m, 0.05, 30, **kw))
        zi = loss(p, t, n, m, 0.05, 30, reduction="none", zero_infinity=True, **kw)
        assert zi[1] == 0 and torch.equal(zi[[0, 2, 3]], value[[0, 2, 3]])
        loss(p, t, n, m, 0.05, 30, reduction="sum", zero_infinity=True, **kw).backward()
        assert not p.grad[1].any() and not t.grad[1].any()
        for b in (0, 2, 3):
            assert p.grad[b].any() and t.grad[b].any()
        assert torch.isfinite(p.grad).all() and torch.isfinite(t.grad).all()
        # bf16 inputs get bf16 gradients, the fp32 kernels on the bf16 values; an input that requires none gets None
        pb, tb = pred.to(torch.bfloat16).requires_grad_(), target.to(torch.bfloat16).requires_grad_()
        loss(pb, tb, n, m, 0.05, 30, reduction="sum", zero_infinity=True, **kw).backward()
        assert pb.grad.dtype == torch.bfloat16 and tb.grad.dtype == torch.bfloat16
        pf, tf = pb.detach().float().requires_grad_(), tb.detach().float()
        loss(pf, tf, n, m, 0.05, 30, reduction="sum", zero_infinity=True, **kw).backward()
        assert tf.grad is None and torch.equal(pb.grad, pf.grad.to(torch.bfloat16))


def test_loss_past_1024_rows_in_band_storage(dev):
    import aligner_amd
    r, pred, target, _, _, n, m, _ = _operands("long_band", dev)
    p = pred.clone().requires_grad_()
    value = aligner_amd.dtw_l1_loss(p, target, n, m, orc.PENALTY, r.c.band, reduction="none")
    dp = aligner_amd.dtw_path_l1(pred, target, n, m, orc.PENALTY, r.c.band)
    assert torch.equal(value.detach(), dp.value) and torch.isfinite(value).all() and int(dp.length.min()) >= 1488
    value.sum().backward()
    dpred, none = aligner_amd.path_cost_backward(None, pred, target, dp.path, dp.length, n, m, "l1", want=(True, False))
    assert none is None and torch.equal(p.grad, dpred) and p.grad.any()
    with pytest.raises(aligner_amd._lib.AlignerError):
        aligner_amd.dtw_l1_loss(pred, target, n, m, orc.PENALTY, 200)      # (dense: N <= 1024)
