"""l2_cost() / l2_cost_backward() / soft_dtw_l2_loss(), their band-storage forms, dtw_path_l2() and mcd_dtw() on the GPU
against the float64 oracle (tests/l2cost_oracle.py) inside its derived bounds, on the shapes of l1cost_oracle.CASES (the
tiles are the L1 kernels') and, in band storage, on the cost cases of tests/test_banddtw_gpu.py, restated here.  G
carries a NaN at every cell that does not exist.  Then what needs no oracle: exact fill values, the band table against
the dense one bit for bit, a NaN that stays in its utterance, two runs with the same bits, each gradient alone with the
bits it has beside the other, stores inside their buffers, the autograd face, and the hard path fed the GPU's own
costs against tests/dtwpath_oracle.py bit for bit.  Every comparison prints observed / bound."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import banddtw_oracle as bo
import dtwpath_oracle as dpo
import l2cost_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _i32(t, dev):
    return None if t is None else torch.tensor(t, dtype=torch.int32, device=dev)


def _f32(t, dev):
    return None if t is None else torch.tensor(t, dtype=torch.float32, device=dev)


def _operands(name, dev):
    c, pred, target, G, *_ = orc.reference(name)
    return c, torch.tensor(pred).to(dev), torch.tensor(target).to(dev), torch.tensor(G).to(dev), _i32(c.n, dev), _i32(c.m, dev)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One GPU run per case, shared by the tests: (squared cost, root cost, dpred, dtarget) as numpy arrays."""
    import aligner_amd
    dev = torch.device("cuda:0")
    c, pred, target, G, n, m = _operands(name, dev)
    sq = aligner_amd.l2_cost(pred, target, n, m, c.band, c.scale)
    rt = aligner_amd.l2_cost(pred, target, n, m, c.band, c.scale, squared=False)
    dpred, dtarget = aligner_amd.l2_cost_backward(G, pred, target, n, m, c.band, c.scale, _f32(c.row_scale, dev))
    torch.cuda.synchronize()
    return sq.cpu().numpy(), rt.cpu().numpy(), dpred.cpu().numpy(), dtarget.cpu().numpy()


# ---- 1. bounds, dense ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_costs_and_gradients_inside_the_bounds(dev, name):
    c = orc.CASES[name]
    sq, rt, dpred, dtarget = _run(name)
    rs = orc.check_cost(name, sq, True, "GPU")                  # (asserts the exact fill values as well)
    rr = orc.check_cost(name, rt, False, "GPU")
    rp, rg = orc.check_grads(name, dpred, dtarget, "GPU")
    assert rs <= 1.0 and rr <= 1.0 and rp <= 1.0 and rg <= 1.0
    ok, inside = orc.exists(c.B, c.N, c.M, c.n, c.m, c.band)
    for cost in (sq, rt):
        assert np.isfinite(cost[ok]).all() and (cost[inside & ~ok] == np.inf).all() and not cost[~inside].any()
    n, m = orc.lengths(c.n, c.B, c.N), orc.lengths(c.m, c.B, c.M)
    for b in range(c.B):
        assert not dpred[b, :, n[b]:].any() and not dtarget[b, :, m[b]:].any()
        assert not dpred[b][:, ~ok[b].any(1)].any() and not dtarget[b][:, ~ok[b].any(0)].any()
    assert np.isfinite(dpred).all() and np.isfinite(dtarget).all()          # none of G's NaNs came through


def test_no_limit_on_the_rows(dev):
    import aligner_amd
    rng = np.random.default_rng(11)
    pred, target = rng.uniform(-1, 1, (1, 2, 1500)).astype(np.float32), rng.uniform(-1, 1, (1, 2, 3)).astype(np.float32)
    for squared in (True, False):
        cost = aligner_amd.l2_cost(torch.tensor(pred).to(dev), torch.tensor(target).to(dev), bandwidth=1200, squared=squared).cpu().numpy()
        want = orc.cost64(pred, target, band=1200, squared=squared)
        ratio = orc.cost_ratio(cost, want, np.isfinite(want), 2, squared)
        print(f"1500 rows, squared={squared}: cost error / bound {ratio:.3f}")
        assert ratio <= 1.0 and (~np.isfinite(want)).sum() == 299 + 298 + 297


# ---- band storage: the cost cases of tests/test_banddtw_gpu.py -------------------------------------------------------

def _cost_case(C, w, N=70, M=90, n=(70, 50), m=(66, 90), seed=0):
    return SimpleNamespace(B=2, C=C, N=N, M=M, w=w, n=n, m=m, scale=0.5, row_scale=(-1.5, 2.0), seed=seed)


BAND_CASES = {f"c{C}_w{w}": _cost_case(C, w, seed=C * 1000 + w) for C in (1, 3, 8, 9) for w in (5, 64)}
BAND_CASES["m_below_n"] = _cost_case(3, 5, N=70, M=40, n=(70, 33), m=(40, 40), seed=11)
BAND_CASES["m_past_n_plus_w"] = _cost_case(3, 5, N=30, M=90, n=(30, 30), m=(90, 33), seed=12)


@functools.lru_cache(maxsize=None)
def _band_reference(name):
    """(case, pred, target, G_band with NaN where no cell exists, exists [B,N,W], squared cost64 and root cost64 in band
    storage, dpred64, dtarget64 and their bounds) -- inputs quantised to 1/4 so that pred == target happens."""
    c = BAND_CASES[name]
    rng = np.random.default_rng(c.seed)
    pred = (np.round(rng.uniform(-1.0, 1.0, (c.B, c.C, c.N)) * 4) / 4).astype(np.float32)
    target = (np.round(rng.uniform(-1.0, 1.0, (c.B, c.C, c.M)) * 4) / 4).astype(np.float32)
    exists = bo.exists_band(c)
    G = rng.normal(0.0, 1.0, exists.shape).astype(np.float32)
    G[~exists] = np.nan
    band = lambda x: bo.to_band(np.where(np.isfinite(x), x, 0.0), c.w)      # noqa: E731
    sq = band(orc.cost64(pred, target, c.n, c.m, c.w, c.scale, True))
    rt = band(orc.cost64(pred, target, c.n, c.m, c.w, c.scale, False))
    grads = orc.grads64(bo.to_dense(G, c.M, np.nan), pred, target, c.n, c.m, c.w, c.scale, c.row_scale)
    return (c, pred, target, G, exists, sq, rt) + tuple(grads)


def _band_operands(name, dev):
    c, pred, target, G, *_ = _band_reference(name)
    rs = torch.tensor(c.row_scale, dtype=torch.float32, device=dev)
    return c, torch.tensor(pred).to(dev), torch.tensor(target).to(dev), torch.tensor(G).to(dev), _i32(c.n, dev), _i32(bo.m_of(c), dev), rs


@functools.lru_cache(maxsize=None)
def _band_run(name):
    import aligner_amd
    dev = torch.device("cuda:0")
    c, p, t, g, n, m, rs = _band_operands(name, dev)
    sq = aligner_amd.l2_cost_banded(p, t, n, m, c.w, c.scale)
    rt = aligner_amd.l2_cost_banded(p, t, n, m, c.w, c.scale, squared=False)
    dpred, dtarget = aligner_amd.l2_cost_banded_backward(g, p, t, n, m, c.scale, rs)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (sq, rt, dpred, dtarget))


@pytest.mark.parametrize("name", list(BAND_CASES))
def test_costs_and_gradients_in_band_storage_inside_the_bounds(dev, name):
    c, pred, target, G, exists, sq64, rt64, dp64, dt64, bp, bt = _band_reference(name)
    sq, rt, dpred, dtarget = _band_run(name)
    assert sq.shape == exists.shape and rt.shape == exists.shape
    rs = orc.cost_ratio(sq, sq64, exists, c.C, True)            # (asserts exactly 0 where no cell exists)
    rr = orc.cost_ratio(rt, rt64, exists, c.C, False)
    print(f"{name}: squared cost error / bound {rs:.3f}, root cost error / bound {rr:.3f} over {int(exists.sum())} cells")
    rp, rg = orc.grad_ratios(name, dpred, dtarget, (dp64, dt64, bp, bt), "GPU band")
    assert rs <= 1.0 and rr <= 1.0 and rp <= 1.0 and rg <= 1.0
    ok, _ = orc.exists(c.B, c.N, c.M, c.n, c.m, c.w)
    for b in range(c.B):
        assert not dpred[b][:, ~ok[b].any(1)].any() and not dtarget[b][:, ~ok[b].any(0)].any()
    assert np.isfinite(dpred).all() and np.isfinite(dtarget).all()


# ---- 2. band against dense -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BAND_CASES))
def test_band_table_has_the_dense_tables_bits(dev, name):
    import aligner_amd
    c, p, t, _, n, m, _ = _band_operands(name, dev)
    exists = torch.tensor(_band_reference(name)[4]).to(dev)
    for squared, got in zip((True, False), _band_run(name)[:2]):
        dense = aligner_amd.l2_cost(p, t, n, m, c.w, c.scale, squared=squared)
        want = aligner_amd.dense_to_band(dense, c.w)
        got = torch.tensor(got).to(dev)
        assert torch.equal(got[exists].view(torch.int32), want[exists].view(torch.int32)), (name, squared)
        assert bool(torch.isfinite(want[exists]).all()) and not got[~exists].any()


# ---- 3. determinism and robustness -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edges", "band30", "scaled"])
def test_two_runs_give_the_same_bits_and_each_gradient_alone_too(dev, name):
    import aligner_amd
    c, pred, target, G, n, m = _operands(name, dev)
    rs = _f32(c.row_scale, dev)
    sq0, rt0, dpred0, dtarget0 = _run(name)
    assert np.array_equal(aligner_amd.l2_cost(pred, target, n, m, c.band, c.scale).cpu().numpy(), sq0)
    assert np.array_equal(aligner_amd.l2_cost(pred, target, n, m, c.band, c.scale, squared=False).cpu().numpy(), rt0)
    dpred, dtarget = aligner_amd.l2_cost_backward(G, pred, target, n, m, c.band, c.scale, rs)
    assert np.array_equal(dpred.cpu().numpy(), dpred0) and np.array_equal(dtarget.cpu().numpy(), dtarget0)
    only_p, none = aligner_amd.l2_cost_backward(G, pred, target, n, m, c.band, c.scale, rs, want=(True, False))
    assert none is None and np.array_equal(only_p.cpu().numpy(), dpred0)
    none, only_t = aligner_amd.l2_cost_backward(G, pred, target, n, m, c.band, c.scale, rs, want=(False, True))
    assert none is None and np.array_equal(only_t.cpu().numpy(), dtarget0)


@pytest.mark.parametrize("name", ["c9_w5", "c3_w64", "m_past_n_plus_w"])
def test_two_runs_in_band_storage_give_the_same_bits_and_each_gradient_alone_too(dev, name):
    import aligner_amd
    c, p, t, g, n, m, rs = _band_operands(name, dev)
    sq0, rt0, dpred0, dtarget0 = _band_run(name)
    assert np.array_equal(aligner_amd.l2_cost_banded(p, t, n, m, c.w, c.scale).cpu().numpy(), sq0)
    assert np.array_equal(aligner_amd.l2_cost_banded(p, t, n, m, c.w, c.scale, squared=False).cpu().numpy(), rt0)
    only_p, none = aligner_amd.l2_cost_banded_backward(g, p, t, n, m, c.scale, rs, want=(True, False))
    assert none is None and np.array_equal(only_p.cpu().numpy(), dpred0)
    none, only_t = aligner_amd.l2_cost_banded_backward(g, p, t, n, m, c.scale, rs, want=(False, True))
    assert none is None and np.array_equal(only_t.cpu().numpy(), dtarget0)


def test_nan_stays_in_its_utterance(dev):
    import aligner_amd
    c, pred, target, G, n, m = _operands("edges", dev)
    bad = pred.clone()
    bad[1, 0, 5] = float("nan")
    bad[1, 2, 63] = float("nan")
    sq0, rt0, dpred0, dtarget0 = _run("edges")
    for squared, cost0 in ((True, sq0), (False, rt0)):
        cost = aligner_amd.l2_cost(bad, target, n, m, c.band, c.scale, squared=squared)
        assert torch.isnan(cost[1, 5, :128]).all()
        for b in (0, 2, 3, 4, 5):
            assert np.array_equal(cost[b].cpu().numpy(), cost0[b])
    dpred, dtarget = aligner_amd.l2_cost_backward(G, bad, target, n, m, c.band, c.scale)
    for b in (0, 2, 3, 4, 5):
        assert np.array_equal(dpred[b].cpu().numpy(), dpred0[b]) and np.array_equal(dtarget[b].cpu().numpy(), dtarget0[b])
    # in band storage (w = 127 holds every cell of these tables)
    cb0 = aligner_amd.l2_cost_banded(pred, target, n, m, 127, c.scale)
    cb = aligner_amd.l2_cost_banded(bad, target, n, m, 127, c.scale)
    Gb = aligner_amd.dense_to_band(G, 127)
    g0 = aligner_amd.l2_cost_banded_backward(Gb, pred, target, n, m, c.scale)
    g1 = aligner_amd.l2_cost_banded_backward(Gb, bad, target, n, m, c.scale)
    assert torch.isnan(cb[1]).any()
    for b in (0, 2, 3, 4, 5):
        assert torch.equal(cb[b], cb0[b]) and torch.equal(g1[0][b], g0[0][b]) and torch.equal(g1[1][b], g0[1][b])


def test_nan_past_the_lengths_reaches_nothing(dev):
    """pred rows at or past n[b] and target columns at or past m[b] are padding: the gradient multiplies a masked G of
    +0 by a difference, and takes that difference from inside the lengths."""
    import aligner_amd
    c, pred, target, G, n, m = _operands("edges", dev)
    sq0, rt0, dpred0, dtarget0 = _run("edges")
    ns, ms = orc.lengths(c.n, c.B, c.N), orc.lengths(c.m, c.B, c.M)
    bad_p, bad_t = pred.clone(), target.clone()
    for b in range(c.B):
        bad_p[b, :, ns[b]:] = float("nan")
        bad_t[b, :, ms[b]:] = float("nan")
    assert torch.isnan(bad_p).any() and torch.isnan(bad_t).any()
    assert np.array_equal(aligner_amd.l2_cost(bad_p, bad_t, n, m, c.band, c.scale).cpu().numpy(), sq0)
    assert np.array_equal(aligner_amd.l2_cost(bad_p, bad_t, n, m, c.band, c.scale, squared=False).cpu().numpy(), rt0)
    dpred, dtarget = aligner_amd.l2_cost_backward(G, bad_p, bad_t, n, m, c.band, c.scale)
    assert np.array_equal(dpred.cpu().numpy(), dpred0) and np.array_equal(dtarget.cpu().numpy(), dtarget0)
    Gb = aligner_amd.dense_to_band(G, 127)
    g0 = aligner_amd.l2_cost_banded_backward(Gb, pred, target, n, m, c.scale)
    g1 = aligner_amd.l2_cost_banded_backward(Gb, bad_p, bad_t, n, m, c.scale)
    assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])
    assert torch.equal(aligner_amd.l2_cost_banded(bad_p, bad_t, n, m, 127, c.scale),
                       aligner_amd.l2_cost_banded(pred, target, n, m, 127, c.scale))


FENCE = 1024                                                   # floats of canary on either side


def _fenced(count, dev):
    buf = torch.full((FENCE + count + FENCE,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[FENCE:FENCE + count]


def _intact(buf, count):
    return bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + count:]).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("name", ["one", "edges", "channels129", "tall", "band30", "scaled"])
def test_stores_stay_inside_their_buffers(dev, name):
    """The costs, dpred and dtarget carved out of NaN-filled allocations, the C ABI called on the interior pointers: the
    canaries are intact and the results are the wrapper's.  (No call has a workspace.)"""
    from aligner_amd import _lib
    lib = _lib.load()
    c, pred, target, G, n, m = _operands(name, dev)
    rs = _f32(c.row_scale, dev)
    sbuf, sq = _fenced(c.B * c.N * c.M, dev)
    rbuf, rt = _fenced(c.B * c.N * c.M, dev)
    pbuf, dpred = _fenced(c.B * c.C * c.N, dev)
    tbuf, dtarget = _fenced(c.B * c.C * c.M, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    band = -1 if c.band is None else c.band
    for squared, out in ((1, sq), (0, rt)):
        _lib.check(lib.aligner_l2_cost_f32(pred.data_ptr(), target.data_ptr(), _ptr(n), _ptr(m), band, c.scale, squared,
                                           out.data_ptr(), c.B, c.C, c.N, c.M, stream))
    _lib.check(lib.aligner_l2_cost_backward_f32(G.data_ptr(), pred.data_ptr(), target.data_ptr(), _ptr(n), _ptr(m), band, c.scale,
                                                _ptr(rs), dpred.data_ptr(), dtarget.data_ptr(), c.B, c.C, c.N, c.M, stream))
    torch.cuda.synchronize()
    for buf, count in ((sbuf, sq.numel()), (rbuf, rt.numel()), (pbuf, dpred.numel()), (tbuf, dtarget.numel())):
        assert _intact(buf, count)
    sq0, rt0, dpred0, dtarget0 = _run(name)
    assert np.array_equal(sq.view(c.B, c.N, c.M).cpu().numpy(), sq0) and np.array_equal(rt.view(c.B, c.N, c.M).cpu().numpy(), rt0)
    assert np.array_equal(dpred.view(c.B, c.C, c.N).cpu().numpy(), dpred0)
    assert np.array_equal(dtarget.view(c.B, c.C, c.M).cpu().numpy(), dtarget0)
    for out in (sq, rt, dpred, dtarget):
        assert not torch.isnan(out).any()


@pytest.mark.parametrize("name", ["c9_w5", "c3_w64", "m_below_n", "m_past_n_plus_w"])
def test_band_storage_stores_stay_inside_their_buffers(dev, name):
    from aligner_amd import _lib
    lib = _lib.load()
    c, p, t, g, n, m, rs = _band_operands(name, dev)
    W = 2 * c.w + 1
    sbuf, sq = _fenced(c.B * c.N * W, dev)
    rbuf, rt = _fenced(c.B * c.N * W, dev)
    pbuf, dpred = _fenced(c.B * c.C * c.N, dev)
    tbuf, dtarget = _fenced(c.B * c.C * c.M, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for squared, out in ((1, sq), (0, rt)):
        _lib.check(lib.aligner_l2_cost_banded_f32(p.data_ptr(), t.data_ptr(), n.data_ptr(), m.data_ptr(), c.w, c.scale, squared,
                                                  out.data_ptr(), c.B, c.C, c.N, c.M, stream))
    _lib.check(lib.aligner_l2_cost_banded_backward_f32(g.data_ptr(), p.data_ptr(), t.data_ptr(), n.data_ptr(), m.data_ptr(), c.w,
                                                       c.scale, rs.data_ptr(), dpred.data_ptr(), dtarget.data_ptr(),
                                                       c.B, c.C, c.N, c.M, stream))
    torch.cuda.synchronize()
    for buf, count in ((sbuf, sq.numel()), (rbuf, rt.numel()), (pbuf, dpred.numel()), (tbuf, dtarget.numel())):
        assert _intact(buf, count)
    sq0, rt0, dpred0, dtarget0 = _band_run(name)
    assert np.array_equal(sq.view(c.B, c.N, W).cpu().numpy(), sq0) and np.array_equal(rt.view(c.B, c.N, W).cpu().numpy(), rt0)
    assert np.array_equal(dpred.view(c.B, c.C, c.N).cpu().numpy(), dpred0)
    assert np.array_equal(dtarget.view(c.B, c.C, c.M).cpu().numpy(), dtarget0)


# ---- 4. soft_dtw_l2_loss ---------------------------------------------------------------------------------------------

GAMMA, PENALTY = 1.0, 0.1


@pytest.mark.parametrize("name", ["edges", "band30", "scaled"])
def test_loss_value_is_the_composition_and_its_gradients_are_inside_the_bound(dev, name):
    """value: the bits of soft_dtw_loss(l2_cost(...)).  Gradients: the oracle fed with the GPU's own E and the upstream
    gradient as row_scale, so that only the arithmetic of l2_cost_backward is judged."""
    import aligner_amd
    c, pred, target, _, n, m = _operands(name, dev)
    pred.requires_grad_()
    target.requires_grad_()
    value = aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band, c.scale, reduction="none")
    cost = aligner_amd.l2_cost(pred, target, n, m, c.band, c.scale)
    assert torch.equal(value, aligner_amd.soft_dtw_loss(cost, n, m, GAMMA, PENALTY, c.band, reduction="none"))
    up = np.linspace(-1.5, 2.0, c.B).astype(np.float32)
    value.backward(torch.tensor(up).to(dev))
    _, E = aligner_amd.soft_dtw(cost, n, m, GAMMA, PENALTY, c.band)
    expect = orc.grads64(E.cpu().numpy(), pred.detach().cpu().numpy(), target.detach().cpu().numpy(), c.n, c.m, c.band, c.scale, up)
    rp, rt = orc.check_grads(name, pred.grad.cpu().numpy(), target.grad.cpu().numpy(), "GPU loss", expect=expect)
    assert rp <= 1.0 and rt <= 1.0
    assert pred.grad.abs().sum() > 0 and target.grad.abs().sum() > 0


def test_loss_band_excludes_an_utterance_and_leaves_its_neighbours_their_gradients(dev):
    import aligner_amd
    c, pred, target, _, n, m = _operands("band30", dev)               # utterance 1: |n - m| = 35 > 30
    pred.requires_grad_()
    target.requires_grad_()
    value = aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="none")
    assert torch.isinf(value[1]) and torch.isfinite(value[[0, 2, 3]]).all()
    assert torch.isinf(aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band))
    zi = aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="none", zero_infinity=True)
    assert zi[1] == 0 and torch.equal(zi[[0, 2, 3]], value[[0, 2, 3]])
    aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert not pred.grad[1].any() and not target.grad[1].any()
    for b in (0, 2, 3):
        assert pred.grad[b].any() and target.grad[b].any()
    assert torch.isfinite(pred.grad).all() and torch.isfinite(target.grad).all()


def test_loss_half_precision_and_an_input_without_a_gradient(dev):
    import aligner_amd
    c, pred, target, _, n, m = _operands("band30", dev)
    pb, tb = pred.to(torch.bfloat16).requires_grad_(), target.to(torch.bfloat16).requires_grad_()
    aligner_amd.soft_dtw_l2_loss(pb, tb, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert pb.grad.dtype == torch.bfloat16 and tb.grad.dtype == torch.bfloat16
    pf, tf = pb.detach().float().requires_grad_(), tb.detach().float()    # (the same fp32 kernels on the bf16 values)
    assert not tf.requires_grad
    aligner_amd.soft_dtw_l2_loss(pf, tf, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert tf.grad is None                                               # None came back for the target
    assert torch.equal(pb.grad, pf.grad.to(torch.bfloat16))


def test_loss_keeps_no_cost_tensor(dev):
    """What the autograd node saves is pred, target and E: no cost tensor, no cdist graph."""
    import aligner_amd
    c, pred, target, _, n, m = _operands("band30", dev)
    pred.requires_grad_()
    value = aligner_amd.soft_dtw_l2_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="none")
    saved = value.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == pred.data_ptr() and tuple(saved[2].shape) == (c.B, c.N, c.M)
    assert tuple(saved[1].shape) == tuple(target.shape)


def test_loss_agrees_with_the_cdist_composition(dev):
    """The comparison, and the tolerances, of the L1 test of that name."""
    import aligner_amd
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(2, 50, 8, generator=g).to(dev).requires_grad_()                 # [B,T,C]
    target = torch.rand(2, 70, 8, generator=g).to(dev).requires_grad_()
    want = aligner_amd.soft_dtw_loss(torch.cdist(pred, target, p=2) ** 2 * (1 / 8), gamma=1.0, warp_penalty=0.1, bandwidth=40, reduction="sum")
    want.backward()
    p2 = pred.detach().transpose(1, 2).contiguous().requires_grad_()                  # [B,C,T]
    t2 = target.detach().transpose(1, 2).contiguous().requires_grad_()
    got = aligner_amd.soft_dtw_l2_loss(p2, t2, gamma=1.0, warp_penalty=0.1, bandwidth=40, scale=1 / 8, reduction="sum")
    got.backward()
    dv = abs(got.item() - want.item()) / abs(want.item())
    dp = (p2.grad.transpose(1, 2) - pred.grad).abs().max().item()
    dt = (t2.grad.transpose(1, 2) - target.grad).abs().max().item()
    print(f"fused against cdist composition: value {dv:.2e} relative, dpred {dp:.2e}, dtarget {dt:.2e} absolute "
          f"(largest |dpred| {pred.grad.abs().max().item():.2e})")
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-6)
    assert torch.allclose(p2.grad.transpose(1, 2), pred.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(t2.grad.transpose(1, 2), target.grad, rtol=1e-4, atol=1e-6)


# ---- 5. soft_dtw_l2_banded_loss --------------------------------------------------------------------------------------

def _loss_operands(dev, w=30):
    """[3,8,100,120] with lengths that leave utterance 1 without an alignment at w = 30 (|n - m| = 35)."""
    rng = np.random.default_rng(5)
    pred = torch.tensor(rng.uniform(-1, 1, (3, 8, 100)).astype(np.float32)).to(dev)
    target = torch.tensor(rng.uniform(-1, 1, (3, 8, 120)).astype(np.float32)).to(dev)
    return pred, target, (100, 60, 90), (120, 95, 110), w


def test_banded_loss_value_is_the_dense_losss_and_gradients_agree_with_it(dev):
    """value: the bits of soft_dtw_banded(l2_cost_banded(...)) and of the dense loss.  Gradients against soft_dtw_l2_loss
    on the same inputs and band, inside the sum of the two bounds GRAD (of the band sums and of the dense sums)."""
    import aligner_amd
    pred, target, ns, ms, w = _loss_operands(dev)
    n, m = _i32(ns, dev), _i32(ms, dev)
    scale = 1.0 / 8
    up = np.array([1.5, -2.0, 0.75], np.float32)
    grads = {}
    for kind in ("band", "dense"):
        p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
        if kind == "band":
            value = aligner_amd.soft_dtw_l2_banded_loss(p, t, n, m, GAMMA, PENALTY, w, scale, reduction="none")
            cost = aligner_amd.l2_cost_banded(pred, target, n, m, w, scale)
            parts, E = aligner_amd.soft_dtw_banded(cost, n, m, GAMMA, PENALTY)
            assert torch.equal(value, parts)
            Ed = bo.to_dense(E.cpu().numpy(), 120)
        else:
            value = aligner_amd.soft_dtw_l2_loss(p, t, n, m, GAMMA, PENALTY, w, scale, reduction="none")
            _, E = aligner_amd.soft_dtw(aligner_amd.l2_cost(pred, target, n, m, w, scale), n, m, GAMMA, PENALTY, w)
            Ed = E.cpu().numpy()
        assert torch.isinf(value[1]) and torch.isfinite(value[[0, 2]]).all()
        value.backward(torch.tensor(up).to(dev))
        exact = orc.grads64(Ed, pred.cpu().numpy(), target.cpu().numpy(), ns, ms, w, scale, up)
        grads[kind] = (value.detach().cpu().numpy(), p.grad.cpu().numpy(), t.grad.cpu().numpy(), exact)
    vb, pb, tb, (dpb, dtb, bpb, btb) = grads["band"]
    vd, pd, td, (dpd, dtd, bpd, btd) = grads["dense"]
    assert np.array_equal(vb, vd)                                           # the forward values share their bits
    rp, rt = orc.grad_ratios("loss", pb, tb, (dpb, dtb, bpb, btb), "band loss")
    assert rp <= 1.0 and rt <= 1.0
    print(f"loss: largest |dpred_band - dpred_dense| / bound "
          f"{(np.abs(pb.astype(np.float64) - pd) / np.maximum(bpb + bpd, 1e-300)).max():.3f}, dtarget "
          f"{(np.abs(tb.astype(np.float64) - td) / np.maximum(btb + btd, 1e-300)).max():.3f}")
    assert (np.abs(pb.astype(np.float64) - pd) <= bpb + bpd).all()
    assert (np.abs(tb.astype(np.float64) - td) <= btb + btd).all()
    assert not pb[1].any() and not tb[1].any() and pb[0].any() and tb[2].any()


def test_banded_loss_past_1024_frames_half_precision_and_no_target_gradient(dev):
    import aligner_amd
    rng = np.random.default_rng(6)
    pred = torch.tensor(rng.uniform(-1, 1, (2, 4, 1100)).astype(np.float32)).to(dev).to(torch.bfloat16).requires_grad_()
    target = torch.tensor(rng.uniform(-1, 1, (2, 4, 1090)).astype(np.float32)).to(dev)
    with pytest.raises(aligner_amd._lib.AlignerError):
        aligner_amd.soft_dtw_l2_loss(pred, target, bandwidth=20)
    loss = aligner_amd.soft_dtw_l2_banded_loss(pred, target, None, None, GAMMA, PENALTY, 20, 0.25, reduction="sum")
    loss.backward()
    assert torch.isfinite(loss) and pred.grad.dtype == torch.bfloat16 and target.grad is None
    assert torch.isfinite(pred.grad.float()).all() and pred.grad.any()


# ---- 6. dtw_path_l2 --------------------------------------------------------------------------------------------------

def _assert_oracle_path(r, cost, c_n, c_m, p, w, L):
    """value, path and length of the GPU against dtwpath_oracle on the GPU's own (dense) cost table, bit for bit."""
    value, path, length = dpo.dtw_path32(cost, c_n, c_m, p, w, L)
    assert np.array_equal(r.value.cpu().numpy().view(np.int32), value.view(np.int32)), (r.value.cpu().numpy(), value)
    assert np.array_equal(r.length.cpu().numpy(), length)
    assert np.array_equal(r.path.cpu().numpy(), path)
    return value, path, length


# (edges without a band runs dense and with w = 127 in band storage; band30 with w = 30 in band storage and with w = 200,
# which band storage does not take, dense)
@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("name, w", [("edges", None), ("edges", 127), ("band30", 30), ("band30", 200)])
def test_path_is_the_oracles_on_the_gpus_own_costs(dev, name, w, squared):
    import aligner_amd
    c, pred, target, _, n, m = _operands(name, dev)
    p = 0.05
    r = aligner_amd.dtw_path_l2(pred, target, n, m, p, w, 0.5, squared=squared)
    banded = w is not None and w <= 127
    L = 2 * c.N + w - 1 if banded else c.N + c.M - 1
    assert tuple(r.path.shape) == (c.B, L, 2)
    cost = aligner_amd.l2_cost(pred, target, n, m, w, 0.5, squared=squared).cpu().numpy()
    value, _, length = _assert_oracle_path(r, cost, c.n, c.m, p, w, L)
    assert (length > 0).any() and np.isfinite(value[length > 0]).all() and (value[length == 0] == np.inf).all()


def test_path_past_1024_rows_in_band_storage(dev):
    import aligner_amd
    from aligner_amd import _lib
    rng = np.random.default_rng(12)
    N, M, w = 1500, 1490, 20
    pred = rng.uniform(-1, 1, (1, 2, N)).astype(np.float32).cumsum(2) * np.float32(0.1)
    target = rng.uniform(-1, 1, (1, 2, M)).astype(np.float32).cumsum(2) * np.float32(0.1)
    p, t = torch.tensor(pred).to(dev), torch.tensor(target).to(dev)
    r = aligner_amd.dtw_path_l2(p, t, warp_penalty=0.01, bandwidth=w)
    cost = aligner_amd.l2_cost(p, t, bandwidth=w, squared=False)
    _assert_oracle_path(r, cost.cpu().numpy(), None, None, 0.01, w, 2 * N + w - 1)
    assert int(r.length[0]) >= N
    with pytest.raises(_lib.AlignerError) as err:
        aligner_amd.dtw_path(cost, bandwidth=w)
    assert err.value.code == _lib.EDOM


# ---- 7. mcd_dtw ------------------------------------------------------------------------------------------------------

# (each case has utterances with and without an alignment; edges runs dense and, with w = 127, in band storage)
@pytest.mark.parametrize("name, w", [("edges", None), ("edges", 127), ("band30", 30), ("scaled", 40)])
def test_mcd_along_the_path(dev, name, w):
    import aligner_amd
    c, pred, target, _, n, m = _operands(name, dev)
    mcd, r = aligner_amd.mcd_dtw(pred, target, n, m, 0.05, w)
    assert mcd.dtype == torch.float32 and tuple(mcd.shape) == (c.B,)
    same = aligner_amd.dtw_path_l2(pred, target, n, m, 0.05, w, orc.MCD_SCALE)
    assert torch.equal(r.path, same.path) and torch.equal(r.length, same.length) and torch.equal(r.value, same.value)
    banded = w is not None and w <= 127
    cost = aligner_amd.l2_cost(pred, target, n, m, w, orc.MCD_SCALE, squared=False).cpu().numpy()
    _, path, length = _assert_oracle_path(r, cost, c.n, c.m, 0.05, w, 2 * c.N + w - 1 if banded else c.N + c.M - 1)
    want = orc.mcd64(orc.reference(name)[1], orc.reference(name)[2], path, length)
    got = mcd.cpu().numpy().astype(np.float64)
    assert (length == 0).any() and (length > 0).any()
    assert (got[length == 0] == np.inf).all() and (want[length == 0] == np.inf).all()
    for b in np.nonzero(length)[0]:
        bound = orc.mcd_constant(c.C, int(length[b])) * orc.U * want[b]
        print(f"{name} w={w} [{b}]: K = {length[b]}, mcd {got[b]:.4f} dB, error / bound {abs(got[b] - want[b]) / bound:.3f}")
        assert abs(got[b] - want[b]) <= bound


def test_mcd_does_not_depend_on_the_penalty_when_the_path_does_not(dev):
    """band0: the diagonal is the only path, whatever the penalty."""
    import aligner_amd
    c, pred, target, _, n, m = _operands("band0", dev)
    mcd0, r0 = aligner_amd.mcd_dtw(pred, target, n, m, 0.0, c.band)
    mcd1, r1 = aligner_amd.mcd_dtw(pred, target, n, m, 7.5, c.band)
    assert torch.equal(r0.path, r1.path) and torch.equal(r0.length, r1.length)
    assert torch.equal(mcd0, mcd1) and torch.isfinite(mcd0[0]) and torch.isinf(mcd0[1])
    # and with stalls on the path: the value carries the penalty, the mean does not
    c, pred, target, _, n, m = _operands("band30", dev)
    mcd0, r0 = aligner_amd.mcd_dtw(pred, target, n, m, 0.0, c.band)
    mcd1, r1 = aligner_amd.mcd_dtw(pred, target, n, m, 1e-3, c.band)
    for b in range(c.B):
        if int(r0.length[b]) > 0 and torch.equal(r0.path[b], r1.path[b]):
            assert torch.equal(mcd0[b], mcd1[b])
            if int(r0.length[b]) > max(int(n[b]), int(m[b])):
                assert r1.value[b] > r0.value[b]
