"""The band-storage Soft-DTW on the GPU (aligner_amd/banddtw.py, csrc/banddtw.hip): value and E_band against the float64
oracle of the dense image inside its derived bounds (tests/banddtw_oracle.py has the cases and says which kernel edges
they straddle), the forward value against the dense kernel bit for bit, the flow, the exact zeros, NaN in elements
without a cell, determinism, guard bands; the L1 cost and its gradients in band layout against tests/l1cost_oracle.py;
the loss as one autograd function against its parts and against soft_dtw_l1_loss.  Comparisons print observed / bound."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import banddtw_oracle as bo
import l1cost_oracle as lco
import softdtw_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _i32(t, dev):
    return None if t is None else torch.tensor(t, dtype=torch.int32, device=dev)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One GPU run per case, shared by the tests: (value [B], E_band [B,N,W]) as numpy arrays."""
    import aligner_amd
    dev = torch.device("cuda:0")
    c, _, _, band, *_ = bo.reference(name)
    value, E = aligner_amd.soft_dtw_banded(torch.tensor(band).to(dev), _i32(c.n, dev), _i32(bo.m_of(c), dev), c.gamma, c.p)
    torch.cuda.synchronize()
    return value.cpu().numpy(), E.cpu().numpy()


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_value_and_expected_alignment_inside_the_bounds(dev, name):
    c = bo.reference(name)[0]
    value, E = _run(name)
    assert E.shape == (c.B, c.N, 2 * c.w + 1)
    rv, rg = bo.check(name, value, bo.to_dense(E, c.M), "GPU band")
    assert rv <= 1.0 and rg <= 1.0


@pytest.mark.parametrize("name", bo.DENSE_NAMES)
def test_forward_value_has_the_dense_kernels_bits(dev, name):
    """The two kernels share softdtw_cell.h and a cell is a function of its operands only."""
    import aligner_amd
    c, _, _, band, *_ = bo.reference(name)
    value, _ = _run(name)
    dense = aligner_amd.band_to_dense(torch.tensor(band).to(dev), c.M, fill=float("inf"))
    v_dense, _ = aligner_amd.soft_dtw(dense, _i32(c.n, dev), _i32(bo.m_of(c), dev), c.gamma, c.p, c.w, want_grad=False)
    assert np.array_equal(v_dense.cpu().numpy(), value), (v_dense.cpu().numpy(), value)


def test_the_dense_call_refuses_what_band_storage_runs(dev):
    import aligner_amd
    from aligner_amd import _lib
    c = bo.reference("past1024")[0]
    with pytest.raises(_lib.AlignerError) as err:
        aligner_amd.soft_dtw(torch.zeros(c.B, c.N, c.M, device=dev), bandwidth=c.w)
    assert err.value.code == _lib.EDOM
    value, _ = _run("past1024")
    assert np.isfinite(value).all()


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_flow_is_conserved_and_zero_where_no_cell_exists(dev, name):
    c, _, dense, *_ , stats = bo.reference(name)
    value, E = _run(name)
    exists = bo.exists_band(c)
    for b, st in enumerate(stats):
        if not st.feasible:
            assert value[b] == np.inf and not E[b].any()
            continue
        tol = 8 * (st.n + st.m) * 2.0 ** -24
        first, last = float(E[b, 0, c.w]), float(E[b, st.n - 1, st.m - st.n + c.w])
        print(f"{name}[{b}]: |E[0,0] - 1| = {abs(first - 1):.2e}, |E[n-1,m-1] - 1| = {abs(last - 1):.2e} (tolerance {tol:.2e})")
        assert abs(first - 1) <= tol and abs(last - 1) <= tol
        assert (E[b] >= 0).all()
        assert not E[b][~exists[b]].any()
        Ed = bo.to_dense(E[b:b + 1], c.M)[0]
        assert not Ed[~np.isfinite(dense[b])].any()                      # forbidden cells
        blk = Ed[:st.n, :st.m].astype(np.float64)
        assert blk.sum(1).min() >= 1 - 1e-5 and blk.sum(0).min() >= 1 - 1e-5


def test_infeasible_utterances_leave_their_neighbours_alone(dev):
    import aligner_amd
    c, _, _, band, *_ = bo.reference("ragged")
    value, E = _run("ragged")
    assert (value[4:] == np.inf).all() and not E[4:].any()
    keep = [0, 1, 2, 3]
    v2, E2 = aligner_amd.soft_dtw_banded(torch.tensor(band[keep]).to(dev), _i32([c.n[k] for k in keep], dev),
                                         _i32([c.m[k] for k in keep], dev), c.gamma, c.p)
    assert np.array_equal(v2.cpu().numpy(), value[keep]) and np.array_equal(E2.cpu().numpy(), E[keep])


@pytest.mark.parametrize("name", ["ragged", "w64", "wide", "steps32"])
def test_nan_where_no_cell_exists_changes_no_bit(dev, name):
    import aligner_amd
    c, _, _, band, *_ = bo.reference(name)
    value, E = _run(name)
    bad = band.copy()
    bad[~bo.exists_band(c)] = np.nan
    assert np.isnan(bad).any()
    v, e = aligner_amd.soft_dtw_banded(torch.tensor(bad).to(dev), _i32(c.n, dev), _i32(bo.m_of(c), dev), c.gamma, c.p)
    assert np.array_equal(v.cpu().numpy(), value) and np.array_equal(e.cpu().numpy(), E)


def test_nan_cost_stays_in_its_utterance(dev):
    import aligner_amd
    c, _, _, band, *_ = bo.reference("w31")
    cost = torch.tensor(np.concatenate([band, band[:1]])).to(dev)
    v0, E0 = aligner_amd.soft_dtw_banded(cost, gamma=1.0, warp_penalty=0.1)
    bad = cost.clone()
    bad[1, 20, c.w + 3] = float("nan")
    v1, E1 = aligner_amd.soft_dtw_banded(bad, gamma=1.0, warp_penalty=0.1)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert torch.equal(v0[b], v1[b]) and torch.equal(E0[b], E1[b])


def test_two_runs_give_the_same_bits(dev):
    import aligner_amd
    for name in ("ragged", "w127"):
        c, _, _, band, *_ = bo.reference(name)
        args = (torch.tensor(band).to(dev), _i32(c.n, dev), _i32(bo.m_of(c), dev), c.gamma, c.p)
        v0, E0 = aligner_amd.soft_dtw_banded(*args)
        v1, E1 = aligner_amd.soft_dtw_banded(*args)
        value, E = _run(name)
        assert torch.equal(v0, v1) and torch.equal(E0, E1)
        assert np.array_equal(v0.cpu().numpy(), value) and np.array_equal(E0.cpu().numpy(), E)
        v2, none = aligner_amd.soft_dtw_banded(*args, want_grad=False)
        assert none is None and torch.equal(v2, v0)


FENCE = 1024                                                   # floats of canary on either side


def _fenced(count, dev):
    buf = torch.full((FENCE + count + FENCE,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[FENCE:FENCE + count]


def _intact(buf, count):
    return bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + count:]).all())


@pytest.mark.parametrize("name", ["w0", "w63", "w64", "wide", "ragged", "steps31", "steps32", "past1024"])
def test_dp_stores_stay_inside_their_buffers(dev, name):
    """value, E_band and the workspace carved out of NaN-filled allocations, the C ABI called on the interior pointers."""
    from aligner_amd import _lib
    lib = _lib.load()
    c, _, _, band, *_ = bo.reference(name)
    B, N, W = band.shape
    vbuf, v = _fenced(B, dev)
    ebuf, e = _fenced(B * N * W, dev)
    nws = lib.aligner_soft_dtw_banded_workspace_bytes(B, N, c.w, 1)
    wbuf, w = _fenced(nws // 4, dev)
    cd = torch.tensor(band).to(dev)
    n, m = _i32(c.n, dev), _i32(bo.m_of(c), dev)
    _lib.check(lib.aligner_soft_dtw_banded_f32(cd.data_ptr(), None if n is None else n.data_ptr(), m.data_ptr(),
                                               c.gamma, c.p, c.w, v.data_ptr(), e.data_ptr(), w.data_ptr(), nws, B, N,
                                               torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    for buf, count in ((vbuf, B), (ebuf, B * N * W), (wbuf, nws // 4)):
        assert _intact(buf, count)
    value, E = _run(name)
    assert np.array_equal(v.cpu().numpy(), value) and np.array_equal(e.view(B, N, W).cpu().numpy(), E)
    assert not torch.isnan(e).any()


# ---- the L1 cost and its gradients in band layout ---------------------------------------------------------------------

def _cost_case(C, w, N=70, M=90, n=(70, 50), m=(66, 90), seed=0):
    return SimpleNamespace(B=2, C=C, N=N, M=M, w=w, n=n, m=m, scale=0.5, row_scale=(-1.5, 2.0), seed=seed)


COST_CASES = {f"c{C}_w{w}": _cost_case(C, w, seed=C * 1000 + w) for C in (1, 3, 8, 9) for w in (5, 64)}
COST_CASES["m_below_n"] = _cost_case(3, 5, N=70, M=40, n=(70, 33), m=(40, 40), seed=11)
COST_CASES["m_past_n_plus_w"] = _cost_case(3, 5, N=30, M=90, n=(30, 30), m=(90, 33), seed=12)


@functools.lru_cache(maxsize=None)
def _cost_reference(name):
    """(case, pred, target, G_band with NaN where no cell exists, exists [B,N,W], cost64 dense, dpred64, dtarget64 and
    their bounds) -- inputs quantised to 1/4 so that pred == target happens."""
    c = COST_CASES[name]
    rng = np.random.default_rng(c.seed)
    pred = (np.round(rng.uniform(-1.0, 1.0, (c.B, c.C, c.N)) * 4) / 4).astype(np.float32)
    target = (np.round(rng.uniform(-1.0, 1.0, (c.B, c.C, c.M)) * 4) / 4).astype(np.float32)
    exists = bo.exists_band(c)
    G = rng.normal(0.0, 1.0, exists.shape).astype(np.float32)
    G[~exists] = np.nan
    cost = lco.cost64(pred, target, c.n, c.m, c.w, c.scale)
    grads = lco.grads64(bo.to_dense(G, c.M, np.nan), pred, target, c.n, c.m, c.w, c.scale, c.row_scale)
    ok, _ = lco.exists(c.B, c.N, c.M, c.n, c.m, c.w)
    ties = ((pred[:, :, :, None] == target[:, :, None, :]) & ok[:, None]).sum() / max(ok.sum() * c.C, 1)
    assert ties > 0.05
    return (c, pred, target, G, exists, cost) + tuple(grads)


@functools.lru_cache(maxsize=None)
def _cost_run(name):
    import aligner_amd
    dev = torch.device("cuda:0")
    c, pred, target, G, *_ = _cost_reference(name)
    p, t, n, m = torch.tensor(pred).to(dev), torch.tensor(target).to(dev), _i32(c.n, dev), _i32(bo.m_of(c), dev)
    cost = aligner_amd.l1_cost_banded(p, t, n, m, c.w, c.scale)
    rs = torch.tensor(c.row_scale, dtype=torch.float32, device=dev)
    dpred, dtarget = aligner_amd.l1_cost_banded_backward(torch.tensor(G).to(dev), p, t, n, m, c.scale, rs)
    only_p, none1 = aligner_amd.l1_cost_banded_backward(torch.tensor(G).to(dev), p, t, n, m, c.scale, rs, want=(True, False))
    none2, only_t = aligner_amd.l1_cost_banded_backward(torch.tensor(G).to(dev), p, t, n, m, c.scale, rs, want=(False, True))
    torch.cuda.synchronize()
    assert none1 is None and none2 is None
    return tuple(x.cpu().numpy() for x in (cost, dpred, dtarget, only_p, only_t))


def _ratio(got, want, bound, label, name):
    got = np.asarray(got, np.float64)
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got - want)
    none = bound == 0
    assert not got[none].any(), f"{name}: {label} is not exactly 0 where no cell exists"
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    print(f"{name}: {label} error / bound {r.max():.3f}, {int(none.sum())} of {none.size} elements without a cell")
    return float(r.max())


@pytest.mark.parametrize("name", list(COST_CASES))
def test_cost_and_gradients_in_band_layout_inside_the_bounds(dev, name):
    c, pred, target, G, exists, cost64, dp64, dt64, bp, bt = _cost_reference(name)
    cost, dpred, dtarget, only_p, only_t = _cost_run(name)
    assert cost.shape == exists.shape and not cost[~exists].any()          # exactly 0 where no cell exists
    want = bo.to_band(np.where(np.isfinite(cost64), cost64, 0.0), c.w)
    err, bound = np.abs(cost[exists].astype(np.float64) - want[exists]), (c.C + 2) * lco.U * np.abs(want[exists])
    with np.errstate(invalid="ignore", divide="ignore"):
        rc = float(np.where(err == 0, 0.0, err / bound).max()) if err.size else 0.0
    print(f"{name}: cost error / bound {rc:.3f} over {int(exists.sum())} cells")
    rp, rt = _ratio(dpred, dp64, bp, "dpred", name), _ratio(dtarget, dt64, bt, "dtarget", name)
    assert rc <= 1.0 and rp <= 1.0 and rt <= 1.0
    assert np.array_equal(only_p, dpred) and np.array_equal(only_t, dtarget)


@pytest.mark.parametrize("name", ["c9_w5", "c3_w64", "m_below_n", "m_past_n_plus_w"])
def test_cost_stores_stay_inside_their_buffers_and_two_runs_agree(dev, name):
    from aligner_amd import _lib
    lib = _lib.load()
    c, pred, target, G, *_ = _cost_reference(name)
    W = 2 * c.w + 1
    p, t, g = torch.tensor(pred).to(dev), torch.tensor(target).to(dev), torch.tensor(G).to(dev)
    n, m = _i32(c.n, dev), _i32(bo.m_of(c), dev)
    rs = torch.tensor(c.row_scale, dtype=torch.float32, device=dev)
    cbuf, cost = _fenced(c.B * c.N * W, dev)
    pbuf, dpred = _fenced(c.B * c.C * c.N, dev)
    tbuf, dtarget = _fenced(c.B * c.C * c.M, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.aligner_l1_cost_banded_f32(p.data_ptr(), t.data_ptr(), n.data_ptr(), m.data_ptr(), c.w, c.scale, cost.data_ptr(),
                                              c.B, c.C, c.N, c.M, stream))
    _lib.check(lib.aligner_l1_cost_banded_backward_f32(g.data_ptr(), p.data_ptr(), t.data_ptr(), n.data_ptr(), m.data_ptr(), c.w,
                                                       c.scale, rs.data_ptr(), dpred.data_ptr(), dtarget.data_ptr(),
                                                       c.B, c.C, c.N, c.M, stream))
    torch.cuda.synchronize()
    for buf, count in ((cbuf, cost.numel()), (pbuf, dpred.numel()), (tbuf, dtarget.numel())):
        assert _intact(buf, count)
    cost0, dpred0, dtarget0, *_ = _cost_run(name)
    assert np.array_equal(cost.view(c.B, c.N, W).cpu().numpy(), cost0)
    assert np.array_equal(dpred.view(c.B, c.C, c.N).cpu().numpy(), dpred0)
    assert np.array_equal(dtarget.view(c.B, c.C, c.M).cpu().numpy(), dtarget0)


# ---- soft_dtw_l1_banded_loss ----------------------------------------------------------------------------------------------

GAMMA, PENALTY = 1.0, 0.1


def _loss_operands(dev, w=30):
    """[3,8,100,120] with lengths that leave utterance 1 without an alignment at w = 30 (|n - m| = 35)."""
    rng = np.random.default_rng(5)
    pred = torch.tensor(rng.uniform(-1, 1, (3, 8, 100)).astype(np.float32)).to(dev)
    target = torch.tensor(rng.uniform(-1, 1, (3, 8, 120)).astype(np.float32)).to(dev)
    return pred, target, (100, 60, 90), (120, 95, 110), w


def test_loss_value_is_the_composition_and_gradients_agree_with_the_dense_loss(dev):
    """value: the bits of soft_dtw_banded(l1_cost_banded(...)).  Gradients against soft_dtw_l1_loss on the same inputs and
    band, inside the sum of the two bounds of l1cost_oracle (GRAD of the band sums plus GRAD of the dense sums): the two
    backward sweeps run the same cell code on the same R, so the two E must not add anything to that."""
    import aligner_amd
    pred, target, ns, ms, w = _loss_operands(dev)
    n, m = _i32(ns, dev), _i32(ms, dev)
    scale = 1.0 / 8
    up = np.array([1.5, -2.0, 0.75], np.float32)
    grads = {}
    for kind in ("band", "dense"):
        p, t = pred.clone().requires_grad_(), target.clone().requires_grad_()
        if kind == "band":
            value = aligner_amd.soft_dtw_l1_banded_loss(p, t, n, m, GAMMA, PENALTY, w, scale, reduction="none")
            cost = aligner_amd.l1_cost_banded(pred, target, n, m, w, scale)
            parts, E = aligner_amd.soft_dtw_banded(cost, n, m, GAMMA, PENALTY)
            assert torch.equal(value, parts)
            Ed = bo.to_dense(E.cpu().numpy(), 120)
        else:
            value = aligner_amd.soft_dtw_l1_loss(p, t, n, m, GAMMA, PENALTY, w, scale, reduction="none")
            _, E = aligner_amd.soft_dtw(aligner_amd.l1_cost(pred, target, n, m, w, scale), n, m, GAMMA, PENALTY, w)
            Ed = E.cpu().numpy()
        assert torch.isinf(value[1]) and torch.isfinite(value[[0, 2]]).all()
        value.backward(torch.tensor(up).to(dev))
        exact = lco.grads64(Ed, pred.cpu().numpy(), target.cpu().numpy(), ns, ms, w, scale, up)
        grads[kind] = (value.detach().cpu().numpy(), p.grad.cpu().numpy(), t.grad.cpu().numpy(), Ed.astype(np.float64), exact)
    vb, pb, tb, Eb, (dpb, dtb, bpb, btb) = grads["band"]
    vd, pd, td, Edn, (dpd, dtd, bpd, btd) = grads["dense"]
    assert np.array_equal(vb, vd)                                           # the forward values share their bits
    assert _ratio(pb, dpb, bpb, "dpred (band loss)", "loss") <= 1.0 and _ratio(tb, dtb, btb, "dtarget (band loss)", "loss") <= 1.0
    print(f"loss: largest |E_band - E_dense| {np.abs(Eb - Edn).max():.2e}, largest |dpred_band - dpred_dense| / bound "
          f"{(np.abs(pb.astype(np.float64) - pd) / np.maximum(bpb + bpd, 1e-300)).max():.3f}, dtarget "
          f"{(np.abs(tb.astype(np.float64) - td) / np.maximum(btb + btd, 1e-300)).max():.3f}")
    assert (np.abs(pb.astype(np.float64) - pd) <= bpb + bpd).all()
    assert (np.abs(tb.astype(np.float64) - td) <= btb + btd).all()
    assert not pb[1].any() and not tb[1].any() and pb[0].any() and tb[2].any()


def test_loss_zero_infinity_half_precision_and_an_input_without_a_gradient(dev):
    import aligner_amd
    pred, target, ns, ms, w = _loss_operands(dev)
    n, m = _i32(ns, dev), _i32(ms, dev)
    assert torch.isinf(aligner_amd.soft_dtw_l1_banded_loss(pred, target, n, m, GAMMA, PENALTY, w))
    zi = aligner_amd.soft_dtw_l1_banded_loss(pred, target, n, m, GAMMA, PENALTY, w, reduction="none", zero_infinity=True)
    assert zi[1] == 0 and torch.isfinite(zi).all() and zi.shape == (3,)
    pb, tb = pred.to(torch.bfloat16).requires_grad_(), target.to(torch.bfloat16).requires_grad_()
    aligner_amd.soft_dtw_l1_banded_loss(pb, tb, n, m, GAMMA, PENALTY, w, reduction="sum", zero_infinity=True).backward()
    assert pb.grad.dtype == torch.bfloat16 and tb.grad.dtype == torch.bfloat16
    assert not pb.grad[1].any() and pb.grad[0].any() and torch.isfinite(pb.grad.float()).all()
    pf, tf = pb.detach().float().requires_grad_(), tb.detach().float()     # (the same fp32 kernels on the bf16 values)
    aligner_amd.soft_dtw_l1_banded_loss(pf, tf, n, m, GAMMA, PENALTY, w, reduction="sum", zero_infinity=True).backward()
    assert tf.grad is None
    assert torch.equal(pb.grad, pf.grad.to(torch.bfloat16))
    # m = None: the target's own length, which the DP has to be told
    full = aligner_amd.soft_dtw_l1_banded_loss(pred[:, :, :110], target, None, None, GAMMA, PENALTY, w, reduction="none")
    want = aligner_amd.soft_dtw_l1_loss(pred[:, :, :110], target, None, None, GAMMA, PENALTY, w, reduction="none")
    assert torch.equal(full, want)


def test_banded_loss_scales_the_expected_alignment(dev):
    import aligner_amd
    c, _, _, band, *_ = bo.reference("ragged")
    _, E = _run("ragged")
    x = torch.tensor(band).to(dev).requires_grad_()
    up = torch.tensor([1.0, -2.0, 0.5, 3.0, 0.0, 1.5], device=dev)
    loss = aligner_amd.soft_dtw_banded_loss(x, _i32(c.n, dev), _i32(bo.m_of(c), dev), c.gamma, c.p, reduction="none")
    assert torch.isinf(loss[4:]).all()
    (torch.where(torch.isinf(loss), torch.zeros_like(loss), loss) * up).sum().backward()
    assert torch.equal(x.grad, torch.from_numpy(E).to(dev) * up.view(-1, 1, 1))
