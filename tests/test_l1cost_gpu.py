"""l1_cost() / l1_cost_backward() / soft_dtw_l1_loss() on the GPU against the float64 oracle (tests/l1cost_oracle.py)
inside its derived bounds, on the smallest shapes at which tiling, tails and the band of csrc/l1cost.hip can go wrong
(l1cost_oracle.CASES).  G carries a NaN at every cell that does not exist.  Then what needs no oracle: the fill values
are exact, a NaN stays in its utterance, two runs give the same bits, each output alone has the bits it has beside the
other, stores stay inside their buffers, and the autograd face.  Every comparison prints observed / bound."""
import functools

import numpy as np
import pytest
import torch

import l1cost_oracle as orc

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
    """One GPU run per case, shared by the tests: (cost, dpred, dtarget) as numpy arrays."""
    import aligner_amd
    dev = torch.device("cuda:0")
    c, pred, target, G, n, m = _operands(name, dev)
    cost = aligner_amd.l1_cost(pred, target, n, m, c.band, c.scale)
    dpred, dtarget = aligner_amd.l1_cost_backward(G, pred, target, n, m, c.band, c.scale, _f32(c.row_scale, dev))
    torch.cuda.synchronize()
    return cost.cpu().numpy(), dpred.cpu().numpy(), dtarget.cpu().numpy()


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_cost_and_gradients_inside_the_bounds(dev, name):
    cost, dpred, dtarget = _run(name)
    rc = orc.check_cost(name, cost, "GPU")                     # (asserts the exact fill values as well)
    rp, rt = orc.check_grads(name, dpred, dtarget, "GPU")
    assert rc <= 1.0 and rp <= 1.0 and rt <= 1.0


@pytest.mark.parametrize("name", ["edges", "band0", "band30", "scaled"])
def test_fill_values_are_exact(dev, name):
    c = orc.CASES[name]
    cost, dpred, dtarget = _run(name)
    ok, inside = orc.exists(c.B, c.N, c.M, c.n, c.m, c.band)
    assert np.isfinite(cost[ok]).all()
    assert (cost[inside & ~ok] == np.inf).all() and not cost[~inside].any()
    n, m = orc.lengths(c.n, c.B, c.N), orc.lengths(c.m, c.B, c.M)
    for b in range(c.B):
        assert not dpred[b, :, n[b]:].any() and not dtarget[b, :, m[b]:].any()
    assert np.isfinite(dpred).all() and np.isfinite(dtarget).all()          # none of G's NaNs came through


def test_no_limit_on_the_rows(dev):
    """N <= 1024 is the DP's limit, not the cost's."""
    import aligner_amd
    rng = np.random.default_rng(11)
    pred, target = rng.uniform(-1, 1, (1, 2, 1500)).astype(np.float32), rng.uniform(-1, 1, (1, 2, 3)).astype(np.float32)
    cost = aligner_amd.l1_cost(torch.tensor(pred).to(dev), torch.tensor(target).to(dev), bandwidth=1200).cpu().numpy()
    want = orc.cost64(pred, target, band=1200)
    fin = np.isfinite(want)
    assert np.array_equal(cost[~fin], want[~fin]) and (~fin).sum() == 299 + 298 + 297
    assert (np.abs(cost[fin] - want[fin]) <= 4 * orc.U * want[fin]).all()


def test_nan_stays_in_its_utterance(dev):
    import aligner_amd
    c, pred, target, G, n, m = _operands("edges", dev)
    bad = pred.clone()
    bad[1, 0, 5] = float("nan")
    bad[1, 2, 63] = float("nan")
    cost = aligner_amd.l1_cost(bad, target, n, m, c.band, c.scale)
    dpred, dtarget = aligner_amd.l1_cost_backward(G, bad, target, n, m, c.band, c.scale)
    torch.cuda.synchronize()
    cost0, dpred0, dtarget0 = _run("edges")
    assert torch.isnan(cost[1, 5, :128]).all()
    for b in (0, 2, 3, 4, 5):
        assert np.array_equal(cost[b].cpu().numpy(), cost0[b])
        assert np.array_equal(dpred[b].cpu().numpy(), dpred0[b]) and np.array_equal(dtarget[b].cpu().numpy(), dtarget0[b])


@pytest.mark.parametrize("name", ["edges", "band30", "scaled"])
def test_two_runs_give_the_same_bits_and_each_output_alone_too(dev, name):
    import aligner_amd
    c, pred, target, G, n, m = _operands(name, dev)
    rs = _f32(c.row_scale, dev)
    cost0, dpred0, dtarget0 = _run(name)
    cost = aligner_amd.l1_cost(pred, target, n, m, c.band, c.scale)
    dpred, dtarget = aligner_amd.l1_cost_backward(G, pred, target, n, m, c.band, c.scale, rs)
    assert np.array_equal(cost.cpu().numpy(), cost0)
    assert np.array_equal(dpred.cpu().numpy(), dpred0) and np.array_equal(dtarget.cpu().numpy(), dtarget0)
    only_p, none = aligner_amd.l1_cost_backward(G, pred, target, n, m, c.band, c.scale, rs, want=(True, False))
    assert none is None and np.array_equal(only_p.cpu().numpy(), dpred0)
    none, only_t = aligner_amd.l1_cost_backward(G, pred, target, n, m, c.band, c.scale, rs, want=(False, True))
    assert none is None and np.array_equal(only_t.cpu().numpy(), dtarget0)


@pytest.mark.parametrize("name", ["one", "edges", "channels129", "tall", "band30", "scaled"])
def test_stores_stay_inside_their_buffers(dev, name):
    """cost, dpred and dtarget carved out of NaN-filled allocations, the C ABI called on the interior pointers: the
    canaries are intact and the results are the wrapper's.  (Neither call has a workspace.)"""
    from aligner_amd import _lib
    lib = _lib.load()
    c, pred, target, G, n, m = _operands(name, dev)
    rs = _f32(c.row_scale, dev)
    fence = 1024                                               # floats of canary on either side

    def fenced(count):
        buf = torch.full((fence + count + fence,), float("nan"), dtype=torch.float32, device=dev)
        return buf, buf[fence:fence + count]

    cbuf, cost = fenced(c.B * c.N * c.M)
    pbuf, dpred = fenced(c.B * c.C * c.N)
    tbuf, dtarget = fenced(c.B * c.C * c.M)
    ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    stream = torch.cuda.current_stream(dev).cuda_stream
    band = -1 if c.band is None else c.band
    _lib.check(lib.aligner_l1_cost_f32(pred.data_ptr(), target.data_ptr(), ptr(n), ptr(m), band, c.scale, cost.data_ptr(),
                                       c.B, c.C, c.N, c.M, stream))
    _lib.check(lib.aligner_l1_cost_backward_f32(G.data_ptr(), pred.data_ptr(), target.data_ptr(), ptr(n), ptr(m), band, c.scale,
                                                ptr(rs), dpred.data_ptr(), dtarget.data_ptr(), c.B, c.C, c.N, c.M, stream))
    torch.cuda.synchronize()
    for buf, count in ((cbuf, cost.numel()), (pbuf, dpred.numel()), (tbuf, dtarget.numel())):
        assert bool(torch.isnan(buf[:fence]).all()) and bool(torch.isnan(buf[fence + count:]).all())
    cost0, dpred0, dtarget0 = _run(name)
    assert np.array_equal(cost.view(c.B, c.N, c.M).cpu().numpy(), cost0)
    assert np.array_equal(dpred.view(c.B, c.C, c.N).cpu().numpy(), dpred0)
    assert np.array_equal(dtarget.view(c.B, c.C, c.M).cpu().numpy(), dtarget0)
    assert not torch.isnan(cost).any() and not torch.isnan(dpred).any() and not torch.isnan(dtarget).any()


# ---- soft_dtw_l1_loss ----------------------------------------------------------------------------------------------

GAMMA, PENALTY = 1.0, 0.1


@pytest.mark.parametrize("name", ["edges", "band30", "scaled"])
def test_loss_value_is_the_composition_and_its_gradients_are_inside_the_bound(dev, name):
    """value: the bits of soft_dtw_loss(l1_cost(...)).  Gradients: the oracle fed with the GPU's own E and the upstream
    gradient as row_scale, so that only the arithmetic of l1_cost_backward is judged."""
    import aligner_amd
    c, pred, target, _, n, m = _operands(name, dev)
    pred.requires_grad_()
    target.requires_grad_()
    value = aligner_amd.soft_dtw_l1_loss(pred, target, n, m, GAMMA, PENALTY, c.band, c.scale, reduction="none")
    cost = aligner_amd.l1_cost(pred, target, n, m, c.band, c.scale)
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
    value = aligner_amd.soft_dtw_l1_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="none")
    assert torch.isinf(value[1]) and torch.isfinite(value[[0, 2, 3]]).all()
    assert torch.isinf(aligner_amd.soft_dtw_l1_loss(pred, target, n, m, GAMMA, PENALTY, c.band))
    zi = aligner_amd.soft_dtw_l1_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="none", zero_infinity=True)
    assert zi[1] == 0 and torch.equal(zi[[0, 2, 3]], value[[0, 2, 3]])
    aligner_amd.soft_dtw_l1_loss(pred, target, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert not pred.grad[1].any() and not target.grad[1].any()
    for b in (0, 2, 3):
        assert pred.grad[b].any() and target.grad[b].any()
    assert torch.isfinite(pred.grad).all() and torch.isfinite(target.grad).all()


def test_loss_half_precision_and_an_input_without_a_gradient(dev):
    import aligner_amd
    c, pred, target, _, n, m = _operands("band30", dev)
    pb, tb = pred.to(torch.bfloat16).requires_grad_(), target.to(torch.bfloat16).requires_grad_()
    aligner_amd.soft_dtw_l1_loss(pb, tb, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert pb.grad.dtype == torch.bfloat16 and tb.grad.dtype == torch.bfloat16
    # (the same fp32 kernels on the bf16 values)
    pf, tf = pb.detach().float().requires_grad_(), tb.detach().float()
    assert not tf.requires_grad
    aligner_amd.soft_dtw_l1_loss(pf, tf, n, m, GAMMA, PENALTY, c.band, reduction="sum", zero_infinity=True).backward()
    assert tf.grad is None                                               # None came back for the target
    assert torch.equal(pb.grad, pf.grad.to(torch.bfloat16))

def test_loss_agrees_with_the_cdist_composition(dev):
    """The comparison, and the tolerances, of test_gradient_reaches_the_prediction_through_cdist."""
    import aligner_amd
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(2, 50, 8, generator=g).to(dev).requires_grad_()                 # [B,T,C]
    target = torch.rand(2, 70, 8, generator=g).to(dev).requires_grad_()
    want = aligner_amd.soft_dtw_loss(torch.cdist(pred, target, p=1) * (1 / 8), gamma=1.0, warp_penalty=0.1, bandwidth=40, reduction="sum")
    want.backward()
    p2 = pred.detach().transpose(1, 2).contiguous().requires_grad_()                  # [B,C,T]
    t2 = target.detach().transpose(1, 2).contiguous().requires_grad_()
    got = aligner_amd.soft_dtw_l1_loss(p2, t2, gamma=1.0, warp_penalty=0.1, bandwidth=40, scale=1 / 8, reduction="sum")
    got.backward()
    dv = abs(got.item() - want.item()) / abs(want.item())
    dp = (p2.grad.transpose(1, 2) - pred.grad).abs().max().item()
    dt = (t2.grad.transpose(1, 2) - target.grad).abs().max().item()
    print(f"fused against cdist composition: value {dv:.2e} relative, dpred {dp:.2e}, dtarget {dt:.2e} absolute "
          f"(largest |dpred| {pred.grad.abs().max().item():.2e})")
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-6)
    assert torch.allclose(p2.grad.transpose(1, 2), pred.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(t2.grad.transpose(1, 2), target.grad, rtol=1e-4, atol=1e-6)
