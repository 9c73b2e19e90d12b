"""soft_dtw() / soft_dtw_loss() on the GPU against the float64 oracle (tests/softdtw_oracle.py) inside its derived bounds,
on the smallest shapes at which each mechanism of csrc/softdtw.hip can break (softdtw_oracle.CASES): rows across the wave
and lane edges, columns across the tile edges, N > M and N < M, the largest text, a ragged batch, band and penalty with
an utterance the band excludes, forbidden (+inf) blocks with and without a way round them.  Then the properties that need
no oracle: the flow is conserved, E is exactly 0 outside the utterance and the band, a NaN stays in its utterance, stores
stay inside their buffers, two runs give the same bits, and the autograd face.  Every comparison prints observed / bound."""
import functools

import numpy as np
import pytest
import torch

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
    """One GPU run per case, shared by the tests: (value, E) as numpy arrays."""
    import aligner_amd
    dev = torch.device("cuda:0")
    c, cost, *_ = orc.reference(name)
    value, E = aligner_amd.soft_dtw(torch.tensor(cost).to(dev), _i32(c.n, dev), _i32(c.m, dev), c.gamma, c.p, c.band)
    torch.cuda.synchronize()
    return value.cpu().numpy(), E.cpu().numpy()


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_value_and_expected_alignment_inside_the_bounds(dev, name):
    value, E = _run(name)
    rv, rg = orc.check(name, value, E, "GPU")
    assert rv <= 1.0 and rg <= 1.0


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_flow_is_conserved_and_zero_outside(dev, name):
    """Needs no oracle: E[0,0] and E[n-1,m-1] are 1 to 8 (n+m) 2^-24, every row and column inside [n,m] carries at least
    the whole flow, and E is exactly 0 at and past n, at and past m, and outside the band."""
    c, cost, want_value, _, stats = orc.reference(name)
    value, E = _run(name)
    for b, st in enumerate(stats):
        if not st.feasible:
            assert value[b] == np.inf and not E[b].any()
            continue
        blk = E[b, :st.n, :st.m].astype(np.float64)
        tol = 8 * (st.n + st.m) * 2.0 ** -24
        print(f"{name}[{b}]: |E[0,0] - 1| = {abs(blk[0, 0] - 1):.2e}, |E[n-1,m-1] - 1| = {abs(blk[-1, -1] - 1):.2e} (tolerance {tol:.2e}); "
              f"smallest row sum {blk.sum(1).min():.7f}, column sum {blk.sum(0).min():.7f}")
        assert abs(blk[0, 0] - 1) <= tol and abs(blk[-1, -1] - 1) <= tol
        assert blk.sum(1).min() >= 1 - 1e-5 and blk.sum(0).min() >= 1 - 1e-5
        assert (blk >= 0).all()
        assert not E[b, st.n:].any() and not E[b, :, st.m:].any()
        if c.band is not None:
            i, j = np.mgrid[0:c.N, 0:c.M]
            assert not E[b][np.abs(i - j) > c.band].any()
        assert not E[b][~np.isfinite(cost[b]) & (cost[b] > 0)].any()          # forbidden cells


def test_band_excludes_an_utterance_and_leaves_its_neighbours_alone(dev):
    """Utterance 1 of the band cases has |n - m| = 35 > 30: +inf and a zero E; the others have the bits they have in a
    batch without it."""
    import aligner_amd
    for name in ("band_p0", "band_p05"):
        c, cost, *_ = orc.reference(name)
        value, E = _run(name)
        assert value[1] == np.inf and not E[1].any()
        keep = [0, 2, 3]
        v2, E2 = aligner_amd.soft_dtw(torch.tensor(cost[keep]).to(dev), _i32([c.n[k] for k in keep], dev),
                                      _i32([c.m[k] for k in keep], dev), c.gamma, c.p, c.band)
        assert np.array_equal(v2.cpu().numpy(), value[keep]) and np.array_equal(E2.cpu().numpy(), E[keep])


def test_nan_cost_stays_in_its_utterance(dev):
    import aligner_amd
    cost = torch.from_numpy(orc.uniform_cost(3, 70, 90, seed=3)).to(dev)
    v0, E0 = aligner_amd.soft_dtw(cost, gamma=1.0, warp_penalty=0.1)
    bad = cost.clone()
    bad[1, 20, 30] = float("nan")
    bad[1, 64, 0] = float("nan")
    v1, E1 = aligner_amd.soft_dtw(bad, gamma=1.0, warp_penalty=0.1)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert torch.equal(v0[b], v1[b]) and torch.equal(E0[b], E1[b])


def test_two_runs_give_the_same_bits(dev):
    import aligner_amd
    c, cost, *_ = orc.reference("ragged")
    args = (torch.tensor(cost).to(dev), _i32(c.n, dev), _i32(c.m, dev), c.gamma, c.p, c.band)
    v0, E0 = aligner_amd.soft_dtw(*args)
    v1, E1 = aligner_amd.soft_dtw(*args)
    value, E = _run("ragged")
    assert torch.equal(v0, v1) and torch.equal(E0, E1)
    assert np.array_equal(v0.cpu().numpy(), value) and np.array_equal(E0.cpu().numpy(), E)
    v2, none = aligner_amd.soft_dtw(*args, want_grad=False)
    assert none is None and torch.equal(v2, v0)


@pytest.mark.parametrize("name", ["rows1", "cols1", "rows129", "cols130", "ragged", "band_p05", "largest_text"])
def test_stores_stay_inside_their_buffers(dev, name):
    """value, E and the workspace carved out of NaN-filled allocations, the C ABI called on the interior pointers: the
    canaries are intact and the results are the wrapper's."""
    from aligner_amd import _lib
    lib = _lib.load()
    c, cost, *_ = orc.reference(name)
    B, N, M = cost.shape
    band = 1024                                                # floats of canary on either side

    def fenced(count):
        buf = torch.full((band + count + band,), float("nan"), dtype=torch.float32, device=dev)
        return buf, buf[band:band + count]

    vbuf, v = fenced(B)
    ebuf, e = fenced(B * N * M)
    nws = lib.aligner_soft_dtw_workspace_bytes(B, N, M, 1)
    wbuf, w = fenced(nws // 4)
    cd = torch.tensor(cost).to(dev)
    n, m = _i32(c.n, dev), _i32(c.m, dev)
    _lib.check(lib.aligner_soft_dtw_f32(cd.data_ptr(), None if n is None else n.data_ptr(), None if m is None else m.data_ptr(),
                                        c.gamma, c.p, -1 if c.band is None else c.band, v.data_ptr(), e.data_ptr(),
                                        w.data_ptr(), nws, B, N, M, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    for buf, count in ((vbuf, B), (ebuf, B * N * M), (wbuf, nws // 4)):
        assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + count:]).all())
    value, E = _run(name)
    assert np.array_equal(v.cpu().numpy(), value) and np.array_equal(e.view(B, N, M).cpu().numpy(), E)
    assert not torch.isnan(e).any()


def test_autograd_scales_the_expected_alignment(dev):
    import aligner_amd
    c, cost, *_ = orc.reference("ragged")
    _, E = _run("ragged")
    x = torch.tensor(cost).to(dev).requires_grad_()
    up = torch.tensor([1.0, -2.0, 0.5, 3.0, 0.0, 1.5], device=dev)
    loss = aligner_amd.soft_dtw_loss(x, _i32(c.n, dev), _i32(c.m, dev), c.gamma, c.p, c.band, reduction="none")
    (loss * up).sum().backward()
    assert torch.equal(x.grad, torch.from_numpy(E).to(dev) * up.view(-1, 1, 1))
    x.grad = None
    aligner_amd.soft_dtw_loss(x, _i32(c.n, dev), _i32(c.m, dev), c.gamma, c.p, c.band).backward()
    assert torch.allclose(x.grad, torch.from_numpy(E).to(dev) / 6, rtol=1e-6, atol=0)


def test_autograd_half_precision_and_zero_infinity(dev):
    import aligner_amd
    c, cost, *_ = orc.reference("band_p05")
    n, m = _i32(c.n, dev), _i32(c.m, dev)
    xb = torch.tensor(cost).to(dev).to(torch.bfloat16).requires_grad_()
    loss = aligner_amd.soft_dtw_loss(xb, n, m, c.gamma, c.p, c.band, reduction="sum", zero_infinity=True)
    assert torch.isfinite(loss)
    loss.backward()
    assert xb.grad.dtype == torch.bfloat16 and not xb.grad[1].any() and xb.grad[0].any()
    # (the same fp32 kernels on the bf16 values)
    v32, E32 = aligner_amd.soft_dtw(xb.detach().float(), n, m, c.gamma, c.p, c.band)
    assert torch.equal(xb.grad, E32.to(torch.bfloat16))
    assert torch.equal(loss, v32[[0, 2, 3]].sum()) or torch.allclose(loss, v32[[0, 2, 3]].sum(), rtol=1e-6)
    x = torch.tensor(cost).to(dev).requires_grad_()
    assert torch.isinf(aligner_amd.soft_dtw_loss(x, n, m, c.gamma, c.p, c.band))
    none = aligner_amd.soft_dtw_loss(x, n, m, c.gamma, c.p, c.band, reduction="none", zero_infinity=True)
    assert none[1] == 0 and none.shape == (4,)


def test_gradient_reaches_the_prediction_through_cdist(dev):
    import aligner_amd
    g = torch.Generator().manual_seed(0)
    pred = torch.rand(2, 50, 8, generator=g).to(dev).requires_grad_()
    target = torch.rand(2, 70, 8, generator=g).to(dev)
    cost = torch.cdist(pred, target, p=1) / 8
    cost.retain_grad()
    aligner_amd.soft_dtw_loss(cost, gamma=1.0, warp_penalty=0.1, bandwidth=40, reduction="sum").backward()
    assert pred.grad is not None and torch.isfinite(pred.grad).all() and pred.grad.abs().sum() > 0
    # d loss / d pred[i] = sum_j E[i,j] sign(pred[i] - target[j]) / 8
    want = (cost.grad.unsqueeze(3) * torch.sign(pred.detach().unsqueeze(2) - target.unsqueeze(1)) / 8).sum(2)
    assert torch.allclose(pred.grad, want, rtol=1e-4, atol=1e-6)
