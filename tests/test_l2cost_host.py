"""Host-side checks of l2_cost / l2_cost_backward / soft_dtw_l2_loss and their band-storage forms (no GPU): the float64
oracle (tests/l2cost_oracle.py) equals torch.cdist(p=2), its square and their autograd gradients on the small cases; an
fp32 numpy evaluation sits inside the oracle's bounds; the bounds catch a missing factor 2, a sign error and a leaking
fill; the four new C entry points validate their arguments before they look for a device; the wrappers reject what
they document."""
import math

import numpy as np
import pytest
import torch

import l2cost_oracle as orc

SMALL = [name for name in orc.CASE_NAMES if name not in ("tall", "channels129")]


@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_cdist_and_its_autograd_gradient(name):
    c, pred, target, G, sq, rt, dp, dt, _, _ = orc.reference(name)
    ok, _ = orc.exists(c.B, c.N, c.M, c.n, c.m, c.band)
    n, m = orc.lengths(c.n, c.B, c.N), orc.lengths(c.m, c.B, c.M)
    g = np.ones(c.B) if c.row_scale is None else np.asarray(c.row_scale, np.float64)
    worst = 0.0
    for b in range(c.B):
        x = torch.tensor(pred[b, :, :n[b]].T.astype(np.float64), requires_grad=True)            # [n,C]
        y = torch.tensor(target[b, :, :m[b]].T.astype(np.float64), requires_grad=True)          # [m,C]
        okb = ok[b, :n[b], :m[b]]
        if not okb.any():
            assert not dp[b].any() and not dt[b].any()
            continue
        D = torch.cdist(x, y, p=2, compute_mode="donot_use_mm_for_euclid_dist")
        assert np.allclose((D * c.scale).detach().numpy()[okb], rt[b, :n[b], :m[b]][okb], rtol=1e-12, atol=1e-15)
        assert np.allclose((D ** 2 * c.scale).detach().numpy()[okb], sq[b, :n[b], :m[b]][okb], rtol=1e-12, atol=1e-15)
        w = torch.tensor(np.where(okb, G[b, :n[b], :m[b]].astype(np.float64), 0.0))
        # the square of cdist through autograd; at distance 0 it has the gradient 0 * inf, and there the sum of squares
        # written out stands in for it
        if bool((D > 0).all()):
            S = D ** 2 * c.scale
        else:
            S = ((x[:, None, :] - y[None, :, :]) ** 2).sum(2) * c.scale
        (S * w).sum().mul(g[b]).backward()
        scale = max(np.abs(dp[b]).max(), np.abs(dt[b]).max(), 1e-300)
        worst = max(worst, np.abs(x.grad.numpy().T - dp[b, :, :n[b]]).max() / scale, np.abs(y.grad.numpy().T - dt[b, :, :m[b]]).max() / scale)
        assert not dp[b, :, n[b]:].any() and not dt[b, :, m[b]:].any()
    print(f"{name}: oracle against autograd, largest difference / largest gradient {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_an_fp32_evaluation_is_inside_the_bounds(name):
    c, pred, target, G, *_ = orc.reference(name)
    rs = orc.check_cost(name, orc.cost32(pred, target, c.n, c.m, c.band, c.scale, True), True, "fp32 numpy")
    rr = orc.check_cost(name, orc.cost32(pred, target, c.n, c.m, c.band, c.scale, False), False, "fp32 numpy")
    dp, dt = orc.grads32(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    rp, rt = orc.check_grads(name, dp, dt, "fp32 numpy")
    assert rs <= 1.0 and rr <= 1.0 and rp <= 1.0 and rt <= 1.0


def test_the_bounds_catch_a_missing_factor_a_wrong_sign_and_a_leaking_fill():
    c, pred, target, G, *_ = orc.reference("band30")
    dp, dt = orc.grads32(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    rp, rt = orc.check_grads("band30", dp, dt, "as it should be")
    assert rp <= 1.0 and rt <= 1.0
    rp, _ = orc.check_grads("band30", dp * np.float32(0.5), dt, "factor 2 missing")
    assert rp > 1.0
    _, rt = orc.check_grads("band30", dp, -dt, "dtarget with dpred's sign")
    assert rt > 1.0
    for squared in (True, False):
        cost = orc.cost32(pred, target, c.n, c.m, c.band, c.scale, squared)
        assert orc.check_cost("band30", cost, squared, "as it should be") <= 1.0
        assert cost[1, 100, 100] == 0                                         # (n[1] = 95: past the length)
        cost[1, 100, 100] = np.inf                                            # +inf where 0 belongs
        with pytest.raises(AssertionError):
            orc.check_cost("band30", cost, squared, "leaking fill")
    # and a root where the square belongs, or the other way round
    assert orc.check_cost("band30", orc.cost32(pred, target, c.n, c.m, c.band, c.scale, False), True, "root for squared") > 1.0


def test_abi_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = torch.zeros(64, dtype=torch.float32)
    q = buf.data_ptr()
    ok = dict(G=q, pred=q, target=q, n=None, m=None, band=-1, scale=1.0, rs=None, cost=q, dpred=q, dtarget=q, B=1, C=2, N=4, M=4)

    def forward(fn, squared, **kw):
        a = dict(ok, **kw)
        return fn(a["pred"], a["target"], a["n"], a["m"], a["band"], a["scale"], squared, a["cost"], a["B"], a["C"], a["N"], a["M"], None)

    def backward(fn, **kw):
        a = dict(ok, **kw)
        return fn(a["G"], a["pred"], a["target"], a["n"], a["m"], a["band"], a["scale"], a["rs"], a["dpred"], a["dtarget"],
                  a["B"], a["C"], a["N"], a["M"], None)

    shapes = (dict(B=0), dict(C=0), dict(N=0), dict(M=-1))
    values = (dict(scale=math.nan), dict(scale=math.inf), dict(scale=-math.inf))
    # dense: the errors of aligner_l1_cost_f32 / aligner_l1_cost_backward_f32
    for squared in (0, 1):
        for kw in (dict(pred=None), dict(target=None), dict(cost=None)) + shapes + values + (dict(band=-2),):
            assert forward(lib.aligner_l2_cost_f32, squared, **kw) == _lib.EINVAL, kw
            assert lib.aligner_last_error()
        for kw in (dict(B=65536), dict(C=4097), dict(N=1 << 15, M=1 << 14), dict(N=1, M=1 << 29)):
            assert forward(lib.aligner_l2_cost_f32, squared, **kw) == _lib.EDOM, kw
    for kw in (dict(G=None), dict(pred=None), dict(target=None), dict(dpred=None, dtarget=None)) + shapes + values + (dict(band=-2),):
        assert backward(lib.aligner_l2_cost_backward_f32, **kw) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(B=65536), dict(C=4097), dict(N=1 << 15, M=1 << 14), dict(N=1, M=1 << 29)):
        assert backward(lib.aligner_l2_cost_backward_f32, **kw) == _lib.EDOM, kw
    # band storage: those of aligner_l1_cost_banded_f32 / aligner_l1_cost_banded_backward_f32
    okb = dict(band=3)
    for squared in (0, 1):
        for kw in (dict(pred=None), dict(target=None), dict(cost=None)) + shapes + values + (dict(band=-1),):
            assert forward(lib.aligner_l2_cost_banded_f32, squared, **dict(okb, **kw)) == _lib.EINVAL, kw
            assert lib.aligner_last_error()
        for kw in (dict(band=128), dict(B=65536), dict(C=4097), dict(N=1 << 22, band=127)):
            assert forward(lib.aligner_l2_cost_banded_f32, squared, **dict(okb, **kw)) == _lib.EDOM, kw
    for kw in (dict(G=None), dict(pred=None), dict(target=None), dict(dpred=None, dtarget=None)) + shapes + values + (dict(band=-1),):
        assert backward(lib.aligner_l2_cost_banded_backward_f32, **dict(okb, **kw)) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(band=128), dict(B=65536), dict(C=4097), dict(N=1 << 22, band=127)):
        assert backward(lib.aligner_l2_cost_banded_backward_f32, **dict(okb, **kw)) == _lib.EDOM, kw
    # the same calls, in the same order of checks, as their L1 counterparts: a call that is wrong twice
    both = dict(pred=None, B=65536)
    assert forward(lib.aligner_l2_cost_f32, 1, **both) == _lib.EINVAL
    assert forward(lib.aligner_l2_cost_f32, 1, scale=math.nan, C=4097) == _lib.EINVAL


def test_wrapper_rejections(built_lib):
    import aligner_amd
    p, t = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
    fns = (aligner_amd.l2_cost, aligner_amd.soft_dtw_l2_loss, aligner_amd.l2_cost_banded, aligner_amd.soft_dtw_l2_banded_loss,
           aligner_amd.dtw_path_l2, aligner_amd.mcd_dtw)
    for fn in fns:
        with pytest.raises(ValueError, match=r"B,C,T"):
            fn(p[0], t)
        with pytest.raises(ValueError, match=r"B,C,T"):
            fn(p, t[0])
        with pytest.raises(ValueError, match="disagree"):
            fn(p, torch.zeros(3, 3, 5))
        with pytest.raises(ValueError, match="disagree"):
            fn(p, torch.zeros(2, 4, 5))
        with pytest.raises(ValueError, match="floating"):
            fn(p.long(), t)
        with pytest.raises(ValueError, match="GPU tensor"):
            fn(p, t)
        with pytest.raises(ValueError, match="bandwidth"):
            fn(p, t, bandwidth=-1)
        if fn is not aligner_amd.mcd_dtw:
            with pytest.raises(ValueError, match="scale"):
                fn(p, t, scale=float("nan"))
            with pytest.raises(ValueError, match="scale"):
                fn(p, t, scale=float("inf"))
    for fn in (aligner_amd.l2_cost_banded, aligner_amd.soft_dtw_l2_banded_loss):
        with pytest.raises(ValueError, match="at most 127"):
            fn(p, t, bandwidth=128)
    for fn in (aligner_amd.soft_dtw_l2_loss, aligner_amd.soft_dtw_l2_banded_loss):
        with pytest.raises(ValueError, match="reduction"):
            fn(p, t, reduction="median")
    with pytest.raises(ValueError, match="grad_cost"):
        aligner_amd.l2_cost_backward(torch.zeros(2, 4, 4), p, t)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.l2_cost_backward(torch.zeros(2, 4, 5), p, t)
    with pytest.raises(ValueError, match="grad_band"):
        aligner_amd.l2_cost_banded_backward(torch.zeros(2, 4, 4), p, t)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.l2_cost_banded_backward(torch.zeros(2, 4, 7), p, t)
    with pytest.raises(ValueError, match="warp_penalty"):
        aligner_amd.mcd_dtw(p, t, warp_penalty=-1.0)


def test_the_root_has_no_gradient(built_lib):
    """Refused in the shared helpers before anything else is looked at; the public backward calls have no such kind."""
    from aligner_amd import banddtw, l1cost
    p, t = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
    with pytest.raises(ValueError, match="no gradient"):
        l1cost._cost_backward(l1cost.L2_ROOT, torch.zeros(2, 4, 5), p, t, None, None, None, 1.0, None, (True, True))
    with pytest.raises(ValueError, match="no gradient"):
        banddtw._cost_banded_backward(l1cost.L2_ROOT, torch.zeros(2, 4, 7), p, t, None, None, 1.0, None, (True, True))
