"""Host-side checks of l1_cost / l1_cost_backward / soft_dtw_l1_loss (no GPU): the float64 oracle (tests/l1cost_oracle.py)
equals torch.cdist(p=1) and its autograd gradient on every case restricted to its existing cells, ties included; an fp32
numpy evaluation sits inside the oracle's bounds; the C ABI validates its arguments before it looks for a device; the
wrappers reject what they document."""
import math

import numpy as np
import pytest
import torch

import l1cost_oracle as orc


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_oracle_equals_cdist_and_its_autograd_gradient(name):
    c, pred, target, G, cost, dp, dt, _, _ = orc.reference(name)
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
        D = torch.cdist(x, y, p=1) * c.scale
        assert np.allclose(D.detach().numpy()[okb], cost[b, :n[b], :m[b]][okb], rtol=1e-13, atol=0)
        w = torch.tensor(np.where(okb, G[b, :n[b], :m[b]].astype(np.float64), 0.0))
        (D * w).sum().mul(g[b]).backward()
        scale = max(np.abs(dp[b]).max(), np.abs(dt[b]).max(), 1e-300)
        worst = max(worst, np.abs(x.grad.numpy().T - dp[b, :, :n[b]]).max() / scale, np.abs(y.grad.numpy().T - dt[b, :, :m[b]]).max() / scale)
        assert not dp[b, :, n[b]:].any() and not dt[b, :, m[b]:].any()
    print(f"{name}: oracle against cdist autograd, largest difference / largest gradient {worst:.2e}")
    assert worst <= 1e-12


def test_the_tie_case_has_ties():
    share = orc.tie_share("ties")
    print(f"ties: {share:.3f} of (i,j,c) are exact ties")
    assert share >= 0.10                       # 9 levels in [-1, 1], weights 1/16, 7 x 1/8, 1/16: 0.117 expected
    assert orc.tie_share("edges") == 0.0


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_an_fp32_evaluation_is_inside_the_bounds(name):
    c, pred, target, G, *_ = orc.reference(name)
    rc = orc.check_cost(name, orc.cost32(pred, target, c.n, c.m, c.band, c.scale), "fp32 numpy")
    dp, dt = orc.grads32(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    rp, rt = orc.check_grads(name, dp, dt, "fp32 numpy")
    assert rc <= 1.0 and rp <= 1.0 and rt <= 1.0


def test_the_bounds_catch_a_wrong_sign_and_a_leaking_fill():
    c, pred, target, G, *_ = orc.reference("ties")
    dp, dt = orc.grads32(G, pred, target, c.n, c.m, c.band, c.scale, c.row_scale)
    # sign(0) = 1 in place of 0: the ties count
    s = np.where(pred[:, :, :, None] >= target[:, :, None, :], np.float32(1), np.float32(-1))
    wrong = (np.where(np.isnan(G), np.float32(0), G)[:, None] * s).sum(3, dtype=np.float32)
    rp, _ = orc.check_grads("ties", wrong, dt, "sign(0) = 1")
    assert rp > 1.0
    c, pred, target, *_ = orc.reference("band30")
    cost = orc.cost32(pred, target, c.n, c.m, c.band, c.scale)
    cost[0, 0, 40] = 3.0                       # a cell outside the band that is not +inf
    with pytest.raises(AssertionError):
        orc.check_cost("band30", cost, "leaking fill")


def test_abi_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = torch.zeros(64, dtype=torch.float32)
    q = buf.data_ptr()
    ok = dict(G=q, pred=q, target=q, n=None, m=None, band=-1, scale=1.0, rs=None, cost=q, dpred=q, dtarget=q, B=1, C=2, N=4, M=4)

    def forward(**kw):
        a = dict(ok, **kw)
        return lib.aligner_l1_cost_f32(a["pred"], a["target"], a["n"], a["m"], a["band"], a["scale"], a["cost"],
                                       a["B"], a["C"], a["N"], a["M"], None)

    def backward(**kw):
        a = dict(ok, **kw)
        return lib.aligner_l1_cost_backward_f32(a["G"], a["pred"], a["target"], a["n"], a["m"], a["band"], a["scale"], a["rs"],
                                                a["dpred"], a["dtarget"], a["B"], a["C"], a["N"], a["M"], None)

    shapes = (dict(B=0), dict(C=0), dict(N=0), dict(M=-1))
    values = (dict(scale=math.nan), dict(scale=math.inf), dict(scale=-math.inf), dict(band=-2))
    for kw in (dict(pred=None), dict(target=None), dict(cost=None)) + shapes + values:
        assert forward(**kw) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(G=None), dict(pred=None), dict(target=None), dict(dpred=None, dtarget=None)) + shapes + values:
        assert backward(**kw) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(B=65536), dict(C=4097), dict(N=1 << 15, M=1 << 14), dict(N=1, M=1 << 29)):
        assert forward(**kw) == _lib.EDOM, kw
        assert backward(**kw) == _lib.EDOM, kw


def test_wrapper_rejections(built_lib):
    import aligner_amd
    p, t = torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)
    for fn in (aligner_amd.l1_cost, aligner_amd.soft_dtw_l1_loss):
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
        with pytest.raises(ValueError, match="scale"):
            fn(p, t, scale=float("nan"))
        with pytest.raises(ValueError, match="bandwidth"):
            fn(p, t, bandwidth=-1)
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.soft_dtw_l1_loss(p, t, reduction="median")
    with pytest.raises(ValueError, match="grad_cost"):
        aligner_amd.l1_cost_backward(torch.zeros(2, 4, 4), p, t)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.l1_cost_backward(torch.zeros(2, 4, 5), p, t)
