"""Host-side checks of the band-storage Soft-DTW (no GPU): the index map of dense_to_band / band_to_dense, the caps on
the oracle's bounds on every input the GPU tests use, the np.float32 restatement of the cell arithmetic inside those
bounds (and a band one cell too wide far outside them), the C ABI's argument checks and the wrappers' rejections."""
import math

import numpy as np
import pytest
import torch

import banddtw_oracle as bo
import softdtw_oracle as orc


@pytest.mark.parametrize("N,M,w", [(7, 9, 2), (9, 7, 3), (5, 5, 0), (5, 3, 6), (4, 12, 3), (1, 1, 1)])
def test_band_round_trip_and_index_map(N, M, w):
    import aligner_amd
    x = torch.arange(2 * N * M, dtype=torch.float32).view(2, N, M) + 1.0
    xb = aligner_amd.dense_to_band(x, w, fill=-7.0)
    assert xb.shape == (2, N, 2 * w + 1)
    for i in range(N):
        for d in range(2 * w + 1):
            j = i + d - w
            want = x[:, i, j] if 0 <= j < M else torch.full((2,), -7.0)
            assert torch.equal(xb[:, i, d], want), (i, d)
    back = aligner_amd.band_to_dense(xb, M, fill=-3.0)
    mask = torch.from_numpy(bo.band_mask(N, M, w))
    assert torch.equal(back[:, mask], x[:, mask]) and bool((back[:, ~mask] == -3.0).all())
    # the numpy helpers of the tests are the same map
    assert np.array_equal(bo.to_band(x.numpy(), w, -7.0), xb.numpy())
    assert np.array_equal(bo.to_dense(xb.numpy(), M, -3.0), back.numpy())
    with pytest.raises(ValueError, match="odd"):
        aligner_amd.band_to_dense(torch.zeros(1, 3, 4), 3)


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_bounds_stay_below_their_caps(name):
    """The assertion of test_softdtw_host.py::test_bounds_stay_below_their_caps on the band cases."""
    c, _, _, _, value, E, stats = bo.reference(name)
    assert c.gamma in (1.0, 0.1)
    for b, st in enumerate(stats):
        if c.gamma == 0.1:
            assert st.n + st.m <= 230
        if not st.feasible:
            continue
        gb, vb, cap = orc.grad_bound(st, c.gamma), orc.value_bound(st, value[b], c.gamma), orc.value_cap(st, c.gamma)
        print(f"{name}[{b}]: GRAD {gb:.4f} (cap 0.05), VALUE {vb:.3e} (cap {cap:.3e}), A {st.A:.2f}, max|R| {st.maxR:.2f}")
        assert gb <= 0.05
        assert st.A <= 5.0 * st.maxR + 2.0 * c.p + 1e-9
        assert vb <= cap


def test_cases_are_what_they_claim():
    """The ragged case's last two utterances are infeasible, both of the forbidden case's inside this band and the second
    of forbidden_round's; past1024 is past the dense kernel's rows; every table fits band storage (M <= N + w)."""
    feas = {name: [st.feasible for st in bo.reference(name)[6]] for name in ("ragged", "forbidden", "forbidden_round", "past1024")}
    assert feas["ragged"] == [True, True, True, True, False, False]
    assert feas["forbidden"] == [False, False]
    assert feas["forbidden_round"] == [True, False]
    assert feas["past1024"] == [True, True]
    assert "past1024" not in bo.DENSE_NAMES and len(bo.DENSE_NAMES) == len(bo.CASE_NAMES) - 1
    for c in bo.CASES:
        assert c.M <= c.N + c.w and 0 <= c.w <= 127


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_float32_restatement_is_inside_the_bounds(name):
    c, _, dense, _, _, _, stats = bo.reference(name)
    v32, E32 = orc.soft_dtw32(dense, c.n, c.m, c.gamma, c.p, c.w)
    rv, rg = bo.check(name, v32, E32, "float32 restatement")
    assert rv <= 1.0 and rg <= 1.0
    assert not E32[:, ~bo.band_mask(c.N, c.M, c.w)].any()


@pytest.mark.parametrize("name", ["w1", "steps63", "ragged"])
def test_a_band_one_cell_too_wide_is_far_outside_the_bounds(name):
    c, raw, _, _, value, E, stats = bo.reference(name)
    v32, E32 = orc.soft_dtw32(raw, c.n, c.m, c.gamma, c.p, c.w, sabotage="band_plus_one")
    worst = 0.0
    for b, st in enumerate(stats):
        if not st.feasible or min(st.n, st.m) < 2:
            continue
        rv = abs(float(v32[b]) - value[b]) / orc.value_bound(st, value[b], c.gamma)
        rg = float(np.max(np.abs(E32[b].astype(np.float64) - E[b]))) / orc.grad_bound(st, c.gamma)
        worst = max(worst, rv, rg)
    print(f"band_plus_one on {name}: {worst:.1f} bounds away")
    assert worst >= 4.0


def test_abi_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = torch.zeros(64, dtype=torch.float32)
    q = buf.data_ptr()
    ok = dict(cost=q, n=None, m=None, gamma=1.0, p=0.0, band=1, value=q, grad=q, ws=q, wsb=256, B=1, N=4)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.aligner_soft_dtw_banded_f32(a["cost"], a["n"], a["m"], a["gamma"], a["p"], a["band"], a["value"], a["grad"],
                                               a["ws"], a["wsb"], a["B"], a["N"], None)

    for kw in (dict(cost=None), dict(value=None), dict(ws=None), dict(B=0), dict(N=0), dict(gamma=0.0), dict(gamma=-1.0),
               dict(gamma=math.inf), dict(gamma=math.nan), dict(p=-0.5), dict(p=math.inf), dict(p=math.nan), dict(band=-1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(band=128), dict(B=65536), dict(N=(1 << 29) // 3 + 1), dict(band=127, N=(1 << 29) // 255 + 1)):
        assert call(**kw) == _lib.EDOM, kw
    assert call(band=128) == _lib.EDOM and b"dense" in lib.aligner_last_error()
    assert call(wsb=8) == _lib.ENOSPC
    assert call(B=65, wsb=256) == _lib.ENOSPC
    assert lib.aligner_soft_dtw_banded_workspace_bytes(65, 4, 1, 1) >= 65 * 4
    assert lib.aligner_soft_dtw_banded_workspace_bytes(2, 100000, 60, 0) > 0            # no limit on N alone
    for shape in ((0, 4, 1), (1, 4, 128), (65536, 4, 1), (1, (1 << 29) // 3 + 1, 1), (1, 4, -1)):
        assert lib.aligner_soft_dtw_banded_workspace_bytes(*shape, 1) == 0

    okc = dict(pred=q, target=q, band=1, scale=1.0, out=q, B=1, C=2, N=4, M=4)

    def cost(**kw):
        a = dict(okc, **kw)
        return lib.aligner_l1_cost_banded_f32(a["pred"], a["target"], None, None, a["band"], a["scale"], a["out"],
                                              a["B"], a["C"], a["N"], a["M"], None)

    def back(**kw):
        a = dict(dict(okc, G=q, dp=q, dt=q), **kw)
        return lib.aligner_l1_cost_banded_backward_f32(a["G"], a["pred"], a["target"], None, None, a["band"], a["scale"], None,
                                                       a["dp"], a["dt"], a["B"], a["C"], a["N"], a["M"], None)

    for kw in (dict(pred=None), dict(target=None), dict(B=0), dict(C=0), dict(N=0), dict(M=0), dict(scale=math.inf),
               dict(scale=math.nan), dict(band=-1)):
        assert cost(**kw) == _lib.EINVAL, kw
        assert back(**kw) == _lib.EINVAL, kw
    assert cost(out=None) == _lib.EINVAL and back(G=None) == _lib.EINVAL and back(dp=None, dt=None) == _lib.EINVAL
    for kw in (dict(band=128), dict(B=65536), dict(C=4097), dict(N=(1 << 29) // 3 + 1)):
        assert cost(**kw) == _lib.EDOM, kw
        assert back(**kw) == _lib.EDOM, kw


def test_wrapper_rejections(built_lib):
    import aligner_amd
    cb = torch.zeros(2, 3, 5)
    for bad in (dict(gamma=0.0), dict(gamma=float("nan")), dict(warp_penalty=-1.0), dict(warp_penalty=float("inf"))):
        with pytest.raises(ValueError):
            aligner_amd.soft_dtw_banded(cb, **bad)
    with pytest.raises(ValueError, match="odd"):
        aligner_amd.soft_dtw_banded(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="B,N,W"):
        aligner_amd.soft_dtw_banded(cb[0])
    with pytest.raises(ValueError, match="floating"):
        aligner_amd.soft_dtw_banded(cb.long())
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.soft_dtw_banded(cb)
    with pytest.raises(ValueError, match="soft_dtw\\(\\)"):
        aligner_amd.soft_dtw_banded(torch.zeros(1, 3, 257))
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.soft_dtw_banded_loss(cb, reduction="median")
    pred, target = torch.zeros(2, 4, 6), torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.l1_cost_banded(pred, target, bandwidth=2)
    with pytest.raises(ValueError, match="soft_dtw\\(\\)"):
        aligner_amd.l1_cost_banded(pred, target, bandwidth=128)
    with pytest.raises(ValueError, match="soft_dtw\\(\\)"):
        aligner_amd.soft_dtw_l1_banded_loss(pred, target, bandwidth=128)
    with pytest.raises(ValueError, match="at least 0"):
        aligner_amd.l1_cost_banded(pred, target, bandwidth=-1)
    with pytest.raises(ValueError, match="disagree"):
        aligner_amd.l1_cost_banded(pred, target[:, :3], bandwidth=2)
    with pytest.raises(ValueError, match="odd"):
        aligner_amd.l1_cost_banded_backward(torch.zeros(2, 6, 4), pred, target)
    with pytest.raises(ValueError, match="B,N,W"):
        aligner_amd.l1_cost_banded_backward(torch.zeros(2, 5, 5), pred, target)
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.soft_dtw_l1_banded_loss(pred, target, reduction="median")
