"""Host-side checks of Soft-DTW (no GPU): the float64 oracle against autograd over a plain double loop and against central
differences; the np.float32 restatement of the kernels' arithmetic inside the derived bounds on every input the GPU
tests use, with the caps on those bounds asserted; sabotaged restatements well outside them; the two backward forms
measured against float64; the C ABI's argument checks and the wrappers' rejections."""
import math

import numpy as np
import pytest
import torch

import softdtw_oracle as orc


def _loop_autograd(cost, gamma, p, band):
    """value and d value / d cost of one block by torch float64 autograd over the definition, cell by cell; a cell that
    does not exist is simply left out of its successors' softmin."""
    D = torch.tensor(np.where(np.isfinite(cost), cost, 0.0), dtype=torch.float64, requires_grad=True)
    n, m = cost.shape
    R = {(-1, -1): torch.zeros((), dtype=torch.float64)}
    for i in range(n):
        for j in range(m):
            if not np.isfinite(cost[i, j]) or (band is not None and abs(i - j) > band):
                continue
            ops = [R[k] + pen for k, pen in (((i - 1, j - 1), 0.0), ((i - 1, j), p), ((i, j - 1), p)) if k in R]
            if ops:
                R[(i, j)] = D[i, j] - gamma * torch.logsumexp(-torch.stack(ops) / gamma, dim=0)
    if (n - 1, m - 1) not in R:
        return math.inf, np.zeros((n, m))
    R[(n - 1, m - 1)].backward()
    return R[(n - 1, m - 1)].item(), D.grad.numpy()


@pytest.mark.parametrize("n,m,gamma,p,band,hole", [(7, 9, 1.0, 0.0, None, False), (9, 7, 0.3, 0.25, None, False),
                                                   (8, 11, 1.0, 0.5, 4, False), (12, 5, 0.1, 0.0, None, True),
                                                   (6, 6, 2.0, 1.0, 0, False), (1, 5, 1.0, 0.3, None, False),
                                                   (5, 9, 1.0, 0.0, 3, False)])
def test_oracle_equals_autograd_of_the_definition(n, m, gamma, p, band, hole):
    cost = orc.uniform_cost(1, n, m, seed=n * 100 + m).astype(np.float64)
    if hole:
        cost[0, 3:6, 1:4] = np.inf
    want_v, want_E = _loop_autograd(cost[0], gamma, p, band)
    value, E, _ = orc.soft_dtw64(cost, None, None, gamma, p, band)
    if not math.isfinite(want_v):
        assert value[0] == np.inf and not E.any()
        return
    assert abs(value[0] - want_v) <= 1e-12 * max(1.0, abs(want_v))
    assert np.max(np.abs(E[0] - want_E)) <= 1e-12
    print(f"[{n},{m}] gamma {gamma} p {p} band {band}: value diff {abs(value[0] - want_v):.2e}, E diff {np.max(np.abs(E[0] - want_E)):.2e}")


def test_oracle_lengths_select_the_block():
    cost = orc.uniform_cost(2, 9, 11, seed=5).astype(np.float64)
    value, E, _ = orc.soft_dtw64(cost, (9, 4), (11, 6), 0.7, 0.2, None)
    v1, E1, _ = orc.soft_dtw64(cost[1:, :4, :6], None, None, 0.7, 0.2, None)
    assert value[1] == v1[0] and np.array_equal(E[1, :4, :6], E1[0])
    assert not E[1, 4:].any() and not E[1, :, 6:].any()


def test_oracle_equals_central_differences():
    cost = orc.uniform_cost(1, 5, 7, seed=57).astype(np.float64)
    gamma, p, band = 0.5, 0.2, 3
    _, E, _ = orc.soft_dtw64(cost, None, None, gamma, p, band)
    h = 1e-5
    worst = 0.0
    for i in range(5):
        for j in range(7):
            up, dn = cost.copy(), cost.copy()
            up[0, i, j] += h
            dn[0, i, j] -= h
            fd = (orc.soft_dtw64(up, None, None, gamma, p, band)[0][0] - orc.soft_dtw64(dn, None, None, gamma, p, band)[0][0]) / (2 * h)
            worst = max(worst, abs(fd - E[0, i, j]))
    print(f"central differences: largest |fd - E| = {worst:.2e}")
    assert worst <= 1e-8          # the difference quotient's own error: h^2 |f'''| / 6 ~ 1e-10 / gamma^2, rounding 1e-16 / h


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_bounds_stay_below_their_caps(name):
    """A loose bound cannot hide a failure: GRAD <= 0.05 and VALUE <= 8 (n+m) 2^-24 (max|R| + gamma) on every input."""
    c, cost, value, E, stats = orc.reference(name)
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


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_float32_restatement_is_inside_the_bounds(name):
    c, cost, value, E, stats = orc.reference(name)
    v32, E32 = orc.soft_dtw32(cost, c.n, c.m, c.gamma, c.p, c.band)
    rv, rg = orc.check(name, v32, E32, "float32 restatement")
    assert rv <= 1.0 and rg <= 1.0
    for b, st in enumerate(stats):
        assert not E32[b, st.n:].any() and not E32[b, :, st.m:].any()


SABOTAGES = [("no_penalty", lambda c: c.p > 0), ("band_plus_one", lambda c: c.band is not None),
             ("gamma_doubled", lambda c: True), ("swap_weights", lambda c: True)]


@pytest.mark.parametrize("sabotage,applies", SABOTAGES, ids=[s for s, _ in SABOTAGES])
def test_sabotaged_restatements_are_far_outside_the_bounds(sabotage, applies, capsys):
    """A dropped penalty, a band one cell too wide, a doubled gamma, the diagonal and the upward weight swapped: each is
    at least 4 bounds away on every input it can show on (value or E, whichever it moves)."""
    seen = 0
    for name in orc.CASE_NAMES:
        c, cost, value, E, stats = orc.reference(name)
        if not applies(c):
            continue
        v32, E32 = orc.soft_dtw32(cost, c.n, c.m, c.gamma, c.p, c.band, sabotage=sabotage)
        worst = 0.0
        for b, st in enumerate(stats):
            if not st.feasible or st.n + st.m < 8 or min(st.n, st.m) < 2:
                continue                                   # (one row or column: a single path, nothing to get wrong)
            rv = abs(float(v32[b]) - value[b]) / orc.value_bound(st, value[b], c.gamma)
            rg = float(np.max(np.abs(E32[b].astype(np.float64) - E[b]))) / orc.grad_bound(st, c.gamma)
            worst = max(worst, rv, rg)
        if worst == 0.0:
            continue
        seen += 1
        print(f"{sabotage} on {name}: {worst:.1f} bounds away")
        assert worst >= 4.0, (sabotage, name, worst)
    assert seen >= 2


def test_pushed_backward_beats_the_textbook_recursion_in_float32():
    """Both backward forms in np.float32 against float64 on costs 50 mean|x - y| over 8 channels: the measurement behind
    the kernels' choice (the textbook form subtracts large running costs)."""
    for (n, m, gamma) in [(96, 130, 0.1), (200, 300, 1.0)]:
        D = 50.0 * orc.l1_cost(1, n, m, seed=n + m)[0].astype(np.float64)
        v64, Et64, Ep64 = orc.both_backward_forms(D, gamma, np.float64)
        v32, Et32, Ep32 = orc.both_backward_forms(D, gamma, np.float32)
        forms = np.max(np.abs(Et64 - Ep64))
        et, ep = np.max(np.abs(Et32 - Ep64)), np.max(np.abs(Ep32 - Ep64))
        print(f"[{n},{m}] gamma {gamma}: value {v64:.3f}; float64 forms differ by {forms:.1e}; float32 max error of E: "
              f"textbook {et:.2e}, pushed {ep:.2e}; value error {abs(float(v32) - v64):.2e}")
        assert forms <= 1e-9
        assert ep < et


def test_abi_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = torch.zeros(64, dtype=torch.float32)
    q = buf.data_ptr()
    ok = dict(cost=q, n=None, m=None, gamma=1.0, p=0.0, band=-1, value=q, grad=q, ws=q, wsb=256, B=1, N=4, M=4)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.aligner_soft_dtw_f32(a["cost"], a["n"], a["m"], a["gamma"], a["p"], a["band"], a["value"], a["grad"], a["ws"],
                                        a["wsb"], a["B"], a["N"], a["M"], None)

    for kw in (dict(cost=None), dict(value=None), dict(ws=None), dict(B=0), dict(N=0), dict(M=-1), dict(gamma=0.0),
               dict(gamma=-1.0), dict(gamma=math.inf), dict(gamma=math.nan), dict(p=-0.5), dict(p=math.inf), dict(p=math.nan),
               dict(band=-2)):
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.aligner_last_error()
    for kw in (dict(N=1025), dict(B=65536), dict(N=1024, M=1 << 19), dict(N=1, M=1 << 29)):
        assert call(**kw) == _lib.EDOM, kw
    assert call(wsb=8) == _lib.ENOSPC
    assert call(B=65, wsb=256) == _lib.ENOSPC
    assert lib.aligner_soft_dtw_workspace_bytes(65, 4, 4, 1) >= 65 * 4
    assert lib.aligner_soft_dtw_workspace_bytes(2, 1024, 24, 0) > 0
    for shape in ((0, 4, 4), (1, 1025, 4), (65536, 4, 4), (1, 1024, 1 << 19)):
        assert lib.aligner_soft_dtw_workspace_bytes(*shape, 1) == 0


def test_wrapper_rejections(built_lib):
    import aligner_amd
    c = torch.zeros(2, 3, 4)
    for bad in (dict(gamma=0.0), dict(gamma=float("nan")), dict(warp_penalty=-1.0), dict(warp_penalty=float("inf")),
                dict(bandwidth=-1)):
        with pytest.raises(ValueError):
            aligner_amd.soft_dtw(c, **bad)
    with pytest.raises(ValueError, match="B,N,M"):
        aligner_amd.soft_dtw(c[0])
    with pytest.raises(ValueError, match="floating"):
        aligner_amd.soft_dtw(c.long())
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.soft_dtw(c)
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.soft_dtw_loss(c, reduction="median")
    if built_lib.aligner_device_count() == 0:
        return
    with pytest.raises(ValueError, match="one entry per utterance"):
        aligner_amd.soft_dtw(c.cuda(), n=torch.tensor([1, 2, 3]))
