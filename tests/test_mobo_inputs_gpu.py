"""boundary_search() and its gradient on the GPU against the float64 oracle inside the derived bounds of tests/mobo_cases.py, on
the named inputs that reach each mechanism of csrc/mobo.hip and csrc/mobo_bwd.inc: tight, clamped and degenerate lengths,
short utterances in a launch planned for long ones, a last segment shorter than the window, per-row offsets of 128 nats
(rows that take the exact sums between rows that take the fast ones, in every form of the chain), a step of 160 nats, masked
frames, 16-bit energies, ties.  Then: the three chain kernels agree bit for bit on the hard inputs, one utterance's trouble
stays its own (bad lengths, masked runs, NaN), and the gradient on the same inputs.  Every comparison prints observed / bound."""
import functools

import numpy as np
import pytest
import torch

import mobo_cases as mc
from oracle import mobo_oracle as M
from test_mobo_backward import _check_grad

pytestmark = pytest.mark.gpu

OUTPUTS = ("boundaries", "durations", "map_score", "log_alpha", "gamma")
FORWARD = [(c.name, dt) for c in mc.CASES for dt in c.dtypes]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lengths(c, tx=None, ty=None):
    return torch.tensor(c.tx if tx is None else tx, dtype=torch.int32), torch.tensor(c.ty if ty is None else ty, dtype=torch.int32)


def _search(c, e, dtype="float32", tx=None, ty=None, **kw):
    """One call on the GPU: (BoundarySearch of GPU tensors, status bits the call left)."""
    import aligner_amd
    from aligner_amd import mobo
    dev = torch.device("cuda:0")
    ed = torch.from_numpy(np.array(e)).to(getattr(torch, dtype))
    fin = np.isfinite(e)
    assert np.array_equal(ed.float().numpy()[fin], e[fin])              # the case is exact in the type it is run in
    mobo.read_status(dev)                                               # (clears what earlier tests left)
    txd, tyd = _lengths(c, tx, ty)
    r = aligner_amd.boundary_search(ed.to(dev), txd, tyd, c.D, **kw)
    torch.cuda.synchronize()
    return r, mobo.read_status(dev)


def _numpy(r):
    return {k: getattr(r, k).cpu().numpy() for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def _run(name, dtype="float32"):
    """One GPU run per case and type, shared by the tests: (outputs as numpy arrays, status)."""
    r, status = _search(mc.case(name), mc.energies(name), dtype, want_log_alpha=True, want_gamma=True)
    return _numpy(r), status


def _expected_status(name):
    return 0 if all(r is not None and r.has_answer for r in mc.reference(name)) else mc.ST_BAD_LENGTHS


@pytest.mark.parametrize("name,dtype", FORWARD, ids=[n if d == "float32" else f"{n}-{d}" for n, d in FORWARD])
def test_forward_inside_the_bounds(dev, name, dtype):
    """log_alpha is finite exactly where the oracle's is (-inf outside the lengths); log_alpha, gamma and map_score are inside
    LA, GAMMA and MAP; the MAP sequence is a segmentation, optimal within the margin; gamma is exactly 0 outside the lengths;
    an utterance without an answer has all-zero boundaries and durations, score -inf and ALIGNER_ST_BAD_LENGTHS."""
    got, status = _run(name, dtype)
    for k in OUTPUTS:
        assert not np.isnan(got[k]).any(), k
    wrong = mc.compare(name, got, "GPU " + dtype)
    assert not wrong, wrong
    assert status == _expected_status(name)


CHAIN_CASES = mc.OFFSET_CASES + ["cliff_block_edge", "masked_runs", "masked_sixteen_bit"]


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_three_chains_agree_bit_for_bit(dev, name):
    """The max-product chain alone equals the full kernel (`mobo_full_chain` forces that one), and the sum-product chain
    alone equals it too, where rows take the exact sums between rows that take the fast ones."""
    from aligner_amd import _lib
    lib = _lib.load()
    c, e = mc.case(name), mc.energies(name)
    dtype = c.dtypes[0]
    full, st = _search(c, e, dtype, want_log_alpha=True, want_gamma=True)
    only_map, st_map = _search(c, e, dtype)
    assert lib.aligner_debug_set_option(b"mobo_full_chain", 1) == 0
    try:
        forced, st_forced = _search(c, e, dtype)
    finally:
        lib.aligner_debug_set_option(b"mobo_full_chain", 0)
    only_sum, st_sum = _search(c, e, dtype, want_gamma=True, want_map=False)
    for k in ("boundaries", "durations", "map_score"):
        assert torch.equal(getattr(only_map, k), getattr(forced, k)), k
        assert torch.equal(getattr(only_map, k), getattr(full, k)), k
        assert getattr(only_sum, k) is None
    assert torch.equal(only_sum.log_alpha, full.log_alpha) and torch.equal(only_sum.gamma, full.gamma)
    assert not torch.isnan(full.log_alpha).any() and not torch.isnan(full.gamma).any()
    want = _expected_status(name)
    assert st == want and st_map == want and st_forced == want
    assert st_sum == 0                 # without the MAP outputs masked frames that leave no sequence are not reported


def _same_bits(a, b, utterances):
    for k in OUTPUTS:
        x, y = getattr(a, k), getattr(b, k)
        assert not torch.isnan(x).any() and not torch.isnan(y).any(), k
        for u in utterances:
            assert torch.equal(x[u], y[u]), (k, u)


def test_bad_lengths_stay_their_own(dev):
    """degenerate_lengths twice at the same B, Tx, Ty, D (the same plan): once as it is, once with the four utterances without
    an answer given valid lengths.  Utterances 0 and 4 are bit-identical in every output."""
    c, e = mc.case("degenerate_lengths"), mc.energies("degenerate_lengths")
    bad, st_bad = _search(c, e, want_log_alpha=True, want_gamma=True)
    good, st_good = _search(c, e, tx=(12, 12, 10, 12, 99, 6), ty=(40, 40, 40, 33, 999, 40), want_log_alpha=True, want_gamma=True)
    assert st_bad == mc.ST_BAD_LENGTHS and st_good == 0
    assert int(good.durations[1].sum()) == 40 and int(good.durations[5].sum()) == 40
    _same_bits(bad, good, (0, 4))


def test_masked_run_stays_its_own(dev):
    """masked_runs twice: once as it is, once with utterance 2 unmasked.  Utterances 0 and 1 are bit-identical."""
    c, e = mc.case("masked_runs"), mc.energies("masked_runs")
    open_ = e.copy()
    open_[2] = np.where(np.isfinite(e[2]), e[2], 0.0)
    bad, st_bad = _search(c, e, want_log_alpha=True, want_gamma=True)
    good, st_good = _search(c, open_, want_log_alpha=True, want_gamma=True)
    assert st_bad == mc.ST_BAD_LENGTHS and st_good == 0
    assert int(good.durations[2].sum()) == 90 and int(bad.durations[2].sum()) == 0
    _same_bits(bad, good, (0, 1))


def _handed_on_position(c, b, cus):
    """A boundary position of utterance b that segment 0 hands to segment 1 on a device of `cus` CUs, or None where the
    utterance is not cut (mobo_plan's S and mb_cut's n: the last position of segment 0 is among its last D)."""
    P, D = min(c.ty[b], c.Ty) + 1, min(c.D, c.Ty)
    S = max(1, min(cus // c.B, (c.Ty + 1) // D, (c.Ty + 1 + 63) // 64))
    Sb = max(1, min(S, P // D))
    return None if Sb < 2 else -(-P // Sb) - 1


def test_nan_energy_is_a_masked_frame(dev):
    """A NaN energy fails every "is it live" comparison of the kernels, as -inf does: the utterance's results equal those with
    -inf at the same cells, and the other utterances do not see it.  offsets_h4_helper, utterance 0: one cell at a position
    that segment 0 hands to segment 1 (worked out for this device's CU count: position 60 of segments of 61 on 256 CUs), one
    at a position that is not handed on there."""
    name = "offsets_h4_helper"
    c, e = mc.case(name), mc.energies(name)
    pos = _handed_on_position(c, 0, torch.cuda.get_device_properties(dev).multi_processor_count)
    pos = 60 if pos is None else pos                     # (a device that does not cut the utterance has no halo to reach)
    row = min(c.tx[0] - 1, max(10, pos // c.D + 1))      # a row in which that position is reachable
    lo, hi = M.band(c.tx[0], c.ty[0], c.D, row)
    assert lo <= pos <= min(hi, (row + 1) * c.D)
    cells = ((0, row, pos - 1), (0, 20, 150))
    print(f"NaN at position {pos} of row {row} (handed on) and at position 151 of row 20")
    with_nan, with_inf = e.copy(), e.copy()
    for cell in cells:
        with_nan[cell], with_inf[cell] = np.nan, -np.inf
    base, _ = _search(c, e, want_log_alpha=True, want_gamma=True)
    a, st_a = _search(c, with_nan, want_log_alpha=True, want_gamma=True)
    b, st_b = _search(c, with_inf, want_log_alpha=True, want_gamma=True)
    assert st_a == 0 and st_b == 0
    _same_bits(a, b, (0, 1, 2))
    _same_bits(a, base, (1, 2))
    for (u, i, y) in cells:
        assert torch.isneginf(a.log_alpha[u, i, y]) and not torch.isneginf(base.log_alpha[u, i, y])
    want = M.boundary_search_fast(with_inf[0].astype(np.float64), c.D)
    assert np.array_equal(a.boundaries[0].cpu().numpy(), want["boundaries"])


# ----------------------------------------------------------------------------------------------------------------------
# the gradient on the same inputs

GRAD_CASES = ["tight_ones", "slack_one", "short_in_long", "window_clamped", "offsets_h4_helper", "offsets_h2", "offsets_h1_helper",
              "offsets_several", "cliff_block_edge", "masked_runs", "constant"]


@functools.lru_cache(maxsize=None)
def _checked(name, twin=False, general=False):
    """_check_grad of tests/test_mobo_backward.py (unchanged: its cotangents, its tolerance, its assertions) on a named case,
    with what it computed on the way recorded: (its return value, the HIP gradient [B,Tx,Ty] float64, the float64 adjoint per
    utterance it compared, the status left).  Utterances whose lengths allow no segmentation are left out (the oracle refuses
    them); one whose masked frames leave none is compared like the others (gradient 0 on both sides)."""
    import aligner_amd
    from aligner_amd import _lib, mobo
    dev = torch.device("cuda:0")
    c, e = mc.case(name), np.array(mc.energies(name, twin))
    only = [b for b, r in enumerate(mc.reference(name)) if r is not None]
    rec = {"want": []}
    hip, oracle = aligner_amd.boundary_search_backward, M.boundary_search_backward

    def rec_hip(*a, **k):
        rec["got"] = hip(*a, **k)
        return rec["got"]

    def rec_oracle(*a, **k):
        rec["want"].append(oracle(*a, **k))
        return rec["want"][-1]

    mobo.read_status(dev)                                               # (clears what earlier tests left)
    aligner_amd.boundary_search_backward, M.boundary_search_backward = rec_hip, rec_oracle
    assert _lib.load().aligner_debug_set_option(b"mobo_bwd_general", 1 if general else 0) == 0
    try:
        worst = _check_grad(dev, e, np.array(c.tx, np.int32), np.array(c.ty, np.int32), c.D, only=only)
    finally:
        aligner_amd.boundary_search_backward, M.boundary_search_backward = hip, oracle
        _lib.load().aligner_debug_set_option(b"mobo_bwd_general", 0)
    status = mobo.read_status(dev)
    assert len(rec["want"]) == len(only)
    return worst, rec["got"].cpu().numpy().astype(np.float64), dict(zip(only, rec["want"])), status


def _tolerance(want, I, rtol=3e-3):
    """_check_grad's tolerance of one utterance (test_gradient_matches_oracle checks that it still is)"""
    return rtol * (1 + I / 100) * np.abs(want).max() + 2e-5


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_matches_oracle(dev, name):
    """_check_grad, its tolerance unchanged, on the named inputs.  Also prints what nobody has measured: the largest error of
    a token row relative to that row's own largest entry (not asserted)."""
    worst, got, wants, status = _checked(name)
    assert status == _expected_status(name)
    per_row, ratio = 0.0, 0.0
    for b, want in wants.items():
        I, J = want.shape
        ratio = max(ratio, np.abs(got[b, :I, :J] - want).max() / _tolerance(want, I))
        top = np.abs(want).max(axis=1)
        err = np.abs(got[b, :I, :J] - want).max(axis=1)
        rows = top >= 1e-3 * top.max()                  # (a row with one live cell has the gradient 0: no entry to relate to)
        if rows.any() and top.max() > 0:
            per_row = max(per_row, float((err[rows] / top[rows]).max()))
    assert abs(ratio - worst) <= 1e-9 * max(worst, 1e-30)       # _tolerance above is _check_grad's
    print(f"GPU gradient {name}: err / tolerance = {worst:.4f};  largest row error / the row's largest entry = {per_row:.2e} "
          f"(rows whose largest entry is at least 1e-3 of the utterance's)")


def test_gradient_general_form_matches_oracle(dev):
    """offsets_h4_helper through the gradient chain's general form (`mobo_bwd_general`)."""
    worst, _, _, status = _checked("offsets_h4_helper", general=True)
    assert status == 0
    print(f"GPU gradient offsets_h4_helper, general form: err / tolerance = {worst:.4f}")


@pytest.mark.parametrize("name", GRAD_CASES + ["degenerate_lengths"])
def test_gradient_properties_without_oracle(dev, name):
    """Every live token row's gradient sums to zero (its energies only count up to a shift) within 2e-3 of the utterance's
    largest entry, as tests/test_mobo_backward.py asks at full size.  Only an utterance whose true gradient is identically 0
    (one live cell in every row) has no entry to scale by: what is left of its gradient is the rounding of Z - flow, and it
    gets the 2e-5 that _check_grad allows that rounding.  The gradient is exactly 0 at masked cells, outside the lengths and
    for an utterance without a segmentation (by its lengths or by its masked frames)."""
    e = mc.energies(name)
    _, got, wants, status = _checked(name)
    assert status == _expected_status(name)
    assert np.all(np.isfinite(got))
    for b, ref in enumerate(mc.reference(name)):
        if ref is None or not ref.has_answer:
            assert not got[b].any(), b
            continue
        I, J = ref.I, ref.J
        assert not got[b, I:].any() and not got[b, :, J:].any(), b
        assert not got[b, :I, :J][~np.isfinite(e[b, :I, :J])].any(), b
        scale = np.abs(got[b]).max()
        sums = np.abs(got[b, :I, :J].sum(axis=1)).max()
        zero = np.abs(wants[b]).max() < 1e-9
        tol = 2e-3 * scale + (2e-5 if zero else 0.0)
        print(f"GPU gradient {name}[{b}]: largest row sum {sums:.2e} / (2e-3 x largest entry {scale:.2e}"
              f"{' + 2e-5: the true gradient is 0' if zero else ''}) = {sums / tol:.4f}")
        assert sums < tol, b


@pytest.mark.parametrize("name", [n for n in GRAD_CASES if n in mc.OFFSET_CASES])
def test_gradient_does_not_see_a_row_offset(dev, name):
    """The gradient of an offset case agrees with its offset-free twin within twice _check_grad's tolerance (both through
    _check_grad, so with the same cotangents)."""
    _, got, wants, _ = _checked(name)
    _, twin, _, status = _checked(name, True)
    assert status == 0
    for b, want in wants.items():
        I, J = want.shape
        err, tol = np.abs(got[b, :I, :J] - twin[b, :I, :J]).max(), 2 * _tolerance(want, I)
        print(f"GPU gradient {name}[{b}]: offset case against its twin {err:.2e} / (2 x tolerance {tol / 2:.2e}) = {err / tol:.4f}")
        assert err < tol, b
