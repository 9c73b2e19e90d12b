"""The boundary search's named inputs, bounds and fp32 restatement (tests/mobo_cases.py) checked on the host: the recursion in
np.float32 stays inside LA, GAMMA and MAP on every case (printed as observed / bound), every sabotaged variant of it leaves
them on a case this file names, the cap of the bounds holds, the oracle does not see a per-row offset, and the utterances that
are meant to have no segmentation have none."""
import numpy as np
import pytest

import mobo_cases as mc
from oracle import mobo_oracle as M


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_fp32_restatement_is_inside_the_bounds(name):
    wrong = mc.compare(name, mc.batch32(name), "fp32")
    assert not wrong, wrong


# the case that catches each wrong kernel (first entry), and others that do as well
CAUGHT_BY = {
    "window_shifted": ("slack_one", "window_one", "constant"),
    "lo_without_reach": ("tight_full", "slack_one"),
    "normaliser_of_previous_row": ("offsets_h4", "two_valued", "tight_ones"),
    "row_max_reference": ("cliff_block_edge", "offsets_h4_helper"),
}


def test_every_sabotage_has_a_catching_case():
    assert set(CAUGHT_BY) == set(mc.SABOTAGES)
    assert CAUGHT_BY["row_max_reference"][0] in ["cliff_block_edge"] + mc.OFFSET_CASES


@pytest.mark.parametrize("sabotage,name", [(s, n) for s in mc.SABOTAGES for n in CAUGHT_BY[s]])
def test_sabotaged_restatement_is_caught(sabotage, name):
    wrong = mc.compare(name, mc.batch32(name, sabotage), "fp32 " + sabotage)
    print("\n".join(wrong))
    assert wrong, f"{sabotage} passes on {name}"


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_cap_of_the_bounds(name):
    """LA (at its largest cell) and MAP below the tolerance fitted to log_alpha and map_score on every case; GAMMA below the
    one fitted to gamma on the cases of GAMMA_DERIVED_UNDER_CAP, and compare() asserts the smaller of the two everywhere."""
    for b, ref in enumerate(mc.reference(name)):
        if ref is None:
            continue
        fin = np.isfinite(ref.want["log_alpha"])
        la = ref.bd.LA[-1] + 2 * mc.U * np.abs(ref.want["log_alpha"][fin]).max()
        mp = ref.bd.MAP + (2 * mc.U * abs(ref.want["map_score"]) if ref.has_answer else 0.0)
        ga, cap, cap_ga = ref.bd.GAMMA.max(), mc.fitted_la_tolerance(ref.I), mc.fitted_gamma_tolerance(ref.I)
        print(f"{name}[{b}] I={ref.I}: LA {la:.2e}, MAP {mp:.2e}, cap {cap:.2e};  GAMMA {ga:.2e}, cap {cap_ga:.2e}, ratio {ga / cap_ga:.1f}")
        assert la < cap and mp < cap
        if name in mc.GAMMA_DERIVED_UNDER_CAP:
            assert ga < cap_ga


def test_compare_never_allows_gamma_more_than_the_fitted_tolerance():
    """A gamma off by 1.01 times the fitted tolerance in one cell is refused on every case, whatever GAMMA is there."""
    for name in mc.CASE_NAMES:
        got = {k: np.array(v) for k, v in mc.batch32(name).items()}
        refs = mc.reference(name)
        b = next(i for i, r in enumerate(refs) if r is not None)
        got["gamma"][b, 0, 0] += np.float32(1.01 * mc.fitted_gamma_tolerance(refs[b].I) + 1e-6)
        assert any("gamma outside" in w for w in mc.compare(name, got, "fp32, gamma moved"))


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_rows_of_the_bounds_are_the_oracle_s(name):
    """mobo_cases.rows64 (the magnitudes the bounds are made of) against the oracle's log_alpha and map_score."""
    c = mc.case(name)
    for ref in mc.reference(name):
        if ref is None:
            continue
        la, de, _ = mc.rows64(ref.e, min(c.D, c.Ty))
        fin = np.isfinite(ref.want["log_alpha"])
        assert np.array_equal(np.isfinite(la[1:, 1:]), fin)
        assert np.abs(la[1:, 1:][fin] - ref.want["log_alpha"][fin]).max() < 1e-10
        if ref.has_answer:
            assert abs(de[-1, -1] - ref.want["map_score"]) < 1e-10
        else:
            assert de[-1, -1] == -np.inf


@pytest.mark.parametrize("name", mc.OFFSET_CASES)
def test_oracle_is_shift_invariant_per_row(name):
    """A per-row offset changes no probability: the oracle on the offset case against its offset-free twin."""
    c = mc.case(name)
    assert np.array_equal(mc.energies(name) - mc.row_offsets(c.Tx)[None, :, None], mc.energies(name, True))     # exact in fp32
    worst = 0.0
    for ref, twin in zip(mc.reference(name), mc.reference(name, True)):
        fin = np.isfinite(twin.want["log_alpha"])
        assert np.array_equal(np.isfinite(ref.want["log_alpha"]), fin)
        d = max(np.abs(ref.want["log_alpha"][fin] - twin.want["log_alpha"][fin]).max(),
                np.abs(ref.want["gamma"] - twin.want["gamma"]).max(), abs(ref.want["map_score"] - twin.want["map_score"]))
        worst = max(worst, d)
        assert np.array_equal(ref.want["boundaries"], twin.want["boundaries"])
    print(f"{name}: offset case against its twin, largest difference {worst:.2e}")
    assert worst < 1e-11


def test_utterances_meant_to_have_no_segmentation_have_none():
    refs = mc.reference("masked_runs")
    assert refs[0].has_answer and refs[1].has_answer and not refs[2].has_answer
    assert [r is not None for r in mc.reference("degenerate_lengths")] == [True, False, False, False, True, False]
    c = mc.case("degenerate_lengths")
    for b in (1, 2, 3, 5):
        I, J, _ = mc.clamped_lengths(c, b)
        if I >= 1 and J >= 1:
            with pytest.raises(ValueError):
                M.boundary_search_fast(np.zeros((I, J)), c.D)
    for name in mc.CASE_NAMES:
        if name not in ("masked_runs", "degenerate_lengths"):
            assert all(r is not None and r.has_answer for r in mc.reference(name)), name


def test_tight_and_constant_cases_score_what_they_must():
    """One finite entry per row: probability 1.  All-zero energies [12, 40], D = 8: every step is uniform over its band."""
    for name in ("tight_ones", "tight_full", "window_one"):
        for ref in mc.reference(name):
            assert np.isfinite(ref.want["log_alpha"]).sum(axis=1).max() == 1 and abs(ref.want["map_score"]) < 1e-12
    assert abs(mc.reference("constant")[0].want["map_score"] - (-8.3178)) < 5e-5


def test_sixteen_bit_case_is_exact_in_both_formats():
    e = mc.energies("masked_sixteen_bit")
    fin = np.isfinite(e)
    assert (~fin).any() and np.array_equal(e[fin].astype(np.float16).astype(np.float32), e[fin])
    bits = e[fin].view(np.uint32)
    assert not (bits & 0xFFFF).any()                            # bf16: the low 16 bits of the fp32 pattern are zero
