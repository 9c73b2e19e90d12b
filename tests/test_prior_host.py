"""The beta-binomial prior's oracle (tests/prior_oracle.py) judged on its own, without a GPU: against exact rational
arithmetic where the pmf is rational, against scipy elsewhere, through the identities of the distribution, and then the
float64 emulation of the kernel's two forms against the bound the GPU test uses -- a correct implementation passes it,
the mutated ones do not."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import prior_oracle as orc


def _rel(a, b):
    return abs(a - b) / abs(b)


def _pmf_exact(n, a, b, x):
    """Integer a, b: C(n,x) B(x+a, n-x+b) / B(a,b) in factorials."""
    f = math.factorial
    return Fraction(math.comb(n, x) * f(x + a - 1) * f(n - x + b - 1) * f(a + b - 1), f(n + a + b - 1) * f(a - 1) * f(b - 1))


@pytest.mark.parametrize("n,ty,s", [(1, 1, 1), (1, 7, 1), (5, 1, 2), (6, 9, 1), (9, 6, 1), (12, 30, 2), (30, 11, 3), (40, 40, 1)])
def test_oracle_is_the_exact_rational_pmf_for_integer_scaling(n, ty, s):
    worst = 0
    with mpmath.workdps(orc.DPS):
        for y in range(ty):
            col = orc.column_mp(n, ty, y, float(s))
            for x in range(n + 1):
                q = _pmf_exact(n, s * (y + 1), s * (ty - y), x)
                worst = max(worst, _rel(col[x], mpmath.mpf(q.numerator) / q.denominator))
    print(f"n={n} t_y={ty} s={s}: worst relative difference from the rational pmf {mpmath.nstr(worst, 3)}")
    assert worst <= mpmath.mpf(10) ** -50


@pytest.mark.parametrize("n,ty,s", [(20, 100, 0.5), (17, 33, 1.5), (30, 260, 0.1), (9, 4, 2.25)])
def test_oracle_matches_scipy_for_non_integer_scaling(n, ty, s):
    """scipy.stats.betabinom.pmf is exp(-log(n+1) - betaln(n-x+1, x+1) + betaln(x+a, n-x+b) - betaln(a, b)) in float64.
    Each betaln is three lgamma of magnitude below 500 on these cases; with every libm call good to 4 ulp that is
    4 terms * 3 * 4 ulp * 2^-53 * 500 = 2.7e-12 relative at worst, and the tolerance is that figure (values above 1e-290
    only, clear of float64 underflow).  scipy 1.15 was within 1.1e-14 here.  This pins the formula and the parameter
    convention where the pmf is not rational; the Fraction test pins the digits."""
    from scipy.stats import betabinom
    s32 = orc.f32_scaling(s)
    x = np.arange(n + 1)
    worst = 0.0
    for y in range(ty):
        want = betabinom(n, s32 * (y + 1), s32 * (ty - y)).pmf(x)
        got = np.array([float(v) for v in orc.column_mp(n, ty, y, s32)])
        ok = want > 1e-290
        worst = max(worst, float(np.max(np.abs(got[ok] - want[ok]) / want[ok])))
    print(f"n={n} t_y={ty} s={s}: worst relative difference from scipy {worst:.3e} (tolerance 2.7e-12)")
    assert worst <= 2.7e-12


@pytest.mark.parametrize("n,ty,s", [(1, 300, 1.0), (40, 40, 1.0), (50, 20, 0.5), (500, 4000, 1.0), (30, 260, 0.1), (30, 260, 64.0),
                                    (orc.TX_MAX, 40, 1.0)])
def test_columns_sum_to_one_and_mirror(n, ty, s):
    """Each column plus pmf(n) is 1, and pmf(x; y) = pmf(n - x; t_y - 1 - y), both to 1e-50."""
    s32 = orc.f32_scaling(s)
    with mpmath.workdps(orc.DPS):
        for y in orc.sample_columns(ty)[:: 1 if n < 1000 else 4]:
            col = orc.column_mp(n, ty, y, s32)
            assert abs(mpmath.fsum(col) - 1) <= mpmath.mpf(10) ** -50, (n, ty, y)
            mirror = orc.column_mp(n, ty, ty - 1 - y, s32)
            step = max(1, n // 50)
            assert all(_rel(col[x], mirror[n - x]) <= mpmath.mpf(10) ** -50 for x in range(0, n + 1, step)), (n, ty, y)


def test_one_token_is_b_over_a_plus_b():
    r, = orc.reference("tx_one")
    y = r.ys.astype(np.float64)
    assert r.n == 1 and np.array_equal(r.want[0], (300 - y) / 301)
    assert np.allclose(r.left_out, (y + 1) / 301, rtol=1e-15, atol=0)


def test_scaling_is_the_fp32_value():
    """0.1 is 0.100000001490116 in fp32: the oracle fed the double differs by far more than the GPU bound allows, so the
    convention is part of the specification."""
    assert orc.f32_scaling(0.1) == 0.100000001490116119384765625
    n, ty, y = 30, 260, 200
    with mpmath.workdps(orc.DPS):
        as32 = orc.column_mp(n, ty, y, orc.f32_scaling(0.1))
        as64 = orc.column_mp(n, ty, y, 0.1)
    rel = max(float(_rel(p, q)) for p, q in zip(as32[:n], as64[:n]))
    print(f"oracle at float32(0.1) against the double 0.1: {rel:.3e} relative ({rel / 2.0 ** -24:.2f} fp32 ulp)")
    assert rel > 2.0 ** -26


def test_lengths_are_clamped_and_columns_listed():
    c = orc.case("ragged")
    assert [orc.lengths(c, b) for b in range(c.B)] == [(12, 300), (0, 200), (0, 100), (12, 280), (7, 0), (9, 300), (5, 257)]
    assert [len(orc.columns_of(c, b)) for b in range(c.B)] == [300, 0, 0, 280, 0, 300, 257]
    ys = orc.sample_columns(4000)
    assert {0, 1, 3998, 3999, 255, 256, 3839, 3840}.issubset(ys) and ys == sorted(set(ys))
    for T in (1, 2, 3, 255, 256, 257):
        assert all(0 <= y < T for y in orc.sample_columns(T))


def test_cases_sit_either_side_of_the_form_switch():
    """The form switch is crossed for s = 1 and s = 2, the recurrence runs with an integer scaling, and the top-index
    cases fill the last table shape."""
    forms = {name: orc.form_of(orc.case(name)) for name in orc.CASE_NAMES}
    for s in (1, 2):
        assert forms[f"switch_s{s}_table"] == "table" and forms[f"switch_s{s}_rec"] == "rec"
        t, r = orc.case(f"switch_s{s}_table"), orc.case(f"switch_s{s}_rec")
        assert (t.Tx, t.Ty + 1, t.t_x, t.t_y) == (r.Tx, r.Ty, r.t_x, r.t_y)
        assert t.Tx + s * (t.Ty + 1) + 2 == orc.TABLE_DOUBLES
    for s in (1, 2, 3):
        c = orc.case(f"top_index_s{s}")
        assert forms[c.name] == "table" and c.t_x == (c.Tx,) and c.t_y == (c.Ty,)
        assert not orc.takes_table(c.Tx, c.Ty + 1, c.scaling)
    assert [forms[f"scaling_{s:g}"] for s in orc.SCALINGS] == ["table", "table", "table", "rec", "rec", "rec", "rec"]
    assert forms["largest_text"] == "rec" and forms["underflow"] == "table"


def test_ulp32():
    f = np.float32
    for w in (1.0, 1.5, 0.75, 3e-5, 2.0 ** -126, 1e-30, 0.999999):
        assert orc.ulp32(w) == float(np.nextafter(f(w), f(np.inf))) - float(f(w)), w
    assert orc.ulp32(2.0 ** -127) == orc.ulp32(0.0) == orc.ulp32(1e-300) == 2.0 ** -149


def _emulated(name, form=None, mutation=None):
    c = orc.case(name)
    return np.stack([orc.emulate(c.Tx, c.Ty, c.t_x[b], c.t_y[b], c.scaling, form, mutation) for b in range(c.B)])


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_emulated_kernel_forms_stay_inside_the_gpu_bound(name):
    """A float64 evaluation in the kernel's own form (host libm) is inside the bound the GPU test asserts: a correct
    implementation passes.  Integer scalings are run through both forms, whichever the host would choose."""
    c = orc.case(name)
    for r in orc.reference(name):
        assert r.S.size == 0 or r.S.min() >= 0.5                         # (the exp's share of K assumes it)
    forms = ["table", "rec"] if orc.takes_table(c.Tx, c.Ty, c.scaling) else ["rec"]
    for form in forms:
        rv, rl, _ = orc.check(name, _emulated(name, form), "emulation", form)
        assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("name,mutation", [("top_index_s1", "top_index"), ("scaling_2", "top_index"), ("frames257", "top_index"),
                                           ("switch_s1_rec", "walk_b"), ("scaling_0.5", "walk_b"), ("largest_text", "walk_b"),
                                           ("scaling_1", "lgamma32"), ("scaling_64", "lgamma32"), ("underflow", "lgamma32")])
def test_bound_catches_the_mutated_forms(name, mutation):
    """The wrong kernels -- the table read one entry too high, the second walk stepping with n - x for n - x - 1, lgamma
    in fp32 -- leave the bound on the cases named."""
    rv, _, _ = orc.check(name, _emulated(name, mutation=mutation), f"mutation {mutation}")
    assert rv > 1.0
