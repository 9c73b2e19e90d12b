"""tests/conv_oracle.py checked on the host (no GPU): the float64 restatement against a literal loop and float64 torch, the
bound's derivation against simulations of the kernels' two error sources, the e(n) table against its simulation, the
tests of the tests (a dropped product, reversed taps, a shifted halo must break the bound), and the case list against
the dispatch's channel rules.  `pytest -rP` shows the figures."""
import functools

import numpy as np
import pytest
import torch

import conv_oracle as C


def _loop(x, w, b, relu):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    y = np.zeros((B, Cout, T))
    for bb in range(B):
        for o in range(Cout):
            for t in range(T):
                s = 0.0 if b is None else float(b[o])
                for i in range(Cin):
                    for k in range(K):
                        tt = t + k - K // 2
                        if 0 <= tt < T:
                            s += w[o, i, k] * x[bb, i, tt]
                y[bb, o, t] = max(s, 0.0) if relu else s
    return y


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_oracle_equals_a_loop_and_float64_torch(K, bias, relu):
    rng = np.random.default_rng(K + 10 * bias + 100 * relu)
    x = rng.standard_normal((2, 3, 7)).astype(np.float32)
    w = rng.standard_normal((4, 3, K)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32) if bias else None
    got = C.conv64(x, w, b, relu)
    assert np.abs(got - _loop(x, w, b, relu)).max() < 1e-13
    t = torch.nn.functional.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                   None if b is None else torch.from_numpy(b).double(), padding=K // 2)
    t = torch.relu(t) if relu else t
    assert np.abs(got - t.numpy()).max() < 1e-13
    A = C.magnitude(np.abs(x.astype(np.float64)), w, b)
    assert np.abs(A - _loop(np.abs(x), np.abs(w), None if b is None else np.abs(b), False)).max() < 1e-13
    # a two-layer stack, each layer with its own flag
    w2 = rng.standard_normal((2, 4, 3)).astype(np.float32)
    got2 = C.encode64(x, [(w, b, relu), (w2, None, not relu)])
    assert np.abs(got2 - _loop(_loop(x, w, b, relu), w2, None, not relu)).max() < 1e-12


def test_relu_of_the_oracle_passes_nan():
    x = np.zeros((1, 2, 5), np.float32)
    x[0, 1, 2] = np.nan
    y = C.conv64(x, np.ones((3, 2, 3), np.float32), None, True)
    assert np.isnan(y[0, :, 1:4]).all() and (y[0, :, [0, 4]] == 0).all()


# ---- every layer of every base case, with the input that reaches it in float64 ----
@functools.lru_cache(maxsize=None)
def _layer_inputs(base, family):
    """[(h_in float64 [B,Cin,T], w, b)] per layer of a base case: the first layer sees the family's draw, the later ones
    the float64 activations."""
    x, layers = C.inputs(base, family)
    hs = C.encode64(x, layers, every=True)
    ins = [x.astype(np.float64)] + hs[:-1]
    return [(h.astype(np.float32), w, b) for h, (w, b, _) in zip(ins, layers)]


@pytest.mark.parametrize("base", C.BASES)
def test_split_products_stay_inside_3_2m16(base):
    """|simulate_split - conv64| <= 3 * 2^-16 A in every cell, every layer, every family: the derivation, checked."""
    worst = 0.0
    for family in C.FAMILIES:
        for h, w, b in _layer_inputs(base, family):
            A = C.magnitude(np.abs(h.astype(np.float64)), w, b)
            err = np.abs(C.simulate_split(h, w, b, w.shape[2]) - C.conv64(h, w, b, False))
            assert (err <= C.SPLIT * A).all(), (base, family)
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.nanmax(np.where(A > 0, err / A, 0.0)) * 2.0 ** 16
            worst = max(worst, r)
            print(f"{base:28s} {family:8s} {w.shape[1]:4d}->{w.shape[0]:4d} k{w.shape[2]}: split error {r:.2f} * 2^-16 A (bound 3)")
    assert worst <= 3.0


@functools.lru_cache(maxsize=None)
def _chain_ratio(base, family):
    """{(Cin, K): max |fp32 chain - exact| / A in units of 2^-24} over the layers of a base case."""
    out = {}
    for h, w, b in _layer_inputs(base, family):
        A = C.magnitude(np.abs(h.astype(np.float64)), w, b)
        err = np.abs(C.simulate_fp32_chain(h, w, b) - C.conv64(h, w, b, False))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = float(np.max(np.where(A > 0, err / A, 0.0))) * 2.0 ** 24
        key = (w.shape[1], w.shape[2])
        out[key] = max(out.get(key, 0.0), r)
    return out


def _simulated_e():
    sim = {}
    for base in C.BASES:
        for family in C.FAMILIES:
            for key, r in _chain_ratio(base, family).items():
                sim[key] = max(sim.get(key, 0.0), r)
    return sim


def test_e_table_covers_the_fp32_chain_and_is_not_padded():
    sim = _simulated_e()
    for key in sorted(sim):
        print(f"Cin {key[0]:4d} k{key[1]} n {key[0] * key[1]:4d}: simulated e(n) {sim[key]:6.2f}, table {C.E_TABLE.get(key)}")
    assert set(sim) == set(C.E_TABLE)
    for key, r in sim.items():
        assert r <= C.E_TABLE[key] <= 2 * r, key


def _wrong_ratio(h, w, b, y_wrong):
    _, E = C.layer_bound(h, w, b)
    err = np.abs(y_wrong - C.conv64(h, w, b, False))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(E > 0, err / E, np.where(err > 0, np.inf, 0.0))))


@pytest.mark.parametrize("drop", ["hl", "lh"])
def test_a_dropped_product_breaks_the_bound(drop):
    """The test of the tests: without one of the two cross products the largest error / E exceeds 2 on every layer of
    every case and every family -- but for "lh" on a layer fed with impulses: 1.0 has no low half, that product is empty."""
    worst = np.inf
    for base in C.BASES:
        for family in C.FAMILIES:
            for n, (h, w, b) in enumerate(_layer_inputs(base, family)):
                if family == "impulse" and drop == "lh" and n == 0:
                    continue
                r = _wrong_ratio(h, w, b, C.simulate_split(h, w, b, w.shape[2], drop=(drop,)))
                print(f"{base:28s} {family:8s} layer {n} without {drop}: error / E = {r:.1f}")
                worst = min(worst, r)
                assert r > 2, (base, family, n, drop)
    print(f"smallest ratio without {drop}: {worst:.2f}")


@pytest.mark.parametrize("family", ["unit", "impulse"])
def test_reversed_taps_and_a_shifted_halo_break_the_bound(family):
    for base in C.BASES:
        h, w, b = _layer_inputs(base, family)[0]
        K = w.shape[2]
        shifted = np.zeros_like(h)
        shifted[:, :, 1:] = h[:, :, :-1]                       # the halo one frame off
        r_shift = _wrong_ratio(h, w, b, C.conv64(shifted, w, b, False))
        assert r_shift > 100, (base, family, r_shift)
        if K > 1:
            r_rev = _wrong_ratio(h, w, b, C.conv64(h, w[:, :, ::-1].copy(), b, False))
            assert r_rev > 100, (base, family, r_rev)
            print(f"{base:28s} {family:8s}: reversed taps {r_rev:.0f} E, shifted halo {r_shift:.0f} E")


@pytest.mark.parametrize("base", ["mixed_k5331", "mixed_wide_ring_fused"])
def test_simulated_stack_stays_inside_the_stack_bound(base):
    """Every layer's input is the previous simulated (split-product) output: the error carried along stays inside E_l."""
    for family in C.FAMILIES:
        x, layers = C.inputs(base, family)
        hs, Es = C.stack_bound(x, layers)
        g = x.astype(np.float64)
        for n, (w, b, relu) in enumerate(layers):
            g = C.simulate_split(g.astype(np.float32), w, b, w.shape[2])
            g = np.maximum(g, 0.0) if relu else g
            r = C.ratio(g, hs[n], Es[n])
            print(f"{base} {family:8s} layer {n}: simulated error / E_l = {r:.3f}")
            assert r <= 1.0, (base, family, n)


def test_case_list_follows_the_dispatch():
    """Each case's form as conv_form / conv_plan / fused_plan's channel rules give it (restated in conv_oracle): a case
    list that drifts away from the dispatch fails here.  Every form and every instantiated fused key has a case."""
    for c in C.CASES.values():
        assert C.expected_form(c) == c.form, (c.name, C.expected_form(c), c.form)
        assert all(k in (1, 3, 5) for k in c.ks) and len(c.chans) == len(c.ks) + 1
    forms = {c.form for c in C.CASES.values()}
    assert forms >= {"none", "wide8", "wide13", "narrow", "ring", "chain", "fused110", "fused111", "fused210", "fused211"}
    assert set(C.IMPULSE_FRAMES) >= {15, 16, 127, 128, 207, 208}


def test_no_stack_reaches_the_fused_key_220():
    """Why no case has the form "fused220": two output tiles a wave in the first fused layer mean more than 128 output
    channels, so the second layer has 129 or more inputs and is narrow only below 128 outputs -- where two tiles for
    each of five or six waves do not fit its image.  Should the dispatch (and its restatement) change, this fails and
    the case list gets a 220 case."""
    assert all(C.fused_key([(64, a, 3), (a, b, 1)]) != 220 for a in range(16, 300) for b in range(16, 300))


def test_impulse_places_differ_per_utterance():
    places = C.impulse_places(2, 80, 333)
    per = [{(c, t) for b, c, t in places if b == u} for u in range(2)]
    assert per[0] and per[1] and not (per[0] & per[1])
    assert {t for _, _, t in places} == set(C.IMPULSE_FRAMES) | {332}
    assert {c for _, c, _ in places} <= {0, 7, 8, 31, 32, 79}
    x = C.draw("impulse", np.random.default_rng(0), (2, 80, 333))
    assert x.sum() == len(places) and set(np.unique(x)) == {0.0, 1.0}
