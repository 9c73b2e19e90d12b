"""Soft-attention forward, the parts that need no GPU: the float64 oracle (tests/softattn_oracle64.py) against a cell-by-cell
loop and against the fp32 oracle, and the three figures the GPU tests' bound is made of --

  * max |simulate_split - oracle| / Scol   <= split_bound(C): 2^-17 from 80 channels on (the three bf16 split products,
    exact accumulation),
  * max |simulate_fp32_chain - oracle| / Scol <= CHAIN_RATIO[C] (fp32 products and norms, channel by channel),
  * the fp32 log-sum-exp floor F_LSE (four times what fp32 torch.log_softmax loses on exact logits)

-- and the 1e-4 consequences include/aligner_amd.h states for the split-product kernels at the host's sharp rule."""
import numpy as np
import pytest
import torch

import softattn_oracle64 as O

def _logit_ratio(sim_logit, k, q, T, sim):
    """max over cells of |simulated logit - exact logit| / Scol (all rows valid)."""
    logit, S = O.logits(k, q, T, sim)
    return float((np.abs(sim_logit - logit) / S.max(1, keepdims=True)).max())


@pytest.mark.parametrize("sim", ["l2", "dot"])
def test_oracle_equals_a_triple_loop(sim):
    rng = np.random.default_rng(3)
    for (B, C, Tx, Ty, fam) in [(3, 3, 5, 4, "unit"), (3, 1, 1, 1, "scale3"), (4, 5, 7, 2, "offset3")]:
        k, q = O.draw(fam, rng, B, C, Tx, Ty)
        t_x = np.array([Tx, 1, 0, Tx + 3][:B], np.int32)
        prior = rng.random((B, Tx, Ty)).astype(np.float32)
        prior[0, 0, 0] = 0.0
        for pr in (None, prior):
            logp, soft, S, Scol, valid = O.soft_attention(k, q, t_x, pr, 0.11, sim)
            wl, ws, wS = O.triple_loop(k, q, t_x, pr, 0.11, sim)
            assert np.array_equal(np.isfinite(logp), np.isfinite(wl)) and np.array_equal(np.isfinite(logp), valid)
            assert np.abs(logp[valid] - wl[valid]).max() < 1e-12
            assert np.abs(soft - ws).max() < 1e-13
            assert np.abs(S - wS).max() <= 1e-13 * wS.max()
            assert np.abs(Scol - np.where(valid, wS, 0.0).max(1)).max() <= 1e-13 * wS.max()


@pytest.mark.parametrize("sim,T", [("l2", 0.0005), ("dot", 0.11)])
def test_oracle_equals_the_fp32_oracle_on_unit(sim, T):
    from oracle import softattn_oracle as S32
    rng = np.random.default_rng(4)
    B, C, Tx, Ty = 3, 80, 70, 50
    k, q = O.draw("unit", rng, B, C, Tx, Ty)
    t_x = np.array([Tx, 33, 1], np.int32)
    prior = rng.random((B, Tx, Ty)).astype(np.float32)
    for pr in (None, prior):
        logp, soft, _, Scol, valid = O.soft_attention(k, q, t_x, pr, T, sim)
        wl, ws = S32.soft_attention(torch.from_numpy(k), torch.from_numpy(q), t_x=torch.from_numpy(t_x),
                                    prior=None if pr is None else torch.from_numpy(pr), temperature=T, sim=sim)
        wl, ws = wl.numpy(), ws.numpy()
        assert np.array_equal(np.isfinite(wl), valid)
        # fp32 rounding of the sums (C terms of magnitude Scol in all) and of the log-sum-exp over Tx terms
        tol = 4 * (C + Tx) * 2.0 ** -24 * (1.0 + Scol.max() + np.abs(logp[valid]).max())
        err = np.abs(wl[valid] - logp[valid]).max()
        print(f"{sim}: fp32 oracle against float64, max |err| = {err:.3e} (tolerance {tol:.3e})")
        assert err < tol
        assert np.abs(ws - soft).max() < tol


@pytest.mark.parametrize("sim", ["l2", "dot"])
def test_one_valid_row_and_none(sim):
    rng = np.random.default_rng(5)
    k, q = O.draw("scale3", rng, 2, 16, 9, 11)
    prior = rng.random((2, 9, 11)).astype(np.float32)
    prior[0, 0, 3] = 0.0
    one = np.array([1, 1], np.int32)
    logp, soft, _, _, valid = O.soft_attention(k, q, one, None, 0.05, sim)
    assert (logp[:, 0] == 0.0).all() and np.isneginf(logp[:, 1:]).all() and valid[:, 0].all() and not valid[:, 1:].any()
    assert (soft[:, 0] == 1.0).all() and (soft[:, 1:] == 0.0).all()
    logp, soft, _, _, _ = O.soft_attention(k, q, one, prior, 0.05, sim)
    assert np.array_equal(logp[:, 0], np.log(prior[:, 0].astype(np.float64) + 1e-8)) and (soft[:, 0] == 1.0).all()
    for t in (np.array([0, -4], np.int32),):
        for pr in (None, prior):
            logp, soft, _, Scol, valid = O.soft_attention(k, q, t, pr, 0.05, sim)
            assert np.isneginf(logp).all() and not soft.any() and not np.signbit(soft).any() and not valid.any()
            assert not Scol.any()


@pytest.mark.parametrize("sim,T", [("l2", 0.0005), ("l2", 0.05), ("dot", 0.11)])
def test_planted_columns_peak_on_their_row(sim, T):
    rng = np.random.default_rng(6)
    B, C, Tx, Ty = (2, 256, 129, 96) if T == 0.05 else (2, 80, 40, 100)
    k, q = O.draw("planted", rng, B, C, Tx, Ty)
    logp, soft, _, _, _ = O.soft_attention(k, q, None, None, T, sim)
    want = np.broadcast_to(O.planted_rows(Tx, Ty), (B, Ty))
    assert np.array_equal(logp.argmax(1), want) and np.array_equal(soft.argmax(1), want)
    if T == 0.05:                                       # hundreds of nats between the rows: exact zeros in an fp32 soft
        assert (soft < 2.0 ** -150).any() and np.isfinite(logp).all() and logp.min() < -200


def _shape_inputs(C, Tx, Ty, fam):
    """Inputs of one family at one of the GPU tests' shapes (two utterances)."""
    return O.draw(fam, np.random.default_rng(1000 * C + Tx + len(fam)), 2, C, Tx, Ty)


def test_split_products_stay_below_the_bound():
    """Source of the GPU tests' c for the split-product forms (twice this bound: 2^-16 from 80 channels on), at the GPU
    tests' own shapes, families and temperatures.  2^-17 does not hold below 80 channels, where a column's error is that of
    a few products: O.split_bound() gives the worst case of one product there."""
    for C, Tx, Ty in O.GPU_SHAPES:
        worst = {}
        for fam in O.FAMILIES:
            k, q = _shape_inputs(C, Tx, Ty, fam)
            for sim in ("l2", "dot"):
                for T in O.GPU_TEMPERATURES[sim]:
                    r = _logit_ratio(O.simulate_split(k, q, T, sim), k, q, T, sim)
                    worst[sim] = max(worst.get(sim, 0.0), r)
                    assert r <= O.split_bound(C), (C, Tx, Ty, fam, sim, T, r / O.split_bound(C))
        print(f"simulate_split [{C},{Tx},{Ty}]: max |err| / Scol = {worst['l2'] * 2.0 ** 16:.3f} (L2), {worst['dot'] * 2.0 ** 16:.3f} (dot) "
              f"* 2^-16 (bound {O.split_bound(C) * 2.0 ** 16:.1f})")


def test_split_bound_notices_a_missing_product():
    """The bound test is tight enough to fail when one of the three products is left out."""
    k, q = _shape_inputs(80, 200, 132, "scale3")
    for drop in ("lh", "hl"):
        for sim, T in (("l2", 0.0005), ("dot", 0.11)):
            r = _logit_ratio(O.simulate_split(k, q, T, sim, drop=(drop,)), k, q, T, sim)
            print(f"simulate_split without {drop} ({sim}): max |err| / Scol = {r * 2.0 ** 16:.1f} * 2^-16")
            assert r > 4 * O.split_bound(1), (drop, sim, r / O.split_bound(1))       # (past the widest bound in use)


def test_fp32_chain_stays_below_the_recorded_ratio():
    """Source of the GPU tests' c for the exact-product form: four times CHAIN_RATIO[C]."""
    for C in O.GPU_CHANNELS:
        worst = 0.0
        for _, Tx, Ty in [s for s in O.GPU_SHAPES if s[0] == C]:
            for fam in O.FAMILIES:
                k, q = _shape_inputs(C, Tx, Ty, fam)
                for sim in ("l2", "dot"):
                    T = O.GPU_TEMPERATURES[sim][0]      # (the ratio does not depend on the temperature: both sides carry it)
                    worst = max(worst, _logit_ratio(O.simulate_fp32_chain(k, q, T, sim), k, q, T, sim))
        print(f"simulate_fp32_chain C = {C:3d}: max |err| / Scol = {worst * 2.0 ** 24:.3f} * 2^-24 "
              f"(recorded {O.CHAIN_RATIO[C] * 2.0 ** 24:.3f})")
        assert worst <= O.CHAIN_RATIO[C], (C, worst / O.CHAIN_RATIO[C])
        assert O.CHAIN_RATIO[C] <= 2 * worst, f"C={C}: the recorded ratio is more than twice the measured one"


def test_lse_floor():
    """F_LSE: what the log-sum-exp costs in fp32 whatever the logits' magnitude.  Exact logits rounded to fp32 through fp32
    torch.log_softmax against the oracle; four times the maximum, since the hardware's exp2 / log2 are 1-2 ulp where libm is
    nearly correctly rounded."""
    worst = 0.0
    for Tx in (1, 33, 224, 500):
        for sim, T in (("l2", 0.0005), ("dot", 0.11)):
            rng = np.random.default_rng(Tx)
            k, q = O.draw("unit", rng, 2, 80, Tx, 64)
            logit, _ = O.logits(k, q, T, sim)
            want, _, _ = O.finish(logit)
            got = torch.log_softmax(torch.from_numpy(logit.astype(np.float32)), dim=1).numpy().astype(np.float64)
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"fp32 log_softmax on exact logits: max |err| = {worst:.3e}; F = 4 x = {4 * worst:.3e} (recorded {O.F_LSE:.3e})")
    assert 4 * worst <= O.F_LSE < 2e-5
    assert O.F_LSE <= 8 * worst, "the recorded floor is more than twice the measured one"


# include/aligner_amd.h on the split-product kernels at the host's sharp rule (the sharpest temperature they are given):
# L2 holds 1e-4 on encodings of a few units per channel, dot only on encodings of about one unit per channel
# (O.PROMISED_1E_4 restates that wording; the GPU tests assert the old 1e-4 on the same set)
@pytest.mark.parametrize("fam", ["unit", "scale3", "offset3"])
@pytest.mark.parametrize("sim,T", [("l2", 0.002), ("dot", 0.2)])
def test_header_1e_4_against_the_split_simulation(sim, T, fam):
    """Promised cells stay below 1e-4 with the log-sum floor added; a cell the header does not promise is one where the
    split products alone pass 1e-4 (T = 0.2 multiplies the product error 50 times more than the L2 rule's 2T = 0.004)."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for C in (80, 256):
        k, q = O.draw(fam, rng, 2, C, 200, 130)
        want, _, _ = O.finish(O.logits(k, q, T, sim)[0])
        got, _, _ = O.finish(O.simulate_split(k, q, T, sim))
        worst = max(worst, float(np.abs(got - want).max()))
    promised = (sim, fam) in O.PROMISED_1E_4
    print(f"{sim} T = {T} {fam}: split products alone move logp by {worst:.3e} ({'promised' if promised else 'not promised'})")
    if promised:
        assert worst + O.F_LSE < 1e-4
    else:
        assert worst > 1e-4, "the header could promise 1e-4 here"
