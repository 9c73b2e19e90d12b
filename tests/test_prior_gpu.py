"""beta_binomial_prior() on the GPU against the 80-digit oracle (tests/prior_oracle.py) inside its derived bound, on the
smallest shapes at which each mechanism of prior_kernel (csrc/prior.hip) can break (prior_oracle.CASES): either side of
the switch between the log-factorial table and the lgamma recurrence, the table's top index, frame blocks of 256, every
degenerate and out-of-range length, the largest text, deep underflow, integer / fractional / inexact scalings.  Then the
properties that need no oracle, on every cell: exact zeros in the padding, column sums, the mirror symmetry, the same
bits on a second run and outside the batch; the domain's edge; and stores that stay inside their buffers.  Every
comparison prints observed / bound.

K of the bound is 16 ulp per device lgamma / log / exp call, counted over the kernel's text (prior_oracle's docstring);
nothing in it is fitted to a run."""
import functools

import numpy as np
import pytest
import torch

import prior_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _i32(t, dev):
    return torch.tensor(t, dtype=torch.int32, device=dev)


def _prior(c, dev, keep=None):
    import aligner_amd
    keep = range(c.B) if keep is None else keep
    out = aligner_amd.beta_binomial_prior(_i32([c.t_x[b] for b in keep], dev), _i32([c.t_y[b] for b in keep], dev), c.Tx, c.Ty,
                                          c.scaling)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(name):
    """One GPU run per case, shared by the tests: prior [B, Tx, Ty] as a numpy array."""
    got = _prior(orc.case(name), torch.device("cuda:0"))
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_values_inside_the_bound_and_what_the_consumer_sees(dev, name):
    """|got - want| <= 0.5 ulp32(want) + K 2^-53 S want and |log(got + 1e-8) - log(want + 1e-8)| <= 2^-22 on every cell the
    oracle evaluated; finite and non-negative; below 2^-126 an exact +0 passes too, and which the GPU did is printed."""
    rv, rl, verdict = orc.check(name, _run(name), "GPU")
    print(f"GPU {name} ({orc.form_of(orc.case(name))} form): worst value err / bound {rv:.4f}, worst log err / 2^-22 {rl:.4f}, "
          f"fp32 subnormals: {verdict}")
    assert rv <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("name", orc.CASE_NAMES)
def test_zeros_column_sums_and_symmetry_on_every_cell(dev, name):
    """Needs no oracle.  +0.0 bits at x >= t_x and at y >= t_y (all of an utterance whose clamped t_x < 1); every column's
    sum over x < t_x in (0, 1 + 2^-20]; prior[x, y] against prior[n - x, t_y - 1 - y] for 1 <= x <= n - 1 within 4 ulp32 --
    the two cells use different table entries and different steps of the walks."""
    c = orc.case(name)
    got = _run(name)
    assert np.isfinite(got).all()
    bits = got.view(np.uint32)
    for b in range(c.B):
        n, ty = orc.lengths(c, b)
        assert not bits[b, n:].any() and not bits[b, :, ty:].any(), (name, b)
        if n < 1 or ty < 1:
            assert not bits[b].any(), (name, b)
            continue
        blk = got[b, :n, :ty].astype(np.float64)
        assert (blk >= 0).all()
        sums = blk.sum(0)
        msg = f"{name}[{b}] n={n} t_y={ty}: column sums in [{sums.min():.3e}, 1 + {sums.max() - 1:.3e}] (limit 1 + {2.0 ** -20:.3e})"
        if n >= 2:
            lo, hi = blk[1:], blk[1:][::-1, ::-1]                          # x = 1..n-1 against n - x, t_y - 1 - y
            diff = np.abs(lo - hi) / orc.ulp32(np.maximum(lo, hi))
            i = np.unravel_index(np.argmax(diff), diff.shape)
            msg += f"; mirror cells differ by at most {diff.max():.2f} ulp32 (limit 4) at x={i[0] + 1} y={i[1]}"
            assert diff.max() <= 4
        print(msg)
        assert sums.min() > 0 and sums.max() <= 1 + 2.0 ** -20


def test_two_runs_and_an_utterance_alone_give_the_same_bits(dev):
    c = orc.case("ragged")
    got = _run("ragged")
    assert np.array_equal(_prior(c, dev).view(np.uint32), got.view(np.uint32))
    for b in range(c.B):
        alone = _prior(c, dev, keep=[b])
        assert np.array_equal(alone[0].view(np.uint32), got[b].view(np.uint32)), b


@pytest.mark.parametrize("s", [1, 2])
def test_both_forms_agree_across_the_switch(dev, s):
    """The last container that takes the table and the first that takes the recurrence carry the same lengths: within
    2 ulp32 of each other on every cell of the common block (each is within half an ulp of the oracle where sampled:
    test_values_inside_the_bound)."""
    tab, rec = _run(f"switch_s{s}_table"), _run(f"switch_s{s}_rec")
    c = orc.case(f"switch_s{s}_table")
    assert orc.form_of(c) == "table" and orc.form_of(orc.case(f"switch_s{s}_rec")) == "rec"
    a, b = tab.astype(np.float64), rec[:, :, :c.Ty].astype(np.float64)
    diff = np.abs(a - b) / orc.ulp32(np.maximum(a, b))
    i = np.unravel_index(np.argmax(diff), diff.shape)
    print(f"s={s}: table [{c.Tx},{c.Ty}] against recurrence [{c.Tx},{c.Ty + 1}]: at most {diff.max():.2f} ulp32 apart (limit 2) at "
          f"x={i[1]} y={i[2]}; {int((diff > 0).sum())} of {diff.size} cells differ")
    assert diff.max() <= 2
    assert not rec[:, :, c.Ty:].view(np.uint32).any()


def _fenced(count, dev, band=1024):
    """`count` floats of NaN between two bands of NaN."""
    buf = torch.full((band + count + band,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[band:band + count], band


def _abi_prior(dev, t_x, t_y, Tx, Ty, scaling):
    from aligner_amd import _lib
    B = len(t_x)
    buf, out, band = _fenced(B * Tx * Ty, dev)
    tx, ty = _i32(t_x, dev), _i32(t_y, dev)
    rc = _lib.load().aligner_beta_binomial_prior_f32(tx.data_ptr(), ty.data_ptr(), out.data_ptr(), B, Tx, Ty, scaling,
                                                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    intact = bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + B * Tx * Ty:]).all())
    return rc, out.view(B, Tx, Ty), intact


@pytest.mark.parametrize("name", ["frames257", "switch_s1_table", "switch_s1_rec", "switch_s2_table", "switch_s2_rec", "top_index_s1",
                                  "largest_text", "ragged"])
def test_stores_stay_inside_their_buffers(dev, name):
    """The output carved out of a NaN-filled allocation, the C ABI called on the interior pointer: the canaries are
    intact, no NaN is left inside (every element is written) and the result is the wrapper's."""
    c = orc.case(name)
    rc, out, intact = _abi_prior(dev, c.t_x, c.t_y, c.Tx, c.Ty, c.scaling)
    assert rc == 0 and intact
    assert not bool(torch.isnan(out).any())
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _run(name).view(np.uint32))


def test_domain_edge_and_bad_arguments(dev):
    """Tx = 7679 runs (largest_text: test_values_inside_the_bound); Tx = 7680 is EDOM and launches nothing; a scaling that
    is 0, negative or NaN is EINVAL; B = 0 is an empty tensor."""
    import aligner_amd
    from aligner_amd import _lib
    assert orc.case("largest_text").Tx == orc.TX_MAX == 7679
    for Tx, scaling, code in [(7680, 1.0, _lib.EDOM), (7680, 0.5, _lib.EDOM), (5, 0.0, _lib.EINVAL), (5, -1.0, _lib.EINVAL),
                              (5, float("nan"), _lib.EINVAL)]:
        rc, out, intact = _abi_prior(dev, [3, 5], [2, 1], Tx, 2, scaling)
        assert rc == code and intact and bool(torch.isnan(out).all()), (Tx, scaling, rc)
        with pytest.raises(_lib.AlignerError) as e:
            aligner_amd.beta_binomial_prior(_i32([3, 5], dev), _i32([2, 1], dev), Tx, 2, scaling)
        assert e.value.code == code
    rc, out, intact = _abi_prior(dev, [3, 5], [2, 1], 7679, 2, 1.0)
    assert rc == 0 and intact and not bool(torch.isnan(out).any())
    empty = aligner_amd.beta_binomial_prior(_i32([], dev), _i32([], dev), 5, 7)
    assert empty.shape == (0, 5, 7) and empty.dtype == torch.float32
