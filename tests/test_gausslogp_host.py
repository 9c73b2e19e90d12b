"""Glow-TTS / VITS log-likelihood front end, the parts that need no GPU: the C ABI's symbols and argument checks, the
Python entry points' argument checks, and the float64 oracle (tests/gausslogp_oracle.py) against a cell-by-cell loop and
against the four-term torch formulation those models run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gausslogp_oracle as GO


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aligner_gauss_logp", "aligner_gauss_logp_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    wsb = lib.aligner_gauss_logp_workspace_bytes
    assert wsb(0, 80, 200) == 0
    assert wsb(1, 0, 200) == 0 and wsb(1, 80, 0) == 0
    assert 0 < wsb(1, 80, 200) < wsb(1, 192, 200) < wsb(1, 192, 400) and wsb(2, 80, 200) > wsb(1, 80, 200)
    # the split [Tx,2C] operand: two bf16 halves of every element, at least
    assert wsb(64, 80, 200) >= 64 * 200 * 160 * 4
    assert wsb(1, 257, 200) == 0 and wsb(1, 80, 1025) == 0

    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def call(z=p, mean=p, logstd=p, out=p, ws=p, ld=8, C=4, Tx=4, Ty=8, B=1, dt=_lib.DT_F32):
        return lib.aligner_gauss_logp(z, mean, logstd, None, None, out, dt, ld, ws, 1 << 30, B, C, Tx, Ty, None)
    # validated before any HIP call: none of these looks for a device (the pointers are host memory)
    for kw in ("z", "mean", "logstd", "out", "ws"):
        assert call(**{kw: None}) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    assert call(ld=7) == _lib.EINVAL and b"ld_value" in lib.aligner_last_error()
    assert call(ld=9) == _lib.EINVAL and b"16-byte" in lib.aligner_last_error()          # a pitch of 36 bytes
    assert call(B=-1) == _lib.EINVAL and call(C=0) == _lib.EINVAL and call(Tx=0) == _lib.EINVAL and call(Ty=0, ld=0) == _lib.EINVAL
    assert call(dt=_lib.DT_F16) == _lib.EINVAL and b"dtype" in lib.aligner_last_error()
    assert call(C=257) == _lib.EDOM and b"C=257" in lib.aligner_last_error()
    assert call(Tx=1025) == _lib.EDOM and b"Tx=1025" in lib.aligner_last_error()
    assert call(B=65536) == _lib.EDOM
    assert call(Tx=1024, Ty=1 << 19, ld=1 << 19) == _lib.EDOM and b"2^29" in lib.aligner_last_error()
    assert call(B=0) == 0                                   # an empty batch: nothing to launch


def test_python_entry_points_are_exported_and_check_arguments():
    import aligner_amd
    for name in ("gaussian_logp", "gaussian_align"):
        assert callable(getattr(aligner_amd, name)) and name in aligner_amd.__all__
    import inspect
    from aligner_amd import gausslogp
    assert "oracle" not in inspect.getsource(gausslogp)
    z, m, s = torch.zeros(2, 3, 7), torch.zeros(2, 3, 5), torch.zeros(2, 3, 5)
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.gaussian_logp(z, m, s)
    with pytest.raises(ValueError, match="disagree in B or C"):
        aligner_amd.gaussian_logp(z, torch.zeros(1, 3, 5), torch.zeros(1, 3, 5))
    with pytest.raises(ValueError, match="disagree in B or C"):
        aligner_amd.gaussian_logp(z, torch.zeros(2, 4, 5), torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match="logstd"):
        aligner_amd.gaussian_logp(z, m, torch.zeros(2, 3, 6))
    with pytest.raises(ValueError, match=r"\[B,C,T\]"):
        aligner_amd.gaussian_logp(z[0], m, s)
    for bad in (torch.zeros(2, 5, 8), torch.zeros(2, 7, 5).transpose(1, 2), torch.zeros(2, 5, 9)[:, :, :7],
                torch.zeros(2, 6, 8)[:, :5, :7]):
        with pytest.raises(ValueError, match="out must be"):
            aligner_amd.gaussian_logp(z, m, s, out=bad)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        aligner_amd.gaussian_logp(z, m, s, out=torch.zeros(2, 5, 7, dtype=torch.float16))
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        aligner_amd.gaussian_logp(z, m, s, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="lengths"):
        aligner_amd.gaussian_align(z, m, s, None, None)


def test_oracle_equals_the_triple_loop():
    rng = np.random.default_rng(5)
    z, m, s = GO.draw_inputs(rng, 1, 3, 2, 4)
    value, S, valid = GO.gaussian_logp(z, m, s)
    want, want_S = GO.triple_loop(z, m, s)
    assert valid.all() and value.shape == (1, 2, 4)
    np.testing.assert_allclose(value, want, rtol=1e-14, atol=0)
    np.testing.assert_allclose(S, want_S, rtol=1e-14, atol=0)
    assert (S >= np.abs(value)).all()                     # the magnitude bounds the sum of its signed terms
    # one hand-made cell: C = 1, z = m: only the constant and the log-std remain
    v, S1, _ = GO.gaussian_logp(np.full((1, 1, 1), 0.75, np.float32), np.full((1, 1, 1), 0.75, np.float32),
                                np.full((1, 1, 1), -0.5, np.float32))
    assert v[0, 0, 0] == pytest.approx(-0.5 * math.log(2 * math.pi) + 0.5, rel=1e-15)
    assert S1[0, 0, 0] == pytest.approx(2 * 0.75 ** 2 * math.e + 0.5 + 0.5 * math.log(2 * math.pi), rel=1e-15)


def test_oracle_lengths_zero_the_masked_cells():
    rng = np.random.default_rng(6)
    z, m, s = GO.draw_inputs(rng, 4, 3, 5, 7)
    full, _, _ = GO.gaussian_logp(z, m, s)
    value, _, valid = GO.gaussian_logp(z, m, s, t_x=[5, 2, 0, 3], t_y=[7, 4, 6, -1])
    assert valid[0].all() and valid[1].sum() == 8 and not valid[2].any() and not valid[3].any()
    assert np.array_equal(value[valid], full[valid]) and not value[~valid].any()


def test_oracle_equals_the_torch_four_term_formulation():
    """What a Glow-TTS / VITS step runs (two matmuls, two reductions, broadcast adds), in float64."""
    rng = np.random.default_rng(7)
    z, m, s = GO.draw_inputs(rng, 2, 16, 9, 21)
    value, S, _ = GO.gaussian_logp(z, m, s)
    zt, mt, st = (torch.from_numpy(a).double() for a in (z, m, s))
    w = torch.exp(-2 * st)                                                       # [b, c, t_text]
    logp1 = torch.sum(-0.5 * math.log(2 * math.pi) - st, [1]).unsqueeze(-1)      # [b, t_text, 1]
    logp2 = torch.matmul(w.transpose(1, 2), -0.5 * (zt ** 2))                    # [b, t_text, t_mel]
    logp3 = torch.matmul((mt * w).transpose(1, 2), zt)
    logp4 = torch.sum(-0.5 * (mt ** 2) * w, [1]).unsqueeze(-1)
    four = (logp1 + logp2 + logp3 + logp4).numpy()
    assert np.abs(four - value).max() <= 1e-12 * S.max()
    np.testing.assert_allclose(four, value, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", range(len(GO.PLANTED_CASES)))
def test_planted_cases_hold_for_the_oracle_alone(n):
    """What the GPU's end-to-end test relies on, checked without a GPU for the committed seeds: the pinned search on the
    float64 values rounded to fp32 returns the planted durations, and the split products' error (simulated in numpy) moves
    neither the path nor any value past the tests' bound."""
    case = GO.planted_case(n)
    assert np.array_equal(case["path"].sum(2), case["durations"])
    assert (case["durations"].sum(1) == case["t_y"]).all()
    sim = GO.simulate_split(case["z"], case["mean"], case["logstd"])
    value, S, valid = GO.gaussian_logp(case["z"], case["mean"], case["logstd"], case["t_x"], case["t_y"])
    ratio = (np.abs(sim - value) / S)[valid].max() * 2.0 ** 16
    print(f"case {n}: simulated split products, max |err| / S = {ratio:.3f} * 2^-16")
    assert ratio <= 4.0
    sim_path = GO.search(np.where(valid, sim, 0.0).astype(np.float32), case["t_x"], case["t_y"])
    assert np.array_equal(sim_path, case["path"])


@pytest.mark.parametrize("lo,hi,C", [(0.5, 1.5, 80), (0.05, 2.0, 16)])
def test_simulated_split_products_stay_inside_the_bound(lo, hi, C):
    """Where 2^-14 S comes from: the three split products in exact accumulation stay near 2^-16 S on the tests' input
    families; the factor four is for fp32 accumulation order and exp in fp32."""
    rng = np.random.default_rng(21)
    z, m, s = GO.draw_inputs(rng, 2, C, 37, 90, lo, hi)
    value, S, _ = GO.gaussian_logp(z, m, s)
    ratio = (np.abs(GO.simulate_split(z, m, s) - value) / S).max() * 2.0 ** 16
    print(f"sigma in ({lo}, {hi}), C = {C}: simulated max |err| / S = {ratio:.3f} * 2^-16")
    assert ratio <= 2.0
