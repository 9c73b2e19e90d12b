"""Gradient of the Glow-TTS / VITS log-likelihood tensor, the parts that need no GPU: the float64 oracle
(tests/gausslogp_bwd_oracle.py) against float64 torch.autograd through the forward oracle's formula, the magnitude S,
the numpy simulation of the kernels' split products that the GPU tests' bound 2^-14 S rests on, the C ABI's symbols and
argument checks, and the Python entry points' argument checks."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import gausslogp_bwd_oracle as BO
import gausslogp_oracle as GO


def autograd_reference(G, z, m, s, t_x=None, t_y=None):
    """d <G, value> / d (z, m, s) by float64 autograd through the direct (z - m)^2 formula."""
    zt, mt, st = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_() for a in (z, m, s))
    d = zt[:, :, None, :] - mt[:, :, :, None]                                  # [B,C,Tx,Ty]
    value = (-GO.HALF_LN_2PI - st[:, :, :, None] - 0.5 * d * d * torch.exp(-2.0 * st[:, :, :, None])).sum(1)
    B, C, Ty = z.shape
    valid = torch.from_numpy(BO.valid_cells(B, m.shape[2], Ty, t_x, t_y))
    Gt = torch.where(valid, torch.from_numpy(np.asarray(G, np.float64)), torch.zeros((), dtype=torch.float64))
    (value * Gt).sum().backward()
    return zt.grad.numpy(), mt.grad.numpy(), st.grad.numpy()


@pytest.mark.parametrize("B,C,Tx,Ty,t_x,t_y", [(1, 1, 1, 1, None, None), (2, 3, 5, 7, None, None), (3, 4, 6, 9, [6, 0, 2], [9, 5, 4]),
                                               (2, 16, 9, 21, [9, 4], [20, 21])])
def test_oracle_equals_float64_autograd(B, C, Tx, Ty, t_x, t_y):
    rng = np.random.default_rng(31 + C)
    z, m, s = GO.draw_inputs(rng, B, C, Tx, Ty, t_x=t_x)
    G = BO.dense_cotangent(rng, B, Tx, Ty)
    got = BO.backward(G, z, m, s, t_x, t_y)
    for name, want in zip(("dz", "dm", "ds"), autograd_reference(G, z, m, s, t_x, t_y)):
        np.testing.assert_allclose(got[name], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        assert (got["S_" + name] >= np.abs(got[name]) * (1 - 1e-12)).all(), name     # the magnitude bounds the signed sum
    if t_x is not None:
        valid = BO.valid_cells(B, Tx, Ty, t_x, t_y)
        assert not got["dz"][~np.broadcast_to(valid.any(1)[:, None, :], got["dz"].shape)].any()
        assert not got["dm"][~np.broadcast_to(valid.any(2)[:, None, :], got["dm"].shape)].any()
        # what G holds outside the lengths is not an input
        poisoned = np.where(valid, G, np.nan)
        again = BO.backward(poisoned, z, m, s, t_x, t_y)
        assert all(np.array_equal(again[k], got[k]) for k in got)


def test_oracle_one_cell_by_hand_and_grad_scale():
    # C = 1, one token, one frame: z = 1.5, m = 0.5, s = ln 2 (w = 1/4), G = 2: d = 1
    z, m = np.full((1, 1, 1), 1.5, np.float32), np.full((1, 1, 1), 0.5, np.float32)
    s = np.full((1, 1, 1), math.log(2.0))
    o = BO.backward(np.full((1, 1, 1), 2.0), z, m, s)
    assert o["dz"][0, 0, 0] == pytest.approx(-2 * 1.0 * 0.25, rel=1e-15)
    assert o["dm"][0, 0, 0] == pytest.approx(2 * 1.0 * 0.25, rel=1e-15)
    assert o["ds"][0, 0, 0] == pytest.approx(2 * (1.0 * 0.25 - 1.0), rel=1e-15)
    assert o["S_dz"][0, 0, 0] == pytest.approx(2 * 0.25 * 2.0, rel=1e-15) and o["S_dm"][0, 0, 0] == o["S_dz"][0, 0, 0]
    assert o["S_ds"][0, 0, 0] == pytest.approx(2 * (1 + 0.25 * 4.0), rel=1e-15)
    # grad_scale[b] multiplies the utterance's cotangent
    rng = np.random.default_rng(3)
    z, m, s = GO.draw_inputs(rng, 2, 3, 4, 6)
    G = BO.dense_cotangent(rng, 2, 4, 6)
    a = BO.backward(G, z, m, s, grad_scale=[0.5, -3.0])
    b = BO.backward(G * np.array([0.5, -3.0])[:, None, None], z, m, s)
    assert all(np.allclose(a[k], b[k], rtol=1e-15, atol=0) for k in a)


def simulated_ratios(G, z, m, s, t_x=None, t_y=None):
    o = BO.backward(G, z, m, s, t_x, t_y)
    out = []
    for name, sim in zip(("dz", "dm", "ds"), BO.simulate_split(G, z, m, s, t_x, t_y)):
        S = o["S_" + name]
        live = S > 0
        assert not sim[~live].any()
        out.append(float((np.abs(sim - o[name])[live] / S[live]).max()) * 2.0 ** 16)
    return out


@pytest.mark.parametrize("kind", ["dense", "posterior"])
@pytest.mark.parametrize("lo,hi,C,Ty", [(0.5, 1.5, 80, 200), (0.05, 2.0, 16, 200), (0.5, 1.5, 80, 1000), (0.05, 2.0, 16, 1000)])
def test_simulated_split_products_stay_inside_the_bound(lo, hi, C, Ty, kind):
    """Where 2^-14 S comes from: the kernels' three split products per fp32 product stay below 2 * 2^-16 S on the input
    families the GPU tests use (dense and posterior-like cotangents); the remaining factor two is for the fp32
    accumulation order and exp in fp32."""
    rng = np.random.default_rng(41)
    t_x, t_y = np.array([70, 52], np.int32), np.array([Ty, (4 * Ty) // 5 + 1], np.int32)
    z, m, s, dur = GO.planted(rng, C, 70, Ty, t_x, t_y, lo, hi)
    G = BO.dense_cotangent(rng, 2, 70, Ty) if kind == "dense" else BO.posterior_cotangent(rng, dur, Ty)
    ratios = simulated_ratios(G, z, m, s, t_x, t_y)
    print(f"sigma in ({lo}, {hi}), C = {C}, Ty = {Ty}, {kind} G: simulated max |err| / S = "
          f"{ratios[0]:.3f} (dz) {ratios[1]:.3f} (dm) {ratios[2]:.3f} (ds) * 2^-16")
    assert max(ratios) <= 2.0


def test_simulation_is_exact_on_small_integers():
    """z, m in {-3..3}, s = 0, G in {-2..2}: every operand is a bf16 number, the simulation equals the oracle."""
    rng = np.random.default_rng(8)
    z = rng.integers(-3, 4, (2, 5, 40)).astype(np.float32)
    m = rng.integers(-3, 4, (2, 5, 9)).astype(np.float32)
    s = np.zeros((2, 5, 9), np.float32)
    G = rng.integers(-2, 3, (2, 9, 40)).astype(np.float32)
    o = BO.backward(G, z, m, s, [9, 4], [33, 40])
    for name, sim in zip(("dz", "dm", "ds"), BO.simulate_split(G, z, m, s, [9, 4], [33, 40])):
        assert np.array_equal(sim, o[name]), name


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aligner_gauss_logp_backward_f32", "aligner_gauss_logp_backward_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = built_lib
    assert lib.aligner_abi_version() == 5                                # additive: the version stays
    wsb = lib.aligner_gauss_logp_backward_workspace_bytes
    assert wsb(0, 80, 200, 1000) == 0 and wsb(1, 0, 200, 1000) == 0 and wsb(1, 80, 0, 1000) == 0 and wsb(1, 80, 200, 0) == 0
    assert wsb(1, 257, 200, 1000) == 0 and wsb(1, 80, 1025, 1000) == 0 and wsb(65536, 80, 200, 1000) == 0
    assert 0 < wsb(1, 80, 200, 1000) < wsb(1, 192, 200, 1000) and wsb(1, 80, 200, 1000) < wsb(2, 80, 200, 1000)
    # the split (z, z^2) operand: two bf16 halves of each, at least
    assert wsb(64, 80, 200, 1000) >= 64 * 80 * 1000 * 8

    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data

    def call(g=p, scale=None, z=p, mean=p, logstd=p, dz=p, dm=p, ds=p, ws=p, wsn=1 << 30, ld=8, C=4, Tx=4, Ty=8, B=1):
        return lib.aligner_gauss_logp_backward_f32(g, ld, scale, z, mean, logstd, None, None, dz, dm, ds, ws, wsn, B, C, Tx, Ty, None)
    # validated before any HIP call: none of these looks for a device (the pointers are host memory)
    for kw in ("g", "z", "mean", "logstd", "ws"):
        assert call(**{kw: None}) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    assert call(dz=None, dm=None, ds=None) == _lib.EINVAL and b"no output" in lib.aligner_last_error()
    assert call(ld=7) == _lib.EINVAL and b"ld_grad" in lib.aligner_last_error()
    assert call(ld=9) == _lib.EINVAL and b"16-byte" in lib.aligner_last_error()          # a pitch of 36 bytes
    assert call(B=-1) == _lib.EINVAL and call(C=0) == _lib.EINVAL and call(Tx=0) == _lib.EINVAL and call(Ty=0, ld=0) == _lib.EINVAL
    assert call(C=257) == _lib.EDOM and b"C=257" in lib.aligner_last_error()
    assert call(Tx=1025) == _lib.EDOM and b"Tx=1025" in lib.aligner_last_error()
    assert call(B=65536) == _lib.EDOM
    assert call(wsn=wsb(1, 4, 4, 8) - 1) == _lib.ENOSPC and b"workspace" in lib.aligner_last_error()
    assert call(B=0) == 0                                   # an empty batch: nothing to launch
    assert call(B=0, dz=None, dm=None) == 0


def test_python_entry_points_are_exported_and_check_arguments():
    import aligner_amd
    from aligner_amd import gausslogp
    for name in ("gaussian_logp_backward", "gaussian_forward_sum_loss"):
        assert callable(getattr(aligner_amd, name)) and name in aligner_amd.__all__
    assert "oracle" not in inspect.getsource(gausslogp)
    assert "differentiable" in inspect.signature(aligner_amd.gaussian_logp).parameters
    z, m, s, g = torch.zeros(2, 3, 7), torch.zeros(2, 3, 5), torch.zeros(2, 3, 5), torch.zeros(2, 5, 7)
    bwd = aligner_amd.gaussian_logp_backward
    with pytest.raises(ValueError, match="GPU tensor"):
        bwd(g, z, m, s)
    with pytest.raises(ValueError, match="disagree in B or C"):
        bwd(g, z, torch.zeros(1, 3, 5), torch.zeros(1, 3, 5))
    with pytest.raises(ValueError, match="disagree in B or C"):
        bwd(g, z, torch.zeros(2, 4, 5), torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match="logstd"):
        bwd(g, z, m, torch.zeros(2, 3, 6))
    with pytest.raises(ValueError, match=r"\[B,C,T\]"):
        bwd(g, z[0], m, s)
    with pytest.raises(ValueError, match="grad_value"):
        bwd(torch.zeros(2, 7, 5), z, m, s)
    with pytest.raises(ValueError, match="grad_value"):
        bwd(g[0], z, m, s)
    with pytest.raises(ValueError, match="at least one"):
        bwd(g, z, m, s, need_z=False, need_mean=False, need_logstd=False)
    # differentiable=True: fp32 results only, and never into a caller's tensor
    with pytest.raises(ValueError, match="float32"):
        aligner_amd.gaussian_logp(z, m, s, differentiable=True, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out"):
        aligner_amd.gaussian_logp(z, m, s, differentiable=True, out=torch.zeros(2, 5, 7))
    with pytest.raises(ValueError, match="GPU tensor"):
        aligner_amd.gaussian_logp(z.requires_grad_(), m, s, differentiable=True)
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.gaussian_forward_sum_loss(z, m, s, torch.tensor([5, 5]), torch.tensor([7, 7]), reduction="max")
    with pytest.raises(ValueError, match="lengths"):
        aligner_amd.gaussian_forward_sum_loss(z, m, s, None, None)
