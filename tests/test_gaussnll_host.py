"""Glow-TTS / VITS likelihood loss on the hard path, the parts that need no GPU: the float64 oracle
(tests/gaussnll_oracle.py) against torch.autograd on the formula composed from index gathers, the C ABI's symbols and
argument checks, and the Python entry points' argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gausslogp_oracle as GO
import gaussnll_oracle as NO


def _composed(z, m, s, dur, t_y, scale):
    """nll [B] in float64 torch, from gathers along the token axis: no segment algebra of its own."""
    B, C, Ty = z.shape
    out = []
    for b in range(B):
        d = dur[b].clamp_min(0)
        ends = d.cumsum(0)
        y = torch.arange(Ty)
        tok = torch.searchsorted(ends, y, right=True)                     # first x with ends[x] > y
        counts = (tok < len(d)) & (y < (Ty if t_y is None else int(t_y[b])))
        tok = tok.clamp_max(len(d) - 1)
        mg, sg = m[b][:, tok], s[b][:, tok]                               # [C,Ty] gathers
        term = 0.5 * math.log(2 * math.pi) + sg + 0.5 * (z[b] - mg) ** 2 * torch.exp(-2 * sg)
        out.append((term * counts[None, :]).sum())
    nll = torch.stack(out)
    return nll, (nll * scale).sum()


@pytest.mark.parametrize("B,C,Tx,Ty,flip,with_ty", [(2, 3, 9, 40, 0, True), (3, 5, 17, 70, 1, True), (1, 2, 4, 11, 0, False),
                                                     (1, 1, 1, 1, 0, True)])
def test_oracle_gradients_equal_autograd_on_the_composed_formula(B, C, Tx, Ty, flip, with_ty):
    rng = np.random.default_rng(100 + Tx)
    z, m, s = GO.draw_inputs(rng, B, C, Tx, Ty)
    dur, t_y = NO.edge_durations(rng, B, Tx, Ty, flip)
    if not with_ty:
        t_y = None
    scale = rng.standard_normal(B)
    ref = NO.gaussian_nll(z, m, s, dur, t_y, scale)
    zt, mt, st = (torch.from_numpy(a).double().requires_grad_() for a in (z, m, s))
    nll, total = _composed(zt, mt, st, torch.from_numpy(dur).long(), t_y, torch.from_numpy(scale))
    total.backward()
    np.testing.assert_allclose(ref.nll, nll.detach().numpy(), rtol=1e-12, atol=0)
    for got, want, name in ((ref.dz, zt.grad, "dz"), (ref.dm, mt.grad, "dm"), (ref.ds, st.grad, "ds")):
        want = want.numpy()
        err = np.abs(got - want).max()
        assert err <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, err)
        assert np.array_equal(got == 0, want == 0) or name == "ds", name     # (zeros where nothing counts)
    # the counts, and the magnitudes bound their signed sums
    lim = np.full(B, Ty) if t_y is None else np.clip(t_y, 0, Ty)
    assert np.array_equal(ref.count, np.minimum(np.maximum(dur, 0).sum(1), lim))
    assert np.array_equal(ref.n.sum(1), ref.count) and np.array_equal(ref.counts.sum(1), ref.count)
    assert (ref.S_nll >= np.abs(ref.nll)).all()
    assert (ref.A_m * np.abs(scale)[:, None, None] >= np.abs(ref.dm) * (1 - 1e-12)).all()
    assert (ref.A_s * np.abs(scale)[:, None, None] >= np.abs(ref.ds) * (1 - 1e-12)).all()


def test_oracle_by_hand():
    # C = 1, two tokens, durations (2, 1), T_mel = 4: frame 3 has no owner
    z = np.array([[[1.0, 2.0, 5.0, 9.0]]])
    m = np.array([[[1.5, 4.0]]])
    s = np.array([[[0.0, math.log(2.0)]]])
    r = NO.gaussian_nll(z, m, s, np.array([[2, 1]]))
    c = 0.5 * math.log(2 * math.pi)
    assert r.count[0] == 3 and r.n[0].tolist() == [2, 1] and r.counts[0].tolist() == [True, True, True, False]
    assert r.nll[0] == pytest.approx(3 * c + math.log(2.0) + 0.5 * (0.25 + 0.25) + 0.5 * 1.0 / 4.0, rel=1e-15)
    np.testing.assert_allclose(r.dz[0, 0], [-0.5, 0.5, 0.25, 0.0], rtol=1e-15)
    np.testing.assert_allclose(r.dm[0, 0], [0.0, -0.25], rtol=1e-15, atol=1e-17)
    np.testing.assert_allclose(r.ds[0, 0], [2 - 0.5, 1 - 0.25], rtol=1e-15)
    # t_y cuts the second token off: its gradients vanish, a negative duration is no duration
    r = NO.gaussian_nll(z, m, s, np.array([[2, 1]]), t_y=[2])
    assert r.count[0] == 2 and r.dm[0, 0, 1] == 0 and r.ds[0, 0, 1] == 0 and r.dz[0, 0, 2] == 0
    r = NO.gaussian_nll(z, m, s, np.array([[-5, 1]]))
    assert r.count[0] == 1 and r.n[0].tolist() == [0, 1] and r.dz[0, 0, 0] == pytest.approx((1.0 - 4.0) / 4.0)


def test_edge_durations_hold_what_the_gpu_tests_rely_on():
    rng = np.random.default_rng(3)
    for (B, Tx, Ty) in [(3, 31, 130), (2, 70, 256), (2, 3, 1030), (2, 300, 1000), (2, 4, 40), (2, 5, 40), (2, 6, 40)]:
        dur, t_y = NO.edge_durations(rng, B, Tx, Ty)
        tot = np.maximum(dur, 0).sum(1)
        assert tot[0] > Ty and tot[1] < Ty and t_y[0] == Ty and 0 < t_y[1] < tot[1]
        assert ((dur < 0).sum(1) == 1).all() and (dur[:, 1:-1] == 0).sum(1).min() >= 1


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aligner_gauss_nll_f32", "aligner_gauss_nll_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    wsb = lib.aligner_gauss_nll_workspace_bytes
    assert wsb(0, 80, 200) == 0 and wsb(1, 0, 200) == 0 and wsb(1, 80, 0) == 0 and wsb(1, 80, 2049) == 0
    assert wsb(64, 80, 200) >= 64 * 80 * 4 and wsb(1, 5, 2048) >= 20            # one fp32 partial per (utterance, channel)

    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def call(z=p, mean=p, logstd=p, dur=p, nll=p, count=p, dz=None, dm=None, ds=None, ws=p, nws=1 << 20, B=1, C=2, Tx=4, Ty=8):
        return lib.aligner_gauss_nll_f32(z, mean, logstd, dur, None, None, nll, count, dz, dm, ds, ws, nws, B, C, Tx, Ty, None)
    # validated before any HIP call: none of these looks for a device (the pointers are host memory)
    for kw in ("z", "mean", "logstd", "dur", "ws"):
        assert call(**{kw: None}) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
    for kw in ("B", "C", "Tx", "Ty"):
        assert call(**{kw: 0}) == _lib.EINVAL and b"shape" in lib.aligner_last_error(), kw
    assert call(B=-1) == _lib.EINVAL
    for part in ({"dz": p}, {"dm": p}, {"ds": p}, {"dz": p, "dm": p}, {"dz": p, "ds": p}, {"dm": p, "ds": p}):
        assert call(**part) == _lib.EINVAL and b"all three or none" in lib.aligner_last_error(), part
    assert call(nll=None, count=None) == _lib.EINVAL and b"no output" in lib.aligner_last_error()
    assert call(Tx=2049) == _lib.EDOM and b"Tx=2049" in lib.aligner_last_error()
    assert call(B=65536) == _lib.EDOM
    assert call(B=1024, C=1024, Ty=2048) == _lib.EDOM and b"32-bit" in lib.aligner_last_error()
    assert call(B=1024, C=1024, Tx=2048, Ty=8) == _lib.EDOM
    assert call(nws=7) == _lib.ENOSPC and b"workspace" in lib.aligner_last_error()
    assert call(nws=wsb(1, 2, 4) - 1) == _lib.ENOSPC
    assert call(dz=p, dm=p, ds=p, nws=0) == _lib.ENOSPC


def test_python_entry_points_are_exported_and_check_arguments():
    import inspect

    import aligner_amd
    from aligner_amd import gaussnll
    for name in ("gaussian_nll", "gaussian_nll_loss"):
        assert callable(getattr(aligner_amd, name)) and name in aligner_amd.__all__
    assert "oracle" not in inspect.getsource(gaussnll)
    z, m, s, d = torch.zeros(2, 3, 7), torch.zeros(2, 3, 5), torch.zeros(2, 3, 5), torch.ones(2, 5, dtype=torch.int32)
    for fn in (aligner_amd.gaussian_nll, aligner_amd.gaussian_nll_loss):
        with pytest.raises(ValueError, match="GPU tensor"):
            fn(z, m, s, d)
        with pytest.raises(ValueError, match="disagree in B or C"):
            fn(z, torch.zeros(1, 3, 5), torch.zeros(1, 3, 5), d)
        with pytest.raises(ValueError, match="disagree in B or C"):
            fn(z, torch.zeros(2, 4, 5), torch.zeros(2, 4, 5), d)
        with pytest.raises(ValueError, match="logstd"):
            fn(z, m, torch.zeros(2, 3, 6), d)
        with pytest.raises(ValueError, match=r"\[B,C,T\]"):
            fn(z[0], m, s, d)
        with pytest.raises(ValueError, match=r"durations must be \[B,T_text\]"):
            fn(z, m, s, torch.ones(2, 6, dtype=torch.int32))
        with pytest.raises(ValueError, match="integer"):
            fn(z, m, s, torch.ones(2, 5))
        with pytest.raises(ValueError, match="holds no durations"):
            fn(z, m, s, aligner_amd.Alignment(None, None, None))
        with pytest.raises(ValueError, match="t_y must have one entry"):
            fn(z, m, s, d, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="reduction"):
        aligner_amd.gaussian_nll_loss(z, m, s, d, reduction="batchmean")
