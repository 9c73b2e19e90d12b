"""Gaussian upsampling without a GPU: the float64 oracle (tests/gaussup_oracle.py) against torch's float64 autograd of the
textbook formula and against central differences; the np.float32 restatement of the kernels' arithmetic -- the CUT rule
and the tiles' token intervals included -- inside the derived bounds on every shape the GPU tests use, and sabotaged
restatements outside them; the C ABI's argument checks and the Python wrappers' rejections."""
import ctypes

import numpy as np
import pytest
import torch

import gaussup_oracle as UO


def _textbook(h, c, a, g, t_x, t_y, off, Ty):
    """energy, masked fill, softmax, bmm: what a caller composes in torch (float64 here)."""
    B, C, Tx = h.shape
    tau = torch.arange(Ty, dtype=h.dtype) + off
    e = g[:, None, :] - a[:, None, :] * (tau[None, :, None] - c[:, None, :]) ** 2
    tok = torch.arange(Tx)[None, :] < t_x[:, None]
    frm = torch.arange(Ty)[None, :] < t_y[:, None]
    e = e.masked_fill(~tok[:, None, :], -1e30)                       # (finite: an utterance without tokens stays finite)
    p = torch.softmax(e, dim=2) * (tok[:, None, :] & frm[:, :, None])
    return torch.bmm(h, p.transpose(1, 2))


@pytest.mark.parametrize("form", ["delta", "sigma"])
@pytest.mark.parametrize("off", [0.0, 0.5])
def test_oracle_against_torch_float64_autograd(form, off):
    rng = np.random.default_rng(5)
    B, C, Tx, Ty = 4, 5, 13, 70
    case = UO.draw_inputs(rng, B, C, Tx, Ty, form)
    case["t_x"][2], case["t_y"][3] = 0, 0                            # an utterance without tokens, one without frames
    g = case["log_weight"] if case["log_weight"] is not None else np.zeros((B, Tx), np.float32)
    ref = UO.gaussian_upsample(case["h"], case["centres"], case["precision"], g, case["t_x"], case["t_y"], off, Ty, case["G"])
    h, c, a, gg = (torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (case["h"], case["centres"], case["precision"], g))
    out = _textbook(h, c, a, gg, torch.from_numpy(case["t_x"]), torch.from_numpy(case["t_y"]), off, Ty)
    (out * torch.tensor(case["G"], dtype=torch.float64)).sum().backward()
    assert (case["durations"] == 0).any() and (np.diff(case["centres"], axis=1) == 0).any()      # coincident centres
    for name, got, want in (("out", ref.out, out.detach()), ("dh", ref.dh, h.grad), ("dc", ref.dc, c.grad),
                            ("da", ref.da, a.grad), ("dg", ref.dg, gg.grad)):
        err = np.abs(got - want.numpy()).max()
        scale = max(np.abs(want.numpy()).max(), 1.0)
        assert err <= 1e-12 * scale, (name, err, scale)
    assert not ref.out[2].any() and not ref.out[3].any() and not ref.dh[2].any() and not ref.dc[3].any()


def test_oracle_against_central_differences():
    rng = np.random.default_rng(9)
    B, C, Tx, Ty = 1, 3, 5, 12
    h = rng.standard_normal((B, C, Tx))
    G = rng.standard_normal((B, C, Ty))
    c = np.sort(rng.uniform(0, Ty, (B, Tx)), axis=1)
    a = rng.uniform(0.05, 0.5, (B, Tx))
    g = rng.standard_normal((B, Tx)) * 0.3
    t_x, t_y = np.array([4]), np.array([10])

    def loss(c_, a_, g_):
        return (UO.gaussian_upsample(h, c_, a_, g_, t_x, t_y, 0.5, Ty, bounds=False).out * G[:, :, :]
                * (np.arange(Ty) < 10)[None, None, :]).sum()
    ref = UO.gaussian_upsample(h, c, a, g, t_x, t_y, 0.5, Ty, G)
    eps = 1e-6
    for name, grad, k in (("dc", ref.dc, 0), ("da", ref.da, 1), ("dg", ref.dg, 2)):
        for x in range(Tx):
            args_p, args_m = [c.copy(), a.copy(), g.copy()], [c.copy(), a.copy(), g.copy()]
            args_p[k][0, x] += eps
            args_m[k][0, x] -= eps
            fd = (loss(*args_p) - loss(*args_m)) / (2 * eps)
            assert abs(fd - grad[0, x]) <= 1e-7 * max(1.0, abs(fd)), (name, x, fd, grad[0, x])
    assert ref.dc[0, 4] == 0 and ref.da[0, 4] == 0 and ref.dg[0, 4] == 0 and not ref.dh[0, :, 4].any()


def test_generators_hold_what_the_tests_rely_on():
    rng = np.random.default_rng(3)
    for (B, Tx, Ty) in [(3, 31, 130), (2, 70, 256), (2, 3, 1030), (2, 300, 1000), (1, 2048, 2100)]:
        for flip in ((0, 1) if B == 1 else (0,)):
            dur, t_x, t_y = UO.edge_durations(rng, B, Tx, Ty, flip)
            tot = np.maximum(dur, 0).sum(1)
            assert dur.dtype == np.float32 and np.array_equal(dur * 4, np.round(dur * 4))
            if B > 1:
                assert tot[0] > Ty and tot[1] < Ty and t_x[0] < Tx and t_x[1] == Tx and t_y[0] == Ty and 0 < t_y[1] < tot[1]
            if Tx >= 8:
                assert ((dur < 0).sum(1) == 1).all() and ((dur == 0).sum(1) >= 3).all()
            if Ty >= 256:
                assert (dur.max(1) > 2 * UO.TILE).all()
            c = UO.centres_of(dur)
            assert (np.diff(c.astype(np.float64), axis=1) >= 0).all()


@pytest.mark.parametrize("shape,form,off", UO.CASES)
def test_fp32_restatement_is_inside_the_bounds(shape, form, off):
    """The kernels' arithmetic in np.float32, tile intervals and all, on every case of the GPU tests: the bounds are
    neither violated by the arithmetic they are derived for nor far above it."""
    case = UO.make_case(shape, form, off)
    B, C, Tx, Ty = shape
    got = UO.restated(case["h"], case["centres"], case["precision"], case["log_weight"], case["t_x"], case["t_y"], off, Ty,
                      case["G"])
    r = UO.ratios(case["ref"], got)
    print(f"{shape} {form} offset {off}: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    # the full token range exactly where it is meant
    want_full = form == "shuffled" and Tx > 2
    for b in range(B):
        if case["t_x"][b] > 2:
            assert got.full[b] == want_full, (b, got.full[b])
    if form == "delta" and Tx >= 300:
        width = max(int(hi - lo) for band in got.bands for lo, hi in band)
        assert width < Tx // 2                                      # a band, not everything
    if form == "flat" and Ty <= 300:                                # (R = sqrt(31 / 1e-4) = 557 frames)
        assert all((band[:, 1] - band[:, 0]).max() == case["t_x"][b] for b, band in enumerate(got.bands))


@pytest.mark.parametrize("sabotage,form,outputs", [("drop_chunk_edge", "delta", ("out", "dh")), ("drop_band_edge", "flat", ("out",)),
                                                   ("frame_offset", "delta", ("out", "dc")), ("skip_r", "sigma", ("dc", "da", "dg")),
                                                   ("partials_off_by_1e-3", "sigma", ("dc", "da", "dg"))])
def test_sabotaged_restatements_are_outside_the_bounds(sabotage, form, outputs):
    shape = (2, 80, 70, 257)
    case = UO.make_case(shape, form, 0.5)
    got = UO.restated(case["h"], case["centres"], case["precision"], case["log_weight"], case["t_x"], case["t_y"], 0.5,
                      shape[3], case["G"], sabotage=sabotage)
    r = UO.ratios(case["ref"], got)
    print(f"{sabotage}: error / bound " + "  ".join(f"{k} {v:.1f}" for k, v in r.items()))
    for k in outputs:
        assert r[k] > 10.0, (sabotage, k, r[k])


def test_planted_disorder_takes_the_full_range():
    """Two centres swapped, a precision of 0, a NaN centre: each sends its utterance -- and only it -- to the full range."""
    shape = (3, 7, 31, 130)
    case = UO.make_case(shape, "delta", 0.0)
    B, C, Tx, Ty = shape
    for plant in ("swap", "zero_precision", "nan"):
        c, a = case["centres"].copy(), case["precision"].copy()
        if plant == "swap":
            k = int(np.argmax(np.diff(c[1, :int(case["t_x"][1])])))
            c[1, k], c[1, k + 1] = c[1, k + 1], c[1, k]
        elif plant == "zero_precision":
            a[1, 3] = 0.0
        else:
            c[1, 5] = np.nan
        t_x, t_y = case["t_x"], case["t_y"]
        full = [UO.band32(c[b], a[b], np.zeros(Tx, np.float32), int(t_x[b]), int(t_y[b]), 0.0, Ty)[1] for b in range(B)]
        assert full == [False, True, False], (plant, full)
        if plant == "swap":
            got = UO.restated(case["h"], c, a, None, t_x, t_y, 0.0, Ty, case["G"])
            ref = UO.gaussian_upsample(case["h"], c, a, None, t_x, t_y, 0.0, Ty, case["G"])
            assert all(v <= 1.0 for v in UO.ratios(ref, got).values())
    # past t_x the order does not matter
    c = case["centres"].copy()
    c[0, int(case["t_x"][0]):] = -5.0
    assert not UO.band32(c[0], case["precision"][0], np.zeros(Tx, np.float32), int(case["t_x"][0]), Ty, 0.0, Ty)[1]


@pytest.mark.parametrize("shape,form", [((3, 7, 31, 130), "delta"), ((2, 80, 70, 257), "sigma"), ((2, 16, 3, 1030), "delta")])
def test_an_outlier_shows_above_the_bound_wherever_it_has_weight(shape, form):
    """What the GPU's planted-outlier test relies on, on the oracle alone: 1000 added to one channel of one token's h
    moves out[c,y] by 1000 p[y,x], and that is more than 4 times the bound of the moved output wherever p >= 1e-3."""
    case = UO.make_case(shape, form, 0.0)
    B, C, Tx, Ty = shape
    for b in range(B):
        for x in {0, int(case["t_x"][b]) - 1, int(case["t_x"][b]) // 2}:
            h = case["h"].copy()
            h[b, 0, x] += 1000.0
            ref = UO.gaussian_upsample(h, case["centres"], case["precision"], case["log_weight"], case["t_x"], case["t_y"], 0.0, Ty)
            p = case["ref"].p[b, :, x]
            move = np.abs(ref.out[b, 0] - case["ref"].out[b, 0])
            step = float(h[b, 0, x]) - float(case["h"][b, 0, x])                   # (1000 as fp32 addition left it)
            assert np.allclose(move, step * p, rtol=1e-9, atol=1e-12)
            big = p >= 1e-3
            assert (move[big] > 4 * ref.b_out[b, 0][big]).all()


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ("aligner_gauss_upsample_f32", "aligner_gauss_upsample_workspace_bytes", "aligner_gauss_upsample_backward_f32",
             "aligner_gauss_upsample_backward_workspace_bytes")
    for name in names:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    for wsb in (lib.aligner_gauss_upsample_workspace_bytes, lib.aligner_gauss_upsample_backward_workspace_bytes):
        assert wsb(0, 80, 200, 1000) == 0 and wsb(1, 0, 200, 1000) == 0 and wsb(1, 80, 0, 1000) == 0 and wsb(1, 80, 200, 0) == 0
        assert wsb(1, 80, 2049, 1000) == 0 and wsb(65536, 80, 200, 1000) == 0
        assert wsb(64, 80, 200, 1000) > 0 and wsb(1, 5, 2048, 2100) > 0 and wsb(1, 1, 1, 1) > 0
    assert lib.aligner_gauss_upsample_backward_workspace_bytes(64, 80, 200, 1000) > lib.aligner_gauss_upsample_workspace_bytes(64, 80, 200, 1000)

    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def fwd(h=p, c=p, a=p, g=None, out=p, ws=p, nws=1 << 20, B=1, C=2, Tx=4, Ty=8):
        return lib.aligner_gauss_upsample_f32(h, c, a, g, None, None, 0.0, out, ws, nws, B, C, Tx, Ty, None)

    def bwd(h=p, c=p, a=p, g=None, gout=p, dh=p, dc=p, da=p, dg=p, ws=p, nws=1 << 20, B=1, C=2, Tx=4, Ty=8):
        return lib.aligner_gauss_upsample_backward_f32(h, c, a, g, None, None, 0.0, gout, dh, dc, da, dg, ws, nws, B, C, Tx, Ty, None)
    # validated before any HIP call: none of these looks for a device (the pointers are host memory)
    for call, required in ((fwd, ("h", "c", "a", "out", "ws")), (bwd, ("h", "c", "a", "gout", "ws"))):
        for kw in required:
            assert call(**{kw: None}) == _lib.EINVAL and b"null" in lib.aligner_last_error(), kw
        for kw in ("B", "C", "Tx", "Ty"):
            assert call(**{kw: 0}) == _lib.EINVAL and b"shape" in lib.aligner_last_error(), kw
        assert call(B=-1) == _lib.EINVAL
        assert call(Tx=2049) == _lib.EDOM and b"Tx=2049" in lib.aligner_last_error()
        assert call(B=65536) == _lib.EDOM
        assert call(nws=0) == _lib.ENOSPC and b"workspace" in lib.aligner_last_error()
    assert fwd(nws=lib.aligner_gauss_upsample_workspace_bytes(1, 2, 4, 8) - 1) == _lib.ENOSPC
    assert bwd(nws=lib.aligner_gauss_upsample_backward_workspace_bytes(1, 2, 4, 8) - 1) == _lib.ENOSPC
    assert bwd(nws=lib.aligner_gauss_upsample_workspace_bytes(1, 2, 4, 8)) == _lib.ENOSPC
    assert bwd(dh=None, dc=None, da=None, dg=None) == _lib.EINVAL and b"no output" in lib.aligner_last_error()
    assert lib.aligner_debug_set_option(b"gaussup_full_range", 0) == 0


def test_python_entry_points_are_exported_and_check_arguments():
    import inspect

    import aligner_amd
    from aligner_amd import gaussup
    for name in ("gaussian_upsample", "gaussian_upsample_at"):
        assert callable(getattr(aligner_amd, name)) and name in aligner_amd.__all__
    assert "oracle" not in inspect.getsource(gaussup)
    assert "ESPnet" in aligner_amd.gaussian_upsample.__doc__ and "t_y" in aligner_amd.gaussian_upsample.__doc__
    h, c, d = torch.zeros(2, 3, 5), torch.zeros(2, 5), torch.ones(2, 5)
    up, at = aligner_amd.gaussian_upsample, aligner_amd.gaussian_upsample_at
    with pytest.raises(ValueError, match="GPU tensor"):
        up(h, d, 7)
    with pytest.raises(ValueError, match="GPU tensor"):
        at(h, c, 0.1, T_mel=7)
    with pytest.raises(ValueError, match=r"\[B,C,T_text\]"):
        up(h[0], d, 7)
    with pytest.raises(ValueError, match=r"\[B,C,T_text\]"):
        at(h[0], c, 0.1, T_mel=7)
    with pytest.raises(ValueError, match=r"durations must be \[B,T_text\]"):
        up(h, torch.ones(2, 6), 7)
    with pytest.raises(ValueError, match="float or integer"):
        up(h, torch.ones(2, 5, dtype=torch.bool), 7)
    with pytest.raises(ValueError, match=r"centres must be \[B,T_text\]"):
        at(h, torch.zeros(2, 6), 0.1, T_mel=7)
    with pytest.raises(ValueError, match="T_mel"):
        at(h, c, 0.1)
    with pytest.raises(ValueError, match="floating-point"):
        at(h, c.long(), 0.1, T_mel=7)
    with pytest.raises(ValueError, match="floating-point"):
        at(h.long(), c, 0.1, T_mel=7)
