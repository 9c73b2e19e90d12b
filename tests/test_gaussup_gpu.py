"""gaussian_upsample_at() / gaussian_upsample() on the GPU against the float64 oracle (tests/gaussup_oracle.py).

The bounds are derived, not tuned: the oracle's module text states them term by term (u = 2^-24, K = 8, K' = 14, the
truncation at e^-30) from the kernels' operation count; tests/test_gaussup_host.py holds an np.float32 restatement of that
arithmetic inside them and sabotaged ones outside.  Every test prints the observed ratio to its bound.

Shapes (gaussup_oracle.SHAPES) sit at the edges of the kernels' structure, each in the delta form (0.1), the sigma form,
with a = 1e-4 (the band is everything) and with shuffled centres (the full-range path), at frame offsets 0 and 0.5; the
durations hold runs of zero-duration tokens, a negative entry, a token longer than two frame tiles, a sum above T_mel with
t_x < T_text in one utterance and a sum below it with t_y below the sum in another.  The launch has one form; the full
token range is also pinned through the library's "gaussup_full_range" switch."""
import contextlib
import math

import numpy as np
import pytest
import torch

import gaussup_oracle as UO
from aligner_amd import _lib, gaussian_upsample, gaussian_upsample_at
from aligner_amd import gaussup as gaussup_module

pytestmark = pytest.mark.gpu

U = UO.U


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def to_dev(case, dev):
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("h", "centres", "precision", "t_x", "t_y", "G")}
    t["log_weight"] = None if case["log_weight"] is None else torch.from_numpy(case["log_weight"]).to(dev)
    return t


def run(t, off, Ty, h=None, G=None, grads=True):
    """out and (dh, dc, da, dg) through autograd on the raw operation."""
    h = (t["h"] if h is None else h).clone().requires_grad_(grads)
    c = t["centres"].clone().requires_grad_(grads)
    a = t["precision"].clone().requires_grad_(grads)
    g = None if t["log_weight"] is None else t["log_weight"].clone().requires_grad_(grads)
    out = gaussian_upsample_at(h, c, a, g, Ty, t["t_x"], t["t_y"], off)
    if not grads:
        return out
    out.backward(t["G"] if G is None else G)
    dg = torch.zeros_like(c) if g is None else g.grad
    return out.detach(), h.grad, c.grad, a.grad, dg


class Got:
    def __init__(self, outs, with_dg=True):
        self.out, self.dh, self.dc, self.da, self.dg = (o.cpu().numpy() for o in outs)
        if not with_dg:
            self.dg = None


@contextlib.contextmanager
def full_range():
    lib = _lib.load()
    assert lib.aligner_debug_set_option(b"gaussup_full_range", 1) == 0
    try:
        yield
    finally:
        lib.aligner_debug_set_option(b"gaussup_full_range", 0)


def check_case(dev, shape, form, off, note=""):
    case = UO.make_case(shape, form, off)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    outs = run(t, off, Ty)
    assert outs[0].shape == (B, C, Ty) and outs[1].shape == (B, C, Tx) and outs[2].shape == (B, Tx)
    assert all(o.dtype == torch.float32 for o in outs)
    r = UO.ratios(ref, Got(outs, with_dg=case["log_weight"] is not None))
    print(f"{shape} {form} offset {off}{note}: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (shape, form, off, r)
    # +0.0 where nothing counts
    dead_y = torch.from_numpy(~ref.counts).to(dev)[:, None, :].expand(B, C, Ty)
    dead_x = torch.from_numpy(np.arange(Tx)[None, :] >= ref.tx[:, None]).to(dev)
    assert not bits(outs[0])[dead_y].any() and not bits(outs[1])[dead_x[:, None, :].expand(B, C, Tx)].any()
    for o in outs[2:]:
        assert not bits(o)[dead_x].any()
    return outs


@pytest.mark.parametrize("shape,form,off", UO.CASES)
def test_forward_and_gradients_against_the_oracle(dev, shape, form, off):
    outs = check_case(dev, shape, form, off)
    case = UO.make_case(shape, form, off)
    again = run(to_dev(case, dev), off, shape[3])                   # two runs: the same bits in every output
    for a, b in zip(outs, again):
        assert torch.equal(bits(a), bits(b))
    # without autograd, and without lengths: the full extent
    t = to_dev(case, dev)
    plain = run(t, off, shape[3], grads=False)
    assert not plain.requires_grad and torch.equal(bits(plain), bits(outs[0]))
    full = UO.gaussian_upsample(case["h"], case["centres"], case["precision"], case["log_weight"], None, None, off, shape[3])
    got = gaussian_upsample_at(t["h"], t["centres"], t["precision"], t["log_weight"], shape[3], frame_offset=off)
    r = UO.ratio(got.cpu().numpy(), full.out, full.b_out)
    print(f"{shape} {form} offset {off} no lengths: error / bound out {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("shape,form", [((3, 7, 31, 130), "delta"), ((2, 80, 70, 257), "sigma"), ((2, 16, 3, 1030), "delta"),
                                        ((3, 7, 31, 130), "flat"), ((2, 80, 70, 256), "shuffled")])
def test_full_range_pinned_against_the_oracle(dev, shape, form):
    """Every check of the test above with every tile on the full token range.  Where the launch's own intervals are the
    full range already (shuffled centres; a = 1e-4 on a short utterance) the sums are the same sums: the same bits."""
    free = check_case(dev, shape, form, 0.5)
    with full_range():
        held = check_case(dev, shape, form, 0.5, " full range")
    if form in ("flat", "shuffled"):
        for a, b in zip(free, held):
            assert torch.equal(bits(a), bits(b))


def _band_edge_tokens(case, b, Tx, Ty, off):
    g = case["log_weight"][b] if case["log_weight"] is not None else np.zeros(Tx, np.float32)
    tx = int(case["t_x"][b])
    band, _ = UO.band32(case["centres"][b], case["precision"][b], g, tx, int(case["t_y"][b]), off, Ty)
    xs = {0, tx - 1, tx}
    for lo, hi in band:
        if hi > lo:
            xs.update((lo - 1, lo, hi - 1, hi))
    return sorted(x for x in xs if 0 <= x < Tx)


@pytest.mark.parametrize("shape,form", [((3, 7, 31, 130), "delta"), ((2, 80, 70, 257), "sigma"), ((2, 192, 300, 1000), "delta")])
def test_planted_outliers_in_h_move_out_by_the_oracles_amount(dev, shape, form):
    """1000 added to one channel of one token's h: the first token, the last valid one, one either side of every frame
    tile's interval edge (gaussup_oracle.band32 restates the kernel's intervals) and the first past t_x, in every
    utterance at once.  out moves by step * p[y,x] within the moved output's bound at every frame (that this shows above
    4 x the bound wherever p >= 1e-3: tests/test_gaussup_host.py); the other channels keep their bits; a token past t_x
    moves nothing, bit for bit."""
    off = 0.0
    case = UO.make_case(shape, form, off)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    base = run(t, off, Ty, grads=False)
    tokens = [_band_edge_tokens(case, b, Tx, Ty, off) for b in range(B)]
    worst, moved = 0.0, 0
    coef = ((ref.n_y + UO.K_SUM) * U + UO.K_ENERGY * U * ref.E_y)                                 # [B,Ty]
    for i in range(max(len(x) for x in tokens)):
        hh = t["h"].clone()
        picks = []
        for b in range(B):
            x = tokens[b][min(i, len(tokens[b]) - 1)]
            c = (x + b) % C
            hh[b, c, x] += 1000.0
            picks.append((x, c))
        got = run(t, off, Ty, h=hh, grads=False)
        hh_np, got_np = hh.cpu().numpy(), got.cpu().numpy()
        for b, (x, c) in enumerate(picks):
            if x >= ref.tx[b]:
                assert torch.equal(bits(got[b]), bits(base[b])), (shape, b, x)
                continue
            step = float(hh_np[b, c, x]) - float(case["h"][b, c, x])
            want = ref.out[b, c] + step * ref.p[b, :, x]
            hmax = max(np.abs(hh_np[b, :, :int(ref.tx[b])]).max(), 0.0)
            bound = coef[b] * (ref.Sph[b, c] + (abs(float(hh_np[b, c, x])) - abs(float(case["h"][b, c, x]))) * ref.p[b, :, x]) \
                + 2 * Tx * math.exp(-UO.CUT) * hmax * ref.counts[b]
            worst = max(worst, UO.ratio(got_np[b, c], want, bound))
            moved += 1
            others = [k for k in range(C) if k != c]
            assert torch.equal(bits(got[b, others]), bits(base[b, others])), (shape, b, x)
    print(f"{shape} {form}: {moved} outliers in h, worst error / bound {worst:.3f}")
    assert worst <= 1.0 and moved > 0


@pytest.mark.parametrize("shape,form", [((3, 7, 31, 130), "delta"), ((2, 80, 70, 257), "sigma")])
def test_planted_outliers_in_g_out_move_the_gradients_by_the_oracles_amount(dev, shape, form):
    """1000 added to one channel of one frame of G: frame 0, the last counting frame, either side of every multiple of 64
    and the first frame past t_y.  A counting frame moves every gradient to the oracle's values on the moved G, within
    their bounds; a frame past t_y moves nothing, bit for bit."""
    off = 0.5
    case = UO.make_case(shape, form, off)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    base = run(t, off, Ty)
    frames = []
    for b in range(B):
        ys = {0, int(ref.ty[b]) - 1, int(ref.ty[b])}
        for e in range(64, Ty, 64):
            ys.update((e - 1, e))
        frames.append(sorted(y for y in ys if 0 <= y < Ty))
    worst = {}
    for i in range(max(len(f) for f in frames)):
        GG = t["G"].clone()
        picks = []
        for b in range(B):
            y = frames[b][min(i, len(frames[b]) - 1)]
            GG[b, (y + b) % C, y] += 1000.0
            picks.append(y)
        got = run(t, off, Ty, G=GG)
        moved = UO.gaussian_upsample(case["h"], case["centres"], case["precision"], case["log_weight"], case["t_x"], case["t_y"],
                                     off, Ty, GG.cpu().numpy())
        for b, y in enumerate(picks):
            if y >= ref.ty[b]:
                for o, o0 in zip(got, base):
                    assert torch.equal(bits(o[b]), bits(o0[b])), (shape, b, y)
        r = UO.ratios(moved, Got(got, with_dg=case["log_weight"] is not None))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{shape} {form}: outliers in G, worst error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256)])
def test_nothing_counts(dev, shape):
    """t_x = 0 and t_y = 0: every output +0.0 bit for bit, in that utterance only; empty shapes: zeros without a launch."""
    case = UO.make_case(shape, "sigma", 0.0)
    t = to_dev(case, dev)
    B, C, Tx, Ty = shape
    for name in ("t_x", "t_y"):
        tt = dict(t)
        lens = t[name].clone()
        lens[0] = 0
        tt[name] = lens
        outs = run(tt, 0.0, Ty)
        for o in outs:
            assert not bits(o[0]).any() and o[1].any()
        np_lens = {k: case[k] for k in ("t_x", "t_y")}
        np_lens[name] = lens.cpu().numpy()
        ref = UO.gaussian_upsample(case["h"], case["centres"], case["precision"], case["log_weight"], np_lens["t_x"], np_lens["t_y"],
                                   0.0, Ty, case["G"])
        assert all(v <= 1.0 for v in UO.ratios(ref, Got(outs)).values())
    h0 = t["h"][:, :, :0].clone().requires_grad_()
    out = gaussian_upsample_at(h0, t["centres"][:, :0], 0.1, None, Ty)
    assert out.shape == (B, C, Ty) and not out.any()
    out.sum().backward()
    assert h0.grad.shape == (B, C, 0)
    assert gaussian_upsample_at(t["h"], t["centres"], 0.1, None, 0).shape == (B, C, 0)
    assert gaussian_upsample_at(t["h"][:0], t["centres"][:0], 0.1, None, 5).shape == (0, C, 5)


def test_canaries_around_the_outputs_and_the_workspace(dev):
    """The C ABI on buffers with guard bands: out, dh, dc, da, dg and both workspaces are written inside their extents
    only (the workspace: inside what *_workspace_bytes returns)."""
    shape = (2, 80, 70, 257)
    case = UO.make_case(shape, "sigma", 0.5)
    t = to_dev(case, dev)
    B, C, Tx, Ty = shape
    lib = _lib.load()
    PAD = 1024

    def guarded(n):
        buf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
        buf.view(torch.int32)[:PAD] = 0x7FC0BEEF
        buf.view(torch.int32)[PAD + n:] = 0x7FC0BEEF
        return buf

    def intact(buf, n):
        v = buf.view(torch.int32)
        return bool((v[:PAD] == 0x7FC0BEEF).all() and (v[PAD + n:] == 0x7FC0BEEF).all())
    nf = lib.aligner_gauss_upsample_workspace_bytes(B, C, Tx, Ty)
    nb = lib.aligner_gauss_upsample_backward_workspace_bytes(B, C, Tx, Ty)
    assert nf % 4 == 0 and nb % 4 == 0
    out, dh, ws_f, ws_b = guarded(B * C * Ty), guarded(B * C * Tx), guarded(nf // 4), guarded(nb // 4)
    dc, da, dg = guarded(B * Tx), guarded(B * Tx), guarded(B * Tx)
    p = lambda buf: buf.data_ptr() + 4 * PAD                                     # noqa: E731
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.aligner_gauss_upsample_f32(t["h"].data_ptr(), t["centres"].data_ptr(), t["precision"].data_ptr(),
                                              t["log_weight"].data_ptr(), t["t_x"].data_ptr(), t["t_y"].data_ptr(), 0.5, p(out),
                                              p(ws_f), nf, B, C, Tx, Ty, stream))
    _lib.check(lib.aligner_gauss_upsample_backward_f32(t["h"].data_ptr(), t["centres"].data_ptr(), t["precision"].data_ptr(),
                                                       t["log_weight"].data_ptr(), t["t_x"].data_ptr(), t["t_y"].data_ptr(), 0.5,
                                                       t["G"].data_ptr(), p(dh), p(dc), p(da), p(dg), p(ws_b), nb, B, C, Tx, Ty,
                                                       stream))
    torch.cuda.synchronize()
    for buf, n in ((out, B * C * Ty), (dh, B * C * Tx), (ws_f, nf // 4), (ws_b, nb // 4), (dc, B * Tx), (da, B * Tx), (dg, B * Tx)):
        assert intact(buf, n)
    outs = [buf[PAD:PAD + n].view(s) for buf, n, s in ((out, B * C * Ty, (B, C, Ty)), (dh, B * C * Tx, (B, C, Tx)),
                                                       (dc, B * Tx, (B, Tx)), (da, B * Tx, (B, Tx)), (dg, B * Tx, (B, Tx)))]
    assert not any(torch.isnan(o).any() for o in outs)                                    # every element was written
    for a, b in zip(outs, run(t, 0.5, Ty)):                                               # the wrapper: the same call
        assert torch.equal(bits(a), bits(b))


def _durations_case(dev, shape):
    case = UO.make_case(shape, "sigma", 0.0)
    t = to_dev(case, dev)
    rng = np.random.default_rng(17)
    sigma = torch.from_numpy(rng.uniform(0.5, 3.0, (shape[0], shape[2])).astype(np.float32)).to(dev)
    dur = torch.from_numpy(case["durations"]).to(dev)
    return case, t, dur, sigma


@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256)])
def test_autograd_through_durations_and_sigma(dev, shape):
    """gaussian_upsample() with float durations and sigma requiring grad: the oracle runs on the centres, precisions and
    log-weights torch hands the kernel (the same fp32 expressions, evaluated here once more) and is chained through
    cumsum and 1 / (2 sigma^2), -ln sigma in float64.  The chain in torch is fp32: a reversed cumsum of at most T_text
    terms and a few elementwise roundings on top of each gradient's own bound.  And the composed torch fp32 path on the
    GPU -- energy, masked fill, softmax, bmm, .backward() -- is within twice the bound of it."""
    case, t, dur, sigma = _durations_case(dev, shape)
    B, C, Tx, Ty = shape
    d1, s1, h1 = dur.clone().requires_grad_(), sigma.clone().requires_grad_(), t["h"].clone().requires_grad_()
    out = gaussian_upsample(h1, d1, Ty, t["t_x"], t["t_y"], sigma=s1, frame_offset=0.5)
    out.backward(t["G"])
    with torch.no_grad():
        dpos = dur.clamp_min(0)
        cen = torch.cumsum(dpos, dim=1) - 0.5 * dpos
        a, g = 0.5 / (sigma * sigma), -torch.log(sigma)
    ref = UO.gaussian_upsample(case["h"], cen.cpu().numpy(), a.cpu().numpy(), g.cpu().numpy(), case["t_x"], case["t_y"], 0.5, Ty,
                               case["G"])
    sg = sigma.double().cpu().numpy()
    want_ds = ref.da * (-1.0 / sg ** 3) + ref.dg * (-1.0 / sg)
    b_ds = ref.b_da / sg ** 3 + ref.b_dg / sg + 8 * U * (np.abs(ref.da) / sg ** 3 + np.abs(ref.dg) / sg)
    live = case["durations"] >= 0                                                         # (a negative entry: clamped, no gradient)
    rev = np.cumsum(ref.dc[:, ::-1], axis=1)[:, ::-1]
    want_dd = (rev - 0.5 * ref.dc) * live
    b_rev = np.cumsum(ref.b_dc[:, ::-1], axis=1)[:, ::-1] + (Tx + 2) * U * np.cumsum(np.abs(ref.dc)[:, ::-1], axis=1)[:, ::-1]
    b_dd = (b_rev + 0.5 * ref.b_dc + 2 * U * np.abs(ref.dc)) * live
    r = {"out": UO.ratio(out.detach().cpu().numpy(), ref.out, ref.b_out), "dh": UO.ratio(h1.grad.cpu().numpy(), ref.dh, ref.b_dh),
         "dsigma": UO.ratio(s1.grad.cpu().numpy(), want_ds, b_ds), "ddur": UO.ratio(d1.grad.cpu().numpy(), want_dd, b_dd)}
    print(f"{shape}: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r

    d2, s2, h2 = dur.clone().requires_grad_(), sigma.clone().requires_grad_(), t["h"].clone().requires_grad_()
    dp = d2.clamp_min(0)
    c2 = torch.cumsum(dp, dim=1) - 0.5 * dp
    tau = torch.arange(Ty, device=dev, dtype=torch.float32) + 0.5
    e = -torch.log(s2)[:, None, :] - (0.5 / (s2 * s2))[:, None, :] * (tau[None, :, None] - c2[:, None, :]) ** 2
    tok = torch.arange(Tx, device=dev)[None, :] < t["t_x"][:, None]
    frm = torch.arange(Ty, device=dev)[None, :] < t["t_y"][:, None]
    pw = torch.softmax(e.masked_fill(~tok[:, None, :], float("-inf")), dim=2) * frm[:, :, None]
    composed = torch.bmm(h2, pw.transpose(1, 2))
    composed.backward(t["G"])
    r2 = {"out": UO.ratio(out.detach().cpu().numpy(), composed.detach().double().cpu().numpy(), 2 * ref.b_out),
          "dh": UO.ratio(h1.grad.cpu().numpy(), h2.grad.double().cpu().numpy(), 2 * ref.b_dh),
          "dsigma": UO.ratio(s1.grad.cpu().numpy(), s2.grad.double().cpu().numpy(), 2 * b_ds),
          "ddur": UO.ratio(d1.grad.cpu().numpy(), d2.grad.double().cpu().numpy(), 2 * b_dd)}
    print(f"{shape}: |fused - composed| / (2 bound) " + "  ".join(f"{k} {v:.3f}" for k, v in r2.items()))
    assert all(v <= 1.0 for v in r2.values()), r2


def test_autograd_only_h_requires_grad(dev, monkeypatch):
    """Only dh is asked of the library (the other three pointers NULL), nothing else gets a gradient; integer durations and
    the delta form; nothing requires grad: no graph."""
    shape = (3, 7, 31, 130)
    case, t, dur, sigma = _durations_case(dev, shape)
    Ty = shape[3]
    asked = []
    real = gaussup_module._backward

    def spy(*args):
        asked.append(args[-4:])
        res = real(*args)
        assert [r is not None for r in res] == list(args[-4:])
        return res
    monkeypatch.setattr(gaussup_module, "_backward", spy)
    h = t["h"].clone().requires_grad_()
    idur = dur.round().to(torch.int32)
    out = gaussian_upsample(h, idur, Ty, t["t_x"], t["t_y"], delta=0.1)
    out.backward(t["G"])
    assert asked == [(True, False, False, False)]
    dpos = idur.clamp_min(0).double().cpu().numpy()
    cen = (np.cumsum(dpos, axis=1) - 0.5 * dpos).astype(np.float32)
    ref = UO.gaussian_upsample(case["h"], cen, np.float32(0.1), None, case["t_x"], case["t_y"], 0.0, Ty, case["G"])
    r = {"out": UO.ratio(out.detach().cpu().numpy(), ref.out, ref.b_out), "dh": UO.ratio(h.grad.cpu().numpy(), ref.dh, ref.b_dh)}
    print(f"{shape} only h: error / bound out {r['out']:.3f}  dh {r['dh']:.3f}")
    assert all(v <= 1.0 for v in r.values())
    s = sigma.clone().requires_grad_()
    gaussian_upsample(t["h"], dur, Ty, sigma=s).backward(t["G"])
    assert asked[-1] == (False, False, True, True) and s.grad is not None
    assert not gaussian_upsample(t["h"], dur, Ty).requires_grad


def test_autograd_bf16_inputs_get_bf16_gradients(dev):
    """bf16 inputs are cast to fp32 on the way in (the oracle runs on the bf16 values); the output and the gradients are
    rounded to bf16 on the way out: a relative 2^-8 on top of the fp32 bound."""
    shape = (2, 80, 70, 256)
    case = UO.make_case(shape, "sigma", 0.0)
    t = to_dev(case, dev)
    Ty = shape[3]
    h, c, a, g = (t[k].to(torch.bfloat16).requires_grad_() for k in ("h", "centres", "precision", "log_weight"))
    out = gaussian_upsample_at(h, c, a, g, Ty, t["t_x"], t["t_y"])
    out.backward(t["G"].to(torch.bfloat16))
    assert out.dtype == h.grad.dtype == c.grad.dtype == a.grad.dtype == g.grad.dtype == torch.bfloat16
    f = lambda v: v.detach().float().cpu().numpy()                                        # noqa: E731
    ref = UO.gaussian_upsample(f(h), f(c), f(a), f(g), case["t_x"], case["t_y"], 0.0, Ty, f(t["G"].to(torch.bfloat16)))
    x = 2.0 ** -8
    r = {"out": UO.ratio(f(out), ref.out, ref.b_out + x * np.abs(ref.out)), "dh": UO.ratio(f(h.grad), ref.dh, ref.b_dh + x * np.abs(ref.dh)),
         "dc": UO.ratio(f(c.grad), ref.dc, ref.b_dc + x * np.abs(ref.dc)), "da": UO.ratio(f(a.grad), ref.da, ref.b_da + x * np.abs(ref.da)),
         "dg": UO.ratio(f(g.grad), ref.dg, ref.b_dg + x * np.abs(ref.dg))}
    print(f"{shape} bf16: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


def test_t_text_2049_is_outside_the_domain(dev):
    h, c = torch.zeros(1, 1, 2049, device=dev), torch.arange(2049, device=dev, dtype=torch.float32)[None]
    with pytest.raises(_lib.AlignerError) as e:
        gaussian_upsample_at(h, c, 0.1, None, 2100)
    assert e.value.code == _lib.EDOM and "Tx=2049" in str(e.value)
    with pytest.raises(_lib.AlignerError) as e:
        gaussian_upsample(h, torch.ones(1, 2049, device=dev), 2100)
    assert e.value.code == _lib.EDOM
