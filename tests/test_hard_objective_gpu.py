"""The hard half of the objective on the GPU: segment reduction (the length regulator's gradient, per-token means), the
binarization loss with its sparse gradient, the fused alignment_loss(), and the autograd faces of all of them.

Every reference is a float64 restatement in this file.  Tolerances are derived, not measured; u = 2^-24 (fp32 unit
roundoff):
  a sum of n fp32 terms in ANY order is within (n-1) u sum|terms| of the exact sum (to first order); the tests
  allow twice that with n for n-1:  2 n u sum|terms|;
  the mean is that sum divided in fp32 -- one more rounding, u |quotient|;
  the binarization gradient is one fp32 division and a negation: bit-exact."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MIN_LOGP = math.log(1e-12)


@pytest.fixture(scope="module")
def dev():
    import aligner_amd  # noqa: F401
    from aligner_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- float64 restatements

def _segments(dur, Ty):
    d = np.maximum(dur.astype(np.int64), 0)
    e = np.cumsum(d, axis=-1)
    return np.minimum(e - d, Ty), np.minimum(e, Ty)


def _ref_segment_sums(frames, dur):
    """(sum, sum of |.|) in float64 [B,C,Tx] and the segment lengths [B,Tx].  The non-empty segments tile [0, end of the
    last one) without gaps, so np.add.reduceat over their starts sums exactly each of them."""
    B, C, Ty = frames.shape
    Tx = dur.shape[1]
    s, e = _segments(dur, Ty)
    n = e - s
    tot, ab = np.zeros((B, C, Tx)), np.zeros((B, C, Tx))
    for b in range(B):
        nz = np.nonzero(n[b])[0]
        if nz.size:
            f = frames[b, :, :e[b, nz[-1]]].astype(np.float64)
            tot[b][:, nz] = np.add.reduceat(f, s[b, nz], axis=1)
            ab[b][:, nz] = np.add.reduceat(np.abs(f), s[b, nz], axis=1)
    return tot, ab, n


def _check_segment(got, frames, dur, mean):
    tot, ab, n = _ref_segment_sums(frames, dur)
    nn = n[:, None, :].astype(np.float64)
    bound = 2.0 * nn * U * ab
    got = got.astype(np.float64)
    empty = np.broadcast_to(nn == 0, got.shape)
    assert np.all(got[empty] == 0.0), "an empty segment is not exactly 0"
    if mean:
        n1 = np.maximum(nn, 1)
        ref, tol = tot / n1, bound / n1 + U * (np.abs(tot) + bound) / n1     # (the quotient that is rounded is the computed one)
    else:
        ref, tol = tot, bound
    err = np.abs(got - ref)
    bad = err > tol
    print(f"segment {'mean' if mean else 'sum'}: max err {err.max():.3e}, max err/tol "
          f"{(err[~empty] / np.maximum(tol[~empty], 1e-300)).max() if (~empty).any() else 0:.3f}")
    assert not bad.any(), (int(bad.sum()), float(err[bad].max()))


def _durations(kind, B, Tx, Ty, rng, dev):
    if kind == "align":
        import aligner_amd
        g = torch.Generator(device="cpu").manual_seed(int(rng.integers(1 << 30)))
        t_y = rng.integers(max(Ty // 2, min(Tx, Ty)), Ty + 1, size=B)
        t_x = np.array([rng.integers(max(1, min(Tx, t) // 2), min(Tx, t) + 1) for t in t_y])
        t_x[0], t_y[0] = min(Tx, Ty), Ty
        val = torch.randn((B, Tx, Ty), generator=g).to(dev)
        al = aligner_amd.align(val, torch.from_numpy(t_x.astype(np.int32)).to(dev), torch.from_numpy(t_y.astype(np.int32)).to(dev),
                               want_path=False)
        return al.durations.cpu().numpy().astype(np.int32)
    dur = np.zeros((B, Tx), np.int64)
    if kind == "skewed":                                   # one token owns >= 90 % of the frames
        for b in range(B):
            m = min(Tx - 1, Ty // 10)
            others = rng.choice(Tx, size=m + 1, replace=False)
            dur[b, others[1:]] = 1
            dur[b, others[0]] = Ty - m
        assert (dur.max(1) >= 0.9 * Ty).all()
    elif kind == "zeros_neg":
        dur = rng.integers(-3, max(2, 2 * Ty // Tx + 2), size=(B, Tx))
        dur[rng.random((B, Tx)) < 0.3] = 0
    elif kind == "over":                                   # the sum runs past T_mel
        dur = rng.integers(0, 3 * Ty // Tx + 3, size=(B, Tx))
        dur[:, 0] += np.maximum(0, Ty + 1 - np.maximum(dur, 0).sum(1))
        assert (np.maximum(dur, 0).sum(1) > Ty).all()
    elif kind == "under":                                  # frames at the end that no token owns
        dur = rng.integers(0, max(1, Ty // (2 * Tx)) + 1, size=(B, Tx))
        while (dur.sum(1) >= Ty).any():
            dur = dur // 2
        assert (dur.sum(1) < Ty).all()
    return dur.astype(np.int32)


# The last four: three row groups (the last with rows past C) on the two workgroups an utterance gets at B = 2100, so a
# workgroup takes a second group, with one and with four frames per lane; and two rows per wave (512 < T_text <= 1024),
# four and one frames per lane, again with a row past C.
SEG_SHAPES = [(3, 5, 7, 19), (4, 80, 64, 200), (2, 512, 200, 1000), (2, 33, 300, 1023), (1, 16, 2048, 4000),
              (64, 512, 200, 1000), (2100, 33, 5, 19), (2100, 33, 7, 20), (2, 9, 600, 1200), (1, 9, 600, 1201)]
SEG_KINDS = ["align", "skewed", "zeros_neg", "over", "under"]


@pytest.mark.parametrize("kind", SEG_KINDS)
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_segment_reduce(dev, shape, kind):
    import aligner_amd
    B, C, Tx, Ty = shape
    rng = np.random.default_rng(1000 * SEG_SHAPES.index(shape) + SEG_KINDS.index(kind))
    frames = rng.standard_normal((B, C, Ty), dtype=np.float32) * np.float32(3.0) + np.float32(0.5)
    dur = _durations(kind, B, Tx, Ty, rng, dev)
    fd, dd = torch.from_numpy(frames).to(dev), torch.from_numpy(dur).to(dev)
    for mean in (False, True):
        got = aligner_amd.segment_reduce(fd, dd, mean=mean)
        again = aligner_amd.segment_reduce(fd, dd, mean=mean)
        torch.cuda.synchronize()
        assert got.shape == (B, C, Tx) and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ in their bits"
        _check_segment(got.cpu().numpy(), frames, dur, mean)


def test_the_restated_segments_are_the_regulator_s(dev):
    """The segments of the float64 restatement are the ones regulate() expands over (its tok output); the second shape
    has three tokens per thread in the durations' scan."""
    import aligner_amd
    rng = np.random.default_rng(5)
    for B, C, Tx, Ty in [(3, 6, 50, 333), (2, 3, 700, 1500)]:
        dur = _durations("zeros_neg", B, Tx, Ty, rng, dev)
        dd = torch.from_numpy(dur).to(dev)
        _, tok = aligner_amd.regulate(torch.zeros(B, C, Tx, device=dev), dd, Ty)
        s, e = _segments(dur, Ty)
        want = np.full((B, Ty), -1, np.int32)
        for b in range(B):
            for x in range(Tx):
                want[b, s[b, x]:e[b, x]] = x
        assert np.array_equal(tok.cpu().numpy(), want), (B, C, Tx, Ty)


# ---------------------------------------------------------------- regulate / average_by_duration autograd

def test_regulate_autograd(dev):
    import aligner_amd
    rng = np.random.default_rng(11)
    for (B, C, Tx, Ty), kind in [((4, 80, 64, 200), "zeros_neg"), ((2, 33, 300, 1023), "over"), ((3, 5, 7, 19), "under")]:
        dur = _durations(kind, B, Tx, Ty, rng, dev)
        h = rng.standard_normal((B, C, Tx), dtype=np.float32)
        w = rng.standard_normal((B, C, Ty), dtype=np.float32)
        dd, wd = torch.from_numpy(dur).to(dev), torch.from_numpy(w).to(dev)
        # without grad: a plain gather, bit for bit, and no graph
        plain, tok = aligner_amd.regulate(torch.from_numpy(h).to(dev), dd, Ty)
        assert plain.grad_fn is None and not plain.requires_grad
        t = tok.cpu().numpy()
        want = np.where(t[:, None, :] >= 0, np.take_along_axis(h, np.broadcast_to(np.maximum(t, 0)[:, None, :], (B, C, Ty)), 2), 0)
        assert np.array_equal(plain.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
        hd = torch.from_numpy(h).to(dev).requires_grad_(True)
        out, tok2 = aligner_amd.regulate(hd, dd, Ty)
        assert out.requires_grad and not tok2.requires_grad
        assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32)) and torch.equal(tok, tok2)
        (g,) = torch.autograd.grad((out * wd).sum(), hd)
        torch.cuda.synchronize()
        assert g.dtype == torch.float32 and g.shape == hd.shape
        _check_segment(g.cpu().numpy(), w, dur, mean=False)
        with torch.no_grad():
            ng, _ = aligner_amd.regulate(hd, dd, Ty)
        assert ng.grad_fn is None and torch.equal(ng.view(torch.int32), plain.view(torch.int32))
    # bf16 text encodings get a bf16 gradient
    hb = torch.from_numpy(h).to(dev).to(torch.bfloat16).requires_grad_(True)
    out, _ = aligner_amd.regulate(hb, dd, Ty)
    (gb,) = torch.autograd.grad((out * wd).sum(), hb)
    assert gb.dtype == torch.bfloat16
    tot, ab, n = _ref_segment_sums(w, dur)
    err = np.abs(gb.float().cpu().numpy().astype(np.float64) - tot)
    assert np.all(err <= 2.0 * n[:, None, :] * U * ab + 2.0 ** -8 * np.abs(tot))      # + the rounding to bf16


def test_average_by_duration_forward_and_backward(dev):
    import aligner_amd
    rng = np.random.default_rng(12)
    for (B, C, Tx, Ty), kind in [((4, 80, 64, 200), "align"), ((3, 5, 7, 19), "over"), ((2, 9, 40, 333), "zeros_neg"),
                                 ((2, 7, 30, 128), "under")]:
        dur = _durations(kind, B, Tx, Ty, rng, dev)
        frames = rng.standard_normal((B, C, Ty), dtype=np.float32)
        w = rng.standard_normal((B, C, Tx), dtype=np.float32)
        fd = torch.from_numpy(frames).to(dev).requires_grad_(True)
        out = aligner_amd.average_by_duration(fd, torch.from_numpy(dur).to(dev))
        assert out.requires_grad and out.shape == (B, C, Tx)
        (g,) = torch.autograd.grad((out * torch.from_numpy(w).to(dev)).sum(), fd)
        torch.cuda.synchronize()
        _check_segment(out.detach().cpu().numpy(), frames, dur, mean=True)
        # float64 restatement: a dense 0/1 ownership matrix per utterance, autograd through it
        s, e = _segments(dur, Ty)
        own = torch.zeros((B, Tx, Ty), dtype=torch.float64)
        for b in range(B):
            for x in range(Tx):
                own[b, x, s[b, x]:e[b, x]] = 1.0
        f64 = torch.from_numpy(frames).double().requires_grad_(True)
        ref = torch.einsum("bcy,bxy->bcx", f64, own) / own.sum(2).clamp_min(1.0)[:, None, :]
        (gref,) = torch.autograd.grad((ref * torch.from_numpy(w).double()).sum(), f64)
        got, gref = g.cpu().numpy().astype(np.float64), gref.numpy()
        err = np.abs(got - gref)
        print(f"average_by_duration backward: max rel err {(err / np.maximum(np.abs(gref), 1e-300)).max():.3e}")
        assert np.all(got[gref == 0] == 0)
        assert np.all(err <= 2.0 * U * np.abs(gref))          # one term per frame: the segment bound with n = 1
        plain = aligner_amd.average_by_duration(fd.detach(), torch.from_numpy(dur).to(dev))
        assert plain.grad_fn is None and torch.equal(plain, out.detach())


# ---------------------------------------------------------------- binarization loss

def _log_softmax_np(z):
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def _ref_bin(logp, tok, t_y, min_logp):
    """logp: float32 numpy [B,Tx,Ty] (the values the kernel reads).  (nll, sum|terms|, count, live cells [B,Tx,Ty])."""
    B, Tx, Ty = logp.shape
    y = np.arange(Ty)[None, :]
    counting = (tok >= 0) & (tok < Tx)
    if t_y is not None:
        counting &= y < np.asarray(t_y)[:, None]
    tc = np.clip(tok, 0, Tx - 1)
    vals = np.take_along_axis(logp, tc[:, None, :].astype(np.int64), 1)[:, 0, :].astype(np.float64)
    above = vals > min_logp                                  # (False for NaN and -inf)
    terms = np.where(counting, np.where(above, vals, min_logp), 0.0)
    live = np.zeros((B, Tx, Ty), bool)
    bb, yy = np.nonzero(counting & above)
    live[bb, tc[bb, yy], yy] = True
    return -terms.sum(1), np.abs(terms).sum(1), counting.sum(1).astype(np.int32), live


def _bin_case(dev, B, Tx, Ty, dtype, pitched, form, seed):
    """logp with some path cells below the floor and some at -inf, a hard alignment in the asked form."""
    import aligner_amd
    from aligner_amd.softattn import pitched_logp
    rng = np.random.default_rng(seed)
    t_y = rng.integers(max(Ty // 2, min(Tx, Ty)), Ty + 1, size=B).astype(np.int32)
    t_x = np.array([rng.integers(max(1, min(Tx, t) // 2), min(Tx, t) + 1) for t in t_y], np.int32)
    t_x[0], t_y[0] = min(Tx, Ty), Ty
    logp = _log_softmax_np(rng.standard_normal((B, Tx, Ty)) * 3.0)
    lp = torch.from_numpy(logp).to(dev)
    al = aligner_amd.align(lp, torch.from_numpy(t_x).to(dev), torch.from_numpy(t_y).to(dev), want_tok=True,
                           path_dtype=torch.float32)
    tok = al.tok.cpu().numpy().copy()
    assert (tok[0] >= 0).all() and (tok == -1).any() == bool((t_y < Ty).any())
    # spoil some cells ON the path: far below the floor, and log 0
    bb, yy = np.nonzero(tok >= 0)
    pick = rng.permutation(bb.size)[:max(2, bb.size // 7)]
    half = pick.size // 2
    logp[bb[pick[:half]], tok[bb[pick[:half]], yy[pick[:half]]], yy[pick[:half]]] = -50.0
    logp[bb[pick[half:]], tok[bb[pick[half:]], yy[pick[half:]]], yy[pick[half:]]] = -np.inf
    # a t_y shorter than tok's extent; the dense form of the contiguous cases keeps t_y = None (every frame with a token counts)
    t_y_loss = np.maximum(t_y - rng.integers(0, max(2, Ty // 4), size=B), 0).astype(np.int32)
    if form == "dense" and not pitched:
        t_y_loss = None
    if form == "alignment":
        hard = al
    elif form == "dense":
        hard = al.path
    else:                                                   # a raw token-per-frame tensor with entries that do not count
        tok[rng.random(tok.shape) < 0.05] = -1
        tok[rng.random(tok.shape) < 0.05] = Tx
        tok[rng.random(tok.shape) < 0.02] = Tx + 5
        hard = torch.from_numpy(tok.astype(np.int64 if seed % 2 else np.int32)).to(dev)
    src = torch.from_numpy(logp).to(dev).to(dtype)
    if pitched:
        buf = pitched_logp(B, Tx, Ty, dev, dtype)
        assert not buf.is_contiguous()
        buf.copy_(src)
        src = buf
    seen = src.float().cpu().numpy()                         # what the kernel reads (bf16 values, exactly)
    return src, hard, tok, t_y_loss, seen


BIN_CASES = [(3, 7, 19, torch.float32, False), (4, 64, 200, torch.float32, False), (64, 200, 1000, torch.float32, False),
             (8, 500, 4000, torch.bfloat16, False), (4, 64, 200, torch.float32, True), (3, 40, 301, torch.float16, True)]


@pytest.mark.parametrize("form", ["alignment", "dense", "tok"])
@pytest.mark.parametrize("case", BIN_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{str(c[3])[6:]}{'-pitched' if c[4] else ''}")
def test_binarization_loss_and_gradient(dev, case, form):
    import aligner_amd
    from aligner_amd import objective
    B, Tx, Ty, dtype, pitched = case
    src, hard, tok, t_y, seen = _bin_case(dev, B, Tx, Ty, dtype, pitched, form, seed=B * 1000 + Tx + len(form))
    ty_d = None if t_y is None else torch.from_numpy(t_y).to(dev)
    nll_ref, abs_ref, count_ref, live = _ref_bin(seen, tok, t_y, MIN_LOGP)
    assert live.any() and (count_ref > live.sum((1, 2))).any(), "the case holds no cell under the floor"
    nll, count = objective.bin_loss(src, hard.tok if form == "alignment" else hard, ty_d)
    torch.cuda.synchronize()
    assert np.array_equal(count.cpu().numpy(), count_ref)
    err = np.abs(nll.cpu().numpy().astype(np.float64) - nll_ref)
    tol = 2.0 * count_ref * U * abs_ref
    print(f"bin loss: max err {err.max():.3e}, max err/tol {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert np.all(err <= tol)
    N = max(int(count_ref.sum()), 1)
    # reductions, with autograd; upstream gradient 1
    x = src.detach().requires_grad_(True)
    assert x.data_ptr() == src.data_ptr()
    loss = aligner_amd.binarization_loss(x, hard, ty_d)
    none = aligner_amd.binarization_loss(x, hard, ty_d, reduction="none")
    total = aligner_amd.binarization_loss(x, hard, ty_d, reduction="sum")
    assert torch.equal(none.detach(), nll) and torch.equal(total.detach(), nll.sum())
    assert abs(loss.item() - nll_ref.sum() / N) <= (tol.sum() + (B + 1) * U * abs_ref.sum()) / N      # B-term sum, one division
    (g,) = torch.autograd.grad(loss, x)
    torch.cuda.synchronize()
    assert g.dtype == dtype and g.shape == (B, Tx, Ty)
    cell = -(np.float32(1.0) / np.float32(N))
    want = torch.from_numpy(np.where(live, cell, np.float32(0.0)).astype(np.float32)).to(dtype)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(g.cpu().contiguous().view(bits), want.view(bits)), "the gradient is not bit-exact"
    # a second backward gives the same bits; "sum" puts -1 on the live cells
    (g2,) = torch.autograd.grad(aligner_amd.binarization_loss(x, hard, ty_d), x)
    assert torch.equal(g2.contiguous().view(bits), g.contiguous().view(bits))
    (gs,) = torch.autograd.grad(total, x)
    assert torch.equal(gs.float().cpu(), torch.from_numpy(np.where(live, np.float32(-1.0), np.float32(0.0))))


def test_bin_loss_grad_accumulate_through_the_c_abi(dev):
    from aligner_amd import _lib
    lib = _lib.load()
    for (B, Tx, Ty, dtype, pitched) in [(4, 64, 200, torch.float32, True), (3, 7, 19, torch.float32, False),
                                        (2, 50, 403, torch.bfloat16, False)]:
        src, hard, tok, t_y, seen = _bin_case(dev, B, Tx, Ty, dtype, pitched, "tok", seed=77 + Ty)
        _, _, _, live = _ref_bin(seen, tok, t_y, MIN_LOGP)
        rng = np.random.default_rng(Ty)
        base = rng.standard_normal((B, Tx, Ty), dtype=np.float32)
        scale = (rng.random(B, dtype=np.float32) + np.float32(0.25))
        grad = torch.from_numpy(base).to(dev)
        tokd = torch.from_numpy(tok.astype(np.int32)).to(dev)
        tyd, sd = torch.from_numpy(t_y).to(dev), torch.from_numpy(scale).to(dev)
        dt = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16}[dtype]
        _lib.check(lib.aligner_bin_loss_grad_f32(src.data_ptr(), dt, src.stride(1), tokd.data_ptr(), tyd.data_ptr(), MIN_LOGP,
                                                 sd.data_ptr(), grad.data_ptr(), 1, B, Tx, Ty, None))
        torch.cuda.synchronize()
        got = grad.cpu().numpy()
        assert np.array_equal(got.view(np.int32)[~live], base.view(np.int32)[~live]), "a cell off the path was touched"
        want = base.astype(np.float64) - scale.astype(np.float64)[:, None, None]
        assert np.all(np.abs(got.astype(np.float64) - want)[live] <= U * np.abs(want)[live])
        # accumulate = 0 on the same inputs: the whole tensor, +0 off the path
        _lib.check(lib.aligner_bin_loss_grad_f32(src.data_ptr(), dt, src.stride(1), tokd.data_ptr(), tyd.data_ptr(), MIN_LOGP,
                                                 sd.data_ptr(), grad.data_ptr(), 0, B, Tx, Ty, None))
        torch.cuda.synchronize()
        full = np.where(live, -np.broadcast_to(scale[:, None, None], live.shape), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(grad.cpu().numpy().view(np.int32), full.view(np.int32))


# ---------------------------------------------------------------- alignment_loss

@pytest.mark.parametrize("B,Tx,Ty,w", [(4, 64, 200, 1.0), (3, 7, 19, 0.35), (5, 40, 333, 2.5)])
def test_alignment_loss_equals_the_unfused_pair(dev, B, Tx, Ty, w):
    import aligner_amd
    rng = np.random.default_rng(B * Ty)
    t_y = rng.integers(max(Ty // 2, Tx), Ty + 1, size=B).astype(np.int32)
    t_x = np.array([rng.integers(max(1, Tx // 2), Tx + 1) for _ in t_y], np.int32)
    t_x[0], t_y[0] = Tx, Ty
    logp = _log_softmax_np(rng.standard_normal((B, Tx, Ty)) * 2.0)
    txd, tyd = torch.from_numpy(t_x).to(dev), torch.from_numpy(t_y).to(dev)
    hard = aligner_amd.align(torch.from_numpy(logp).to(dev), txd, tyd, want_tok=True, want_path=False)
    tok = hard.tok.cpu().numpy()
    bb, yy = np.nonzero(tok >= 0)
    logp[bb[::11], tok[bb[::11], yy[::11]], yy[::11]] = -60.0          # path cells under the floor: no binarization gradient
    a = torch.from_numpy(logp).to(dev).requires_grad_(True)
    b = torch.from_numpy(logp).to(dev).requires_grad_(True)
    fs_u = aligner_amd.forward_sum_loss(a, txd, tyd)
    bin_u = aligner_amd.binarization_loss(a, hard, tyd)
    (g_fs,) = torch.autograd.grad(fs_u, a, retain_graph=True)
    (g_u,) = torch.autograd.grad(fs_u + w * bin_u, a)
    total, fs_part, bin_part = aligner_amd.alignment_loss(b, txd, tyd, hard, bin_weight=w)
    assert total.requires_grad and not fs_part.requires_grad and not bin_part.requires_grad
    (g,) = torch.autograd.grad(total, b)
    torch.cuda.synchronize()
    assert torch.equal(fs_part, fs_u.detach()) and torch.equal(bin_part, bin_u.detach())
    assert torch.equal(total.detach(), (fs_u + w * bin_u).detach())       # the same fp32 operations: not even the add's rounding differs
    _, _, count, live = _ref_bin(logp, tok, t_y, MIN_LOGP)
    N = max(int(count.sum()), 1)
    live_t = torch.from_numpy(live).to(dev)
    assert live.any() and torch.equal(g[~live_t].view(torch.int32), g_fs[~live_t].view(torch.int32)), "off the path"
    err = (g.double() - g_u.double()).abs()[live_t]
    tol = 4 * U * (g_fs.double().abs()[live_t] + w / N)
    print(f"alignment_loss on-path gradient: max err/tol {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all())


def test_alignment_loss_trains_the_encoder(dev):
    import aligner_amd
    g = torch.Generator().manual_seed(3)
    params = aligner_amd.AlignmentEncoderParams.random(64, 80, 80, dev, seed=2)
    weights = [t for w, b in params.key_proj + params.query_proj for t in (w, b)]
    for t in weights:
        t.requires_grad_(True)
    text = torch.randn(2, 64, 40, generator=g).to(dev)
    mel = torch.randn(2, 80, 172, generator=g).to(dev)
    t_x = torch.tensor([40, 25], dtype=torch.int32, device=dev)
    t_y = torch.tensor([172, 120], dtype=torch.int32, device=dev)
    logp, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x)
    hard = aligner_amd.align(logp.detach(), t_x, t_y, want_tok=True, want_path=False)
    total, fs_part, bin_part = aligner_amd.alignment_loss(logp, t_x, t_y, hard, bin_weight=0.5)
    total.backward()
    torch.cuda.synchronize()
    assert math.isfinite(total.item()) and math.isfinite(fs_part.item()) and math.isfinite(bin_part.item())
    for t in weights:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


# ---------------------------------------------------------------- canary bands and streams

SENTINEL = np.float32(-7.25e33).view(np.int32).item()


def _banded(dev, numel, pad=1024):
    """An int32 view of `numel` 4-byte elements between two sentinel-filled bands."""
    buf = torch.full((pad + numel + pad,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[pad:pad + numel]


def _bands_intact(buf, numel, pad=1024):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + numel:] == SENTINEL).all())


def test_canary_bands(dev):
    from aligner_amd import _lib
    lib = _lib.load()
    for (B, C, Tx, Ty) in [(3, 5, 7, 19), (2, 33, 300, 1023), (2, 37, 64, 200), (1, 3, 2048, 4000)]:
        rng = np.random.default_rng(Ty)
        frames = torch.from_numpy(rng.standard_normal((B, C, Ty), dtype=np.float32)).to(dev)
        for kind in ("over", "under"):
            dur = torch.from_numpy(_durations(kind, B, Tx, Ty, rng, dev)).to(dev)
            for mean in (0, 1):
                buf, out = _banded(dev, B * C * Tx)
                _lib.check(lib.aligner_segment_reduce_f32(frames.data_ptr(), dur.data_ptr(), out.data_ptr(), B, C, Tx, Ty, mean, None))
                torch.cuda.synchronize()
                assert _bands_intact(buf, B * C * Tx), (B, C, Tx, Ty, kind, mean)
                assert not bool((out == SENTINEL).any()), "an output element was not written"
    for (B, Tx, Ty, dtype, pitched) in [(3, 7, 19, torch.float32, False), (4, 64, 200, torch.float32, True),
                                        (2, 50, 403, torch.bfloat16, False)]:
        src, hard, tok, t_y, seen = _bin_case(dev, B, Tx, Ty, dtype, pitched, "tok", seed=Ty)
        _, _, _, live = _ref_bin(seen, tok, t_y, MIN_LOGP)
        dt = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16}[dtype]
        tokd, tyd = torch.from_numpy(tok.astype(np.int32)).to(dev), torch.from_numpy(t_y).to(dev)
        nbuf, nll = _banded(dev, B)
        cbuf, cnt = _banded(dev, B)
        _lib.check(lib.aligner_bin_loss(src.data_ptr(), dt, src.stride(1), tokd.data_ptr(), tyd.data_ptr(), MIN_LOGP,
                                        nll.data_ptr(), cnt.data_ptr(), B, Tx, Ty, None))
        scale = torch.ones(B, device=dev)
        gbuf, grad = _banded(dev, B * Tx * Ty)
        _lib.check(lib.aligner_bin_loss_grad_f32(src.data_ptr(), dt, src.stride(1), tokd.data_ptr(), tyd.data_ptr(), MIN_LOGP,
                                                 scale.data_ptr(), grad.data_ptr(), 0, B, Tx, Ty, None))
        torch.cuda.synchronize()
        assert _bands_intact(nbuf, B) and _bands_intact(cbuf, B) and _bands_intact(gbuf, B * Tx * Ty)
        assert not bool((nll == SENTINEL).any()) and not bool((cnt == SENTINEL).any())
        assert not bool((grad == SENTINEL).any()), "accumulate = 0 left an element unwritten"
        abuf, acc = _banded(dev, B * Tx * Ty)
        acc.view(torch.float32).fill_(1.0)
        _lib.check(lib.aligner_bin_loss_grad_f32(src.data_ptr(), dt, src.stride(1), tokd.data_ptr(), tyd.data_ptr(), MIN_LOGP,
                                                 scale.data_ptr(), acc.data_ptr(), 1, B, Tx, Ty, None))
        torch.cuda.synchronize()
        assert _bands_intact(abuf, B * Tx * Ty)
        assert np.array_equal(acc.view(torch.float32).cpu().numpy().reshape(B, Tx, Ty), np.where(live, np.float32(0.0), np.float32(1.0)))


def test_on_a_side_stream(dev):
    import aligner_amd
    rng = np.random.default_rng(21)
    B, C, Tx, Ty = 4, 80, 64, 200
    frames = torch.from_numpy(rng.standard_normal((B, C, Ty), dtype=np.float32)).to(dev)
    dur = torch.from_numpy(_durations("zeros_neg", B, Tx, Ty, rng, dev)).to(dev)
    src, hard, tok, t_y, _ = _bin_case(dev, B, Tx, Ty, torch.float32, False, "tok", seed=9)
    tyd = torch.from_numpy(t_y).to(dev)
    t_x = torch.full((B,), Tx // 2, dtype=torch.int32, device=dev)       # (<= every shortened t_y)

    def run():
        x = src.detach().clone().requires_grad_(True)
        s = aligner_amd.segment_reduce(frames, dur)
        m = aligner_amd.average_by_duration(frames, dur)
        loss = aligner_amd.binarization_loss(x, hard, tyd)
        (g,) = torch.autograd.grad(loss, x)
        z = src.detach().clone().requires_grad_(True)
        total, _, _ = aligner_amd.alignment_loss(z, t_x, tyd, hard.clamp(-1, Tx - 1))
        (gz,) = torch.autograd.grad(total, z)
        return s, m, loss.detach(), g, total.detach(), gz

    ref = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    for r, s in zip(ref, got):
        assert torch.equal(r, s)
