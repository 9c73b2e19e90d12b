"""The weight-gradient kernel of the conv encoders (csrc/conv_bwd.hip) where one workgroup walks MANY 32-frame chunks.

conv_bwd_w_kernel splits the reduction over (utterance, 32-frame chunk) units among `nsplit` workgroups per output tile.  With
one unit per split the loop body runs once: the register prefetch of the next chunk, the step from one utterance to the next
inside a split, the uneven division U sp / nsplit and accumulation over more than 32 frames are then never executed.  This
module holds

 * CONV_SPLIT_CASES, the shapes the GPU tests below run, and a CPU guard that they really do all of that (the split count
   is recovered from the host-side workspace size, the unit ranges recomputed as the kernel computes them);
 * an exact check on small integers: every product and partial sum is an integer below 2^24, so fp32 arithmetic in ANY
   order is exact and grad_w / grad_b / the masked cotangent / grad_x must equal the float64 reference bit for bit -- one
   dropped, doubled or stale term among B T = 57 600 is caught, which no tolerance promises;
 * the float64 check on random data at the project's bound REL = 1e-4 of each tensor's max, not loosened for the long sums.

The float64 reference is written out as matrix products (no [B, Cin K, T] unfold, fast on the CPU at the full sizes); a CPU
test ties it to torch autograd through F.conv1d."""
import pytest
import torch
import torch.nn.functional as F

from test_frontend_backward_gpu import REL, _rel_err

gpu = pytest.mark.gpu

SMALL_CASES = [
    (5, 80, 160, 333, 3),       # 55 units over 32 splits: uneven, splits begin mid-utterance, T % 32 != 0
    (7, 512, 1024, 45, 3),      # 96 tiles: 6 splits of 14 units (two chunks an utterance, the second 13 frames)
    (9, 33, 70, 129, 5),        # odd channel counts, k = 5, a last chunk of one frame
    (11, 160, 256, 100, 5),
    (6, 1024, 80, 200, 1),
    (23, 512, 1024, 20, 3),     # one chunk an utterance, 6 splits: each walks 3-4 utterances
    (3, 512, 1024, 530, 3),     # 51 units over 6 splits: 8-9 chunks a split
]
# the five encoder layers at the size DESIGN.md 4.2 times
FULL_CASES = [
    (64, 512, 1024, 200, 3),
    (64, 1024, 80, 200, 1),
    (64, 80, 160, 900, 3),
    (64, 160, 80, 900, 1),
    (64, 80, 80, 900, 1),
]
CONV_SPLIT_CASES = SMALL_CASES + FULL_CASES
CHUNK, TILE = 32, 128          # conv_bwd.hip: CW_CHUNK, CW_TILE
INT_MAX = 3                    # integer inputs are uniform in {-3 .. 3}


def _align_up(n, a):
    return (n + a - 1) // a * a


def _nsplit(lib, B, Ci, Co, T, K):
    """The kernel's split count, from the workspace size (host code): align_up(ns Cout Cin K 4, 256) + align_up(ns Cout 4,
    256) is strictly monotone in ns, so exactly one ns in 1..32 gives it."""
    got = lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, K)
    hits = [ns for ns in range(1, 33) if _align_up(ns * Co * Ci * K * 4, 256) + _align_up(ns * Co * 4, 256) == got]
    assert len(hits) == 1, (B, Ci, Co, T, K, got, hits)
    return hits[0]


def _splits(B, T, ns):
    """[u0, u1) of every split, as conv_bwd_w_kernel computes them; unit u = utterance u // NTt, chunk u % NTt."""
    ntt = (T + CHUNK - 1) // CHUNK
    U = B * ntt
    return ntt, U, [(U * sp // ns, U * (sp + 1) // ns) for sp in range(ns)]


def test_split_cases_cover_the_chunk_loop(built_lib):
    long_run = uneven = mid_utt = three_utts = capped = tile_bound = False
    for B, Ci, Co, T, K in CONV_SPLIT_CASES:
        ns = _nsplit(built_lib, B, Ci, Co, T, K)
        ntt, U, sp = _splits(B, T, ns)
        assert sp[0][0] == 0 and sp[-1][1] == U and all(a[1] == b[0] for a, b in zip(sp, sp[1:]))
        long_run |= U / ns >= 8
        uneven |= U % ns != 0
        mid_utt |= T % CHUNK != 0 and any(u0 % ntt != 0 for u0, _ in sp[1:])
        three_utts |= any(u1 > u0 and (u1 - 1) // ntt - u0 // ntt + 1 >= 3 for u0, u1 in sp)
        capped |= ns == 32
        tile_bound |= ns < 32 and ns < U
    assert long_run, "no case with >= 8 chunks a split"
    assert uneven, "no case with units % nsplit != 0"
    assert mid_utt, "no split begins in the middle of an utterance whose last chunk is partial"
    assert three_utts, "no split spans three utterances"
    assert capped, "no case at the cap of 32 splits"
    assert tile_bound, "no case whose split count is set by the tile count"


# ---- float64 reference, as matrix products ----

def _ref_conv_backward(x, w, y, gy, relu):
    """(dYpre, dX, dW, db) of y = act(conv1d(x, w, b, padding=K//2)) in float64 on x's device; the ReLU mask is the
    kernel's rule, torch.relu's: 0 where y <= 0 (y = +0, -0 and y < 0 all mask), dY elsewhere (a NaN y passes it)."""
    x, w, gy = x.double(), w.double(), gy.double()
    B, Ci, T = x.shape
    Co, _, K = w.shape
    hk = K // 2
    gyp = torch.where(y <= 0, torch.zeros_like(gy), gy) if relu else gy
    xp = F.pad(x, (hk, hk))
    gp = F.pad(gyp, (hk, hk))
    a = gyp.permute(1, 0, 2).reshape(Co, B * T)
    gw = torch.stack([a @ xp[:, :, k:k + T].permute(0, 2, 1).reshape(B * T, Ci) for k in range(K)], dim=2)
    gx = sum(torch.matmul(w[:, :, k].t(), gp[:, :, 2 * hk - k:2 * hk - k + T]) for k in range(K))
    return gyp, gx, gw, a.sum(1)


@pytest.mark.parametrize("B,Ci,Co,T,K,relu", [(2, 5, 7, 37, 3, True), (3, 4, 6, 33, 5, False), (2, 9, 3, 8, 1, True),
                                              (1, 3, 2, 2, 5, True)])
def test_reference_matches_float64_autograd(B, Ci, Co, T, K, relu):
    g = torch.Generator().manual_seed(B + Ci + T)
    x = torch.randn(B, Ci, T, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(Co, Ci, K, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(Co, generator=g, dtype=torch.float64).requires_grad_()
    gy = torch.randn(B, Co, T, generator=g, dtype=torch.float64)
    pre = F.conv1d(x, w, b, padding=K // 2)
    y = torch.relu(pre) if relu else pre
    y.backward(gy)
    _, gx, gw, gb = _ref_conv_backward(x.detach(), w.detach(), y.detach(), gy, relu)
    for got, want in ((gx, x.grad), (gw, w.grad), (gb, b.grad)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


# ---- exact on integers ----

def _int_inputs(B, Ci, Co, T, K, seed):
    """x, w, y, dY with integer values in {-3..3}; y has exact zeros, and every other zero of it is a negative zero."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randint(-INT_MAX, INT_MAX + 1, s, generator=g).float()  # noqa: E731
    x, w, y, gy = r(B, Ci, T), r(Co, Ci, K), r(B, Co, T), r(B, Co, T)
    z = (y == 0).flatten().nonzero().flatten()[::2]
    y.view(-1)[z] = -0.0
    return x, w, y, gy


def _assert_exact_in_fp32(ref, what):
    """The precondition of the exact check: integer-valued, magnitudes below 2^24, the cast to fp32 loses nothing."""
    for name, t in zip(("dYpre", "dX", "dW", "db"), ref):
        assert torch.equal(t, t.round()), (what, name)
        assert t.abs().max().item() < 2 ** 24, (what, name, t.abs().max().item())
        assert torch.equal(t.float().double(), t), (what, name)


@pytest.mark.parametrize("B,Ci,Co,T,K", CONV_SPLIT_CASES)
def test_integer_sums_stay_below_2_to_24(B, Ci, Co, T, K):
    """Every partial sum of every output, in any order, is bounded by (number of terms) x max|a| max|b|: below 2^24 for every
    case of the list, so no fp32 addition of the kernels can round.  (dW: B T terms; db: B T; dX: Cout K.)"""
    assert B * T * INT_MAX * INT_MAX < 2 ** 24
    assert B * T * INT_MAX < 2 ** 24
    assert Co * K * INT_MAX * INT_MAX < 2 ** 24


@pytest.mark.parametrize("B,Ci,Co,T,K", SMALL_CASES[:5])
@pytest.mark.parametrize("relu", [True, False])
def test_integer_reference_is_exact_in_fp32(B, Ci, Co, T, K, relu):
    x, w, y, gy = _int_inputs(B, Ci, Co, T, K, seed=B + T)
    assert (y == 0).any() and torch.signbit(y[y == 0]).any() and not torch.signbit(y[y == 0]).all()
    _assert_exact_in_fp32(_ref_conv_backward(x, w, y, gy, relu), (B, Ci, Co, T, K))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


CANARY = -12345.0


def _guarded(dev, n, guard):
    """A flat fp32 buffer of n elements with `guard` canary elements on either side: (whole buffer, the n-element view)."""
    buf = torch.full((n + 2 * guard,), CANARY, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n]


def _guards_intact(buf, n, guard):
    return bool((buf[:guard] == CANARY).all().item()) and bool((buf[guard + n:] == CANARY).all().item())


def _raw_backward_weight(dev, x, y, gy, relu, Co, K, want_w, want_b):
    """aligner_conv1d_backward_weight_f32 through the ctypes table, every output in a canary-guarded buffer (the kernel's
    128-row x 32-frame tiles hang over Cout and T: a store past either lands in the next row or in a guard), the workspace
    sized by aligner_conv1d_backward_workspace_bytes and guarded too.  Returns (dYpre, dW or None, db or None)."""
    from aligner_amd import _lib
    lib = _lib.load()
    B, Ci, T = x.shape
    guard = TILE * (T + CHUNK)
    gyp_buf, gyp = _guarded(dev, B * Co * T, guard)
    gw_buf, gw = _guarded(dev, Co * Ci * K, guard)
    gb_buf, gb = _guarded(dev, Co, guard)
    nws = lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, K)
    assert nws > 0 and nws % 4 == 0
    ws_buf, ws = _guarded(dev, nws // 4, 4096)
    need = want_w or want_b
    _lib.check(lib.aligner_conv1d_backward_weight_f32(
        x.data_ptr(), y.data_ptr() if relu else None, gy.data_ptr(), gyp.data_ptr(), gw.data_ptr() if want_w else None,
        gb.data_ptr() if want_b else None, ws.data_ptr() if need else None, nws if need else 0, B, Ci, Co, T, K, int(relu),
        torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert _guards_intact(gyp_buf, B * Co * T, guard), "dYpre: store outside [B,Cout,T]"
    assert _guards_intact(gw_buf, Co * Ci * K, guard) and _guards_intact(gb_buf, Co, guard), "dW / db: store outside"
    assert _guards_intact(ws_buf, nws // 4, 4096), "store past the workspace"
    if not want_w:
        assert bool((gw == CANARY).all().item())
    if not want_b:
        assert bool((gb == CANARY).all().item())
    return gyp.view(B, Co, T), gw.view(Co, Ci, K) if want_w else None, gb if want_b else None


@gpu
@pytest.mark.parametrize("B,Ci,Co,T,K", CONV_SPLIT_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_conv_backward_exact_on_integers(dev, B, Ci, Co, T, K, relu):
    """torch.equal, zero tolerance, for dW, db, the masked cotangent and dX.  dX is the forward GEMM on the transposed weight
    image with bf16 hi/lo splits: integers up to 3 are exact in bf16 (the low halves are zero), the products exact, the
    accumulators fp32 -- exact in every form of that GEMM, so equality is asserted for it as well."""
    import aligner_amd
    x, w, y, gy = _int_inputs(B, Ci, Co, T, K, seed=B + T)
    ref = _ref_conv_backward(x, w, y, gy, relu)            # float64, on the CPU, before the GPU is involved
    _assert_exact_in_fp32(ref, (B, Ci, Co, T, K))
    rgyp, rgx, rgw, rgb = (t.float() for t in ref)
    xd, wd, yd, gyd = x.to(dev), w.to(dev), y.to(dev), gy.to(dev)
    assert torch.equal(torch.signbit(yd).cpu(), torch.signbit(y))      # the negative zeros arrive
    gx, gw, gb = aligner_amd.conv1d_backward(xd, wd, yd, gyd, relu)
    torch.cuda.synchronize()
    bad = lambda got, want: int((got.cpu() != want).sum())  # noqa: E731
    assert torch.equal(gw.cpu(), rgw), ("dW", bad(gw, rgw))
    assert torch.equal(gb.cpu(), rgb), ("db", bad(gb, rgb))
    assert torch.equal(gx.cpu(), rgx), ("dX", bad(gx, rgx))
    # one output at a time
    _, gw1, gb1 = aligner_amd.conv1d_backward(xd, wd, yd, gyd, relu, need_x=False, need_b=False)
    assert gb1 is None and torch.equal(gw1.cpu(), rgw)
    _, gw2, gb2 = aligner_amd.conv1d_backward(xd, wd, yd, gyd, relu, need_x=False, need_w=False)
    assert gw2 is None and torch.equal(gb2.cpu(), rgb)
    gx3, gw3, gb3 = aligner_amd.conv1d_backward(xd, wd, yd, gyd, relu, need_w=False, need_b=False)   # relu: the mask kernel
    assert gw3 is None and gb3 is None and torch.equal(gx3.cpu(), rgx)
    # the masked cotangent itself, from the weight kernel (with each of dW / db, and both) and from the mask kernel
    for want_w, want_b in ((True, True), (True, False), (False, True), (False, False)):
        gyp, gwr, gbr = _raw_backward_weight(dev, xd, yd, gyd, relu, Co, K, want_w, want_b)
        assert torch.equal(gyp.cpu(), rgyp), ("dYpre", want_w, want_b, bad(gyp, rgyp))
        assert gwr is None or torch.equal(gwr.cpu(), rgw)
        assert gbr is None or torch.equal(gbr.cpu(), rgb)


# ---- float64 on random data ----

@gpu
@pytest.mark.parametrize("B,Ci,Co,T,K", CONV_SPLIT_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_conv_backward_long_splits_match_float64(dev, B, Ci, Co, T, K, relu):
    """The inputs, error measure and bound of test_conv1d_backward_matches_float64_autograd at shapes where a split sums many
    chunks.  REL is not loosened: sequential fp32 accumulation of n = B T = 57 600 random-sign terms has a rounding error of
    about sqrt(n) 2^-24 = 1.4e-5 of the sum's rms, the maximum over a tensor a few times that, and max|ref| is several rms.
    The figures are printed before they are asserted (pytest -rP shows them)."""
    import aligner_amd
    g = torch.Generator().manual_seed(B * 7 + Ci + K)
    x = torch.randn(B, Ci, T, generator=g).to(dev)
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).to(dev)
    b = torch.randn(Co, generator=g).to(dev)
    gy = torch.randn(B, Co, T, generator=g).to(dev)
    y = aligner_amd.conv1d(x, w, b, relu)
    gx, gw, gb = aligner_amd.conv1d_backward(x, w, y, gy, relu)
    _, rx, rw, rb = _ref_conv_backward(x, w, y, gy, relu)
    torch.cuda.synchronize()
    errs = (_rel_err(gx, rx), _rel_err(gw, rw), _rel_err(gb, rb))
    print(f"conv backward {(B, Ci, Co, T, K)} relu={int(relu)}: rel err dX {errs[0]:.2e} dW {errs[1]:.2e} db {errs[2]:.2e}")
    assert max(errs) <= REL, errs
    gx2, gw2, gb2 = aligner_amd.conv1d_backward(x, w, y, gy, relu)
    torch.cuda.synchronize()
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    # partial requests: the same bits
    gxa, gwa, gba = aligner_amd.conv1d_backward(x, w, y, gy, relu, need_w=False, need_b=False)
    _, gwb, gbb = aligner_amd.conv1d_backward(x, w, y, gy, relu, need_x=False)
    torch.cuda.synchronize()
    assert gwa is None and gba is None and torch.equal(gxa, gx) and torch.equal(gwb, gw) and torch.equal(gbb, gb)
