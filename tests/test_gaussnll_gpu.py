"""gaussian_nll() / gaussian_nll_loss() on the GPU against the float64 oracle (tests/gaussnll_oracle.py).

The bounds are derived, not tuned.  With u = 2^-24, a value that is a sum of n fp32 terms in any order has a forward error
of at most (n + 8) u times the sum of the terms' magnitudes; the 8 covers the per-term roundings (the subtraction, expf,
the products, the scale):

    dz   8 u |d w|            elementwise
    dm   (n_x + 8) u A_m      A_m = sum |d w| over the token's frames
    ds   (n_x + 8) u A_s      A_s = n_x + w sum d^2
    nll  (C count + 8) u S    S = sum ( 1/2 ln 2pi + |s| + 1/2 d^2 w )

each times |scale[b]| where a scale is given.  Every test prints the observed ratio to its bound.  The nll bound is loose
at large n, so dropped or doubled frames are caught by planted outliers (test_planted_outliers_move_nll_by_the_oracles_amount).

Shapes sit at the edges of the kernel's structure: one element; the scalar form with C no multiple of the rows per pass;
the vector form (T_mel % 4 == 0) and one frame past it; segments longer than several runs; a large one; the largest T_text;
then the launch's other paths -- several rows per wave, several row groups per workgroup -- at the sizes where it takes them
itself and, on small shapes, through the library's testing switches.
Every shape runs with durations that hold skipped tokens, a negative entry, a sum below T_mel in one utterance and above it
in another, and t_y below the sum in one utterance (gaussnll_oracle.edge_durations)."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import gausslogp_oracle as GO
import gaussnll_oracle as NO
from aligner_amd import _lib, gaussian_align, gaussian_nll, gaussian_nll_loss, regulate

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 1), (3, 7, 31, 130), (2, 80, 70, 256), (2, 80, 70, 257), (2, 16, 3, 1030), (2, 192, 300, 1000),
          (1, 5, 2048, 2100)]
# Shapes at which the launch itself takes its other paths (csrc/gaussnll.hip: gauss_nll_rows_per_wave, launch_gauss_nll):
# four rows per wave with C no multiple of 16 (scalar form); two rows per wave with C no multiple of 8 (vector form); more
# row groups than workgroups per utterance, so that a workgroup takes a second group on cleared accumulators.
LAUNCH_SHAPES = [(128, 250, 31, 70), (128, 130, 300, 72), (64, 260, 600, 70)]
# (shape, flip): a batch of one utterance runs with either kind of durations
CASES = [(s, f) for s in SHAPES + LAUNCH_SHAPES for f in ((0, 1) if s[0] == 1 else (0,))]
# The same paths on small shapes, through the library's testing switches: (shape, rows per wave, workgroups per utterance).
# C = 37: with four rows a wave the last wave with work holds one row and three repeats, with two rows one and one; the
# groups (3 and 5) outnumber the workgroups, so every workgroup makes a second pass.  (…, 300, …): four rows asked, two given.
PINNED = [((2, 37, 31, 130), 4, 2), ((2, 37, 31, 132), 4, 2), ((2, 37, 31, 130), 2, 2), ((2, 37, 31, 132), 2, 1),
          ((2, 37, 300, 132), 4, 2), ((3, 7, 31, 130), 4, 0), ((2, 80, 70, 256), 1, 3)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def make_case(shape, flip=0, with_scale=False):
    """Inputs of gaussian_logp's test family with the edge durations, and the oracle's answer.  Cached and shared: never
    modified."""
    B, C, Tx, Ty = shape
    rng = np.random.default_rng(1000003 * C + 1009 * Tx + Ty + flip)
    z, m, s = GO.draw_inputs(rng, B, C, Tx, Ty)
    dur, t_y = NO.edge_durations(rng, B, Tx, Ty, flip)
    scale = None
    if with_scale:
        scale = rng.standard_normal(B).astype(np.float32)
        scale[0] = -abs(scale[0]) - 0.5
        if B > 1:
            scale[1] = 0.0
    return dict(z=z, mean=m, logstd=s, dur=dur, t_y=t_y, scale=scale, ref=NO.gaussian_nll(z, m, s, dur, t_y, scale))


def to_dev(case, dev):
    return {k: torch.from_numpy(case[k]).to(dev) for k in ("z", "mean", "logstd", "dur", "t_y")}


def bits(t):
    return t.contiguous().view(torch.int32)


def ratio(got, want, bound):
    """max |got - want| / bound over the elements with a nonzero bound; where the bound is 0 the two must be equal."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    zero = bound == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def check_grads(ref, dz, dm, ds, scale_abs, tag, extra=0.0):
    """dz, dm, ds (numpy) against the oracle within the derived bounds; extra: a further relative error of the values
    themselves (a reduced-precision output dtype)."""
    sa = np.ones(len(ref.nll)) if scale_abs is None else np.asarray(scale_abs, np.float64)
    sa3 = sa[:, None, None]
    n3 = ref.n[:, None, :]
    r_z = ratio(dz, ref.dz, 8 * U * sa3 * ref.absdw + extra * np.abs(ref.dz))
    r_m = ratio(dm, ref.dm, (n3 + 8) * U * sa3 * ref.A_m + extra * np.abs(ref.dm))
    r_s = ratio(ds, ref.ds, (n3 + 8) * U * sa3 * ref.A_s + extra * np.abs(ref.ds))
    print(f"{tag}: error / bound: dz {r_z:.3f}  dm {r_m:.3f}  ds {r_s:.3f}")
    assert r_z <= 1.0 and r_m <= 1.0 and r_s <= 1.0, (tag, r_z, r_m, r_s)


def check_nll(ref, nll, count, C, tag):
    r_n = ratio(nll, ref.nll, (C * ref.count + 8) * U * ref.S_nll)
    print(f"{tag}: error / bound: nll {r_n:.3f}")
    assert np.array_equal(np.asarray(count), ref.count), tag
    assert r_n <= 1.0, (tag, r_n)


@contextlib.contextmanager
def pinned(rows, grid):
    """The launch's rows per wave and workgroups per utterance pinned for the calls inside (0: its own choice)."""
    lib = _lib.load()
    assert lib.aligner_debug_set_option(b"gaussnll_rows", rows) == 0 and lib.aligner_debug_set_option(b"gaussnll_grid", grid) == 0
    try:
        yield
    finally:
        lib.aligner_debug_set_option(b"gaussnll_rows", 0)
        lib.aligner_debug_set_option(b"gaussnll_grid", 0)


@pytest.mark.parametrize("shape,flip", CASES)
def test_loss_and_gradients_against_the_oracle(dev, shape, flip):
    check_case(dev, shape, flip)


@pytest.mark.parametrize("shape,rows,grid", PINNED)
def test_rows_per_wave_and_passes_against_the_oracle(dev, shape, rows, grid):
    """Every check of the test above with the launch pinned, and: the rows per wave and the number of passes change
    which wave sums a row, not the order in which it is summed -- the same bits as the launch's own choice."""
    free = check_case(dev, shape, 0)
    with pinned(rows, grid):
        held = check_case(dev, shape, 0, f" rows {rows} grid {grid}")
    for a, b in zip(free, held):
        assert torch.equal(bits(a), bits(b))


def check_case(dev, shape, flip, note=""):
    case = make_case(shape, flip)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    nll, count, dz, dm, ds = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"], t["t_y"], want_grad=True)
    assert nll.dtype == torch.float32 and count.dtype == torch.int32 and dz.shape == (B, C, Ty) and dm.shape == ds.shape == (B, C, Tx)
    tag = f"{shape} flip {flip}{note}"
    check_nll(ref, nll.cpu().numpy(), count.cpu().numpy(), C, tag)
    check_grads(ref, dz.cpu().numpy(), dm.cpu().numpy(), ds.cpu().numpy(), None, tag)
    # bit checks: +0.0 where nothing counts
    off = torch.from_numpy(~ref.counts).to(dev)[:, None, :].expand(B, C, Ty)
    empty = torch.from_numpy(ref.n == 0).to(dev)[:, None, :].expand(B, C, Tx)
    assert not bits(dz)[off].any() and not bits(dm)[empty].any() and not bits(ds)[empty].any()
    # two runs: the same bits in every output; the loss-only form: the same nll bits
    again = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"], t["t_y"], want_grad=True)
    for a, b in zip((nll, count, dz, dm, ds), again):
        assert torch.equal(bits(a), bits(b))
    nll0, count0 = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"], t["t_y"])
    assert torch.equal(bits(nll0), bits(nll)) and torch.equal(count0, count)
    # without t_y: the full extent
    full = NO.gaussian_nll(case["z"], case["mean"], case["logstd"], case["dur"])
    nll1, count1 = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"])
    check_nll(full, nll1.cpu().numpy(), count1.cpu().numpy(), C, tag + " no t_y")
    return nll, count, dz, dm, ds


@pytest.mark.parametrize("shape,flip", CASES)
def test_planted_outliers_move_nll_by_the_oracles_amount(dev, shape, flip):
    """1000 added to one channel of one frame's z, at frame 0, the last counting frame, either side of every multiple of
    64 (the scalar form's run; every fourth is a multiple of the vector form's 256) and the first frame past t_y, in
    every utterance at once.  A counting frame moves nll by the oracle's amount, 1/2 w ((d + 1000)^2 - d^2), within the
    bound; any other frame does not move nll at all."""
    case = make_case(shape, flip)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    base, _ = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"], t["t_y"])
    frames = []
    for b in range(B):
        ys = {0, max(int(ref.count[b]) - 1, 0), int(case["t_y"][b])}
        for e in range(64, Ty, 64):
            ys.update((e - 1, e))
        frames.append(sorted(y for y in ys if y < Ty))
    worst, moved = 0.0, 0
    for i in range(max(len(f) for f in frames)):
        zz = t["z"].clone()
        want, S, picks = ref.nll.copy(), ref.S_nll.copy(), []
        for b in range(B):
            y = frames[b][min(i, len(frames[b]) - 1)]
            c = (y + b) % C
            zz[b, c, y] += 1000.0
            picks.append(y)
            if ref.counts[b, y]:
                x = int(np.searchsorted(np.cumsum(np.maximum(case["dur"][b], 0)), y, side="right"))
                w = math.exp(-2.0 * float(case["logstd"][b, c, x]))
                z1 = float(zz[b, c, y].item())
                d0, d1 = float(case["z"][b, c, y]) - float(case["mean"][b, c, x]), z1 - float(case["mean"][b, c, x])
                want[b] += 0.5 * w * (d1 * d1 - d0 * d0)
                S[b] += 0.5 * w * (d1 * d1 - d0 * d0)
        got, _ = gaussian_nll(zz, t["mean"], t["logstd"], t["dur"], t["t_y"])
        got_np = got.cpu().numpy()
        for b in range(B):
            if ref.counts[b, picks[b]]:
                r = abs(float(got_np[b]) - want[b]) / ((C * ref.count[b] + 8) * U * S[b])
                worst = max(worst, r)
                moved += 1
                assert r <= 1.0, (shape, b, picks[b], r)
                assert abs(want[b] - ref.nll[b]) > 4 * (C * ref.count[b] + 8) * U * S[b]      # the outlier shows above the bound
            else:
                assert torch.equal(bits(got[b]), bits(base[b])), (shape, b, picks[b])
    print(f"{shape} flip {flip}: {moved} counting outliers, worst error / bound {worst:.3f}")


def test_t_text_2049_is_outside_the_domain(dev):
    z, m = torch.zeros(1, 1, 2100, device=dev), torch.zeros(1, 1, 2049, device=dev)
    with pytest.raises(_lib.AlignerError) as e:
        gaussian_nll(z, m, m, torch.ones(1, 2049, dtype=torch.int32, device=dev))
    assert e.value.code == _lib.EDOM and "Tx=2049" in str(e.value)


@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256)])
def test_nothing_counts(dev, shape):
    """All-zero durations, and t_y = 0: nll = 0, count = 0, every gradient +0.0 bit for bit."""
    case = make_case(shape)
    t = to_dev(case, dev)
    B = shape[0]
    for dur, ty in ((torch.zeros_like(t["dur"]), t["t_y"]), (t["dur"], torch.zeros_like(t["t_y"])),
                    (torch.full_like(t["dur"], -2), None)):
        out = gaussian_nll(t["z"], t["mean"], t["logstd"], dur, ty, want_grad=True,
                           scale=torch.full((B,), -1.5, device=dev))
        for o in out:
            assert not bits(o).any()
    # empty shapes: zeros without a launch
    nll, count, dz, dm, ds = gaussian_nll(t["z"][:, :, :0], t["mean"], t["logstd"], t["dur"], want_grad=True)
    assert not nll.any() and not count.any() and dz.shape == (B, shape[1], 0) and not dm.any() and not ds.any()
    nll, count = gaussian_nll(t["z"][:0], t["mean"][:0], t["logstd"][:0], t["dur"][:0])
    assert nll.shape == (0,) and count.shape == (0,)


@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256), (2, 16, 3, 1030)])
def test_scale_vector(dev, shape):
    """A random scale per utterance, a negative one and 0 included."""
    case = make_case(shape, 0, True)
    ref, t = case["ref"], to_dev(case, dev)
    scale = torch.from_numpy(case["scale"]).to(dev)
    nll, count, dz, dm, ds = gaussian_nll(t["z"], t["mean"], t["logstd"], t["dur"], t["t_y"], want_grad=True, scale=scale)
    check_nll(ref, nll.cpu().numpy(), count.cpu().numpy(), shape[1], f"{shape} scaled")           # (the loss is not scaled)
    check_grads(ref, dz.cpu().numpy(), dm.cpu().numpy(), ds.cpu().numpy(), np.abs(case["scale"]), f"{shape} scaled")
    empty = torch.from_numpy(ref.n == 0).to(dev)[:, None, :].expand_as(dm)
    assert not bits(dm)[empty].any() and not bits(ds)[empty].any()
    assert not dz[1].any() and not dm[1].any() and not ds[1].any()                               # scale 0


def _reduction_factor(ref, C, reduction):
    return 1.0 / max(C * int(ref.count.sum()), 1) if reduction == "mean" else 1.0


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256)])
def test_autograd_against_the_oracle(dev, shape, reduction):
    case = make_case(shape)
    ref, t = case["ref"], to_dev(case, dev)
    B, C = shape[:2]
    z, m, s = (t[k].clone().requires_grad_() for k in ("z", "mean", "logstd"))
    loss = gaussian_nll_loss(z, m, s, t["dur"], t["t_y"], reduction=reduction)
    f = _reduction_factor(ref, C, reduction)
    if reduction == "none":
        assert loss.shape == (B,)
        check_nll(ref, loss.detach().cpu().numpy(), ref.count, C, f"{shape} none")
        weights = torch.tensor([1.0, -2.0, 0.5][:B], device=dev)
        (loss * weights).sum().backward()
        up = weights.cpu().numpy().astype(np.float64)
    else:
        want = ref.nll.sum() * f
        bound = ((C * ref.count + 8) * U * ref.S_nll).sum() * f + 2 * U * abs(want)              # + the reduction's own roundings
        assert abs(loss.item() - want) <= bound
        loss.backward()
        up = np.full(B, f)
    scaled = NO.gaussian_nll(case["z"], case["mean"], case["logstd"], case["dur"], case["t_y"], up)
    check_grads(scaled, z.grad.cpu().numpy(), m.grad.cpu().numpy(), s.grad.cpu().numpy(), np.abs(up), f"{shape} {reduction}")


def test_autograd_only_mean_requires_grad(dev):
    shape = (3, 7, 31, 130)
    case = make_case(shape)
    ref, t = case["ref"], to_dev(case, dev)
    m = t["mean"].clone().requires_grad_()
    z, s = t["z"].clone(), t["logstd"].clone()
    gaussian_nll_loss(z, m, s, t["dur"], t["t_y"], reduction="sum").backward()
    assert z.grad is None and s.grad is None
    r = ratio(m.grad.cpu().numpy(), ref.dm, (ref.n[:, None, :] + 8) * U * ref.A_m)
    print(f"{shape} only mean: error / bound dm {r:.3f}")
    assert r <= 1.0
    # a duration tensor inside an Alignment is taken as it is; nothing requires grad: no graph
    from aligner_amd import Alignment
    out = gaussian_nll_loss(z, t["mean"], s, Alignment(None, None, t["dur"]), t["t_y"], reduction="sum")
    assert not out.requires_grad and torch.equal(out, gaussian_nll(z, t["mean"], s, t["dur"], t["t_y"])[0].sum())


def test_autograd_bf16_inputs_get_bf16_gradients(dev):
    """bf16 inputs are cast to fp32 on the way in (the oracle runs on the bf16 values) and the fp32 gradients are rounded
    to bf16 on the way out: round to nearest at 8 significand bits (7 stored and the hidden one), a relative 2^-8 on top
    of the fp32 bound."""
    shape = (2, 80, 70, 256)
    case = make_case(shape)
    t = to_dev(case, dev)
    z, m, s = (t[k].to(torch.bfloat16).requires_grad_() for k in ("z", "mean", "logstd"))
    gaussian_nll_loss(z, m, s, t["dur"], t["t_y"], reduction="sum").backward()
    assert z.grad.dtype == m.grad.dtype == s.grad.dtype == torch.bfloat16
    ref = NO.gaussian_nll(z.detach().float().cpu().numpy(), m.detach().float().cpu().numpy(), s.detach().float().cpu().numpy(),
                          case["dur"], case["t_y"])
    check_grads(ref, z.grad.float().cpu().numpy(), m.grad.float().cpu().numpy(), s.grad.float().cpu().numpy(), None,
                f"{shape} bf16", extra=2.0 ** -8)


@pytest.mark.parametrize("shape", [(3, 7, 31, 130), (2, 80, 70, 256)])
def test_autograd_equals_the_composed_gpu_path(dev, shape):
    """What a caller composes from regulate() and torch elementwise ops, and .backward(): the two are interchangeable --
    each is within the fp32 bound of the oracle, so they differ by at most twice the bound."""
    case = make_case(shape)
    ref, t = case["ref"], to_dev(case, dev)
    B, C, Tx, Ty = shape
    z1, m1, s1 = (t[k].clone().requires_grad_() for k in ("z", "mean", "logstd"))
    fused = gaussian_nll_loss(z1, m1, s1, t["dur"], t["t_y"], reduction="sum")
    fused.backward()
    z2, m2, s2 = (t[k].clone().requires_grad_() for k in ("z", "mean", "logstd"))
    m_y, tok = regulate(m2, t["dur"], Ty)
    s_y, _ = regulate(s2, t["dur"], Ty)
    counts = ((tok >= 0) & (torch.arange(Ty, device=dev)[None, :] < t["t_y"][:, None])).unsqueeze(1)
    assert np.array_equal(counts[:, 0].cpu().numpy(), ref.counts)
    term = 0.5 * math.log(2 * math.pi) + s_y + 0.5 * (z2 - m_y) ** 2 * torch.exp(-2 * s_y)
    composed = (term * counts).sum()
    composed.backward()
    nll_bound = ((C * ref.count + 8) * U * ref.S_nll).sum()
    print(f"{shape}: fused {fused.item():.6f} composed {composed.item():.6f}, |difference| / (2 bound) "
          f"{abs(fused.item() - composed.item()) / (2 * nll_bound):.3f}")
    assert abs(fused.item() - composed.item()) <= 2 * nll_bound
    n3 = ref.n[:, None, :]
    for name, a, b, bound in (("dz", z1.grad, z2.grad, 8 * U * ref.absdw), ("dm", m1.grad, m2.grad, (n3 + 8) * U * ref.A_m),
                              ("ds", s1.grad, s2.grad, (n3 + 8) * U * ref.A_s)):
        r = ratio(a.cpu().numpy(), b.double().cpu().numpy(), 2 * bound)
        print(f"{shape}: {name} |fused - composed| / (2 bound) {r:.3f}")
        assert r <= 1.0, name


@pytest.mark.parametrize("n", [0, 2])
def test_end_to_end_on_the_planted_cases(dev, n):
    """gaussian_align() -> gaussian_nll_loss(): the search returns the planted durations (tests/test_gausslogp_host.py
    checks that on the CPU for these seeds) and the loss on them matches the oracle on the planted durations."""
    case = GO.planted_case(n)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("z", "mean", "logstd", "t_x", "t_y")}
    res = gaussian_align(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"], want_path=False)
    assert np.array_equal(res.durations.cpu().numpy(), case["durations"])
    ref = NO.gaussian_nll(case["z"], case["mean"], case["logstd"], case["durations"], case["t_y"])
    assert np.array_equal(ref.count, case["t_y"])
    C = case["z"].shape[1]
    z, m, s = (t[k].clone().requires_grad_() for k in ("z", "mean", "logstd"))
    loss = gaussian_nll_loss(z, m, s, res, t["t_y"])
    f = 1.0 / (C * int(ref.count.sum()))
    want = ref.nll.sum() * f
    bound = ((C * ref.count + 8) * U * ref.S_nll).sum() * f + 2 * U * abs(want)
    print(f"planted case {n}: loss {loss.item():.6f}, oracle {want:.6f}, error / bound {abs(loss.item() - want) / bound:.3f}")
    assert abs(loss.item() - want) <= bound
    loss.backward()
    scaled = NO.gaussian_nll(case["z"], case["mean"], case["logstd"], case["durations"], case["t_y"], np.full(2, f))
    check_grads(scaled, z.grad.cpu().numpy(), m.grad.cpu().numpy(), s.grad.cpu().numpy(), np.full(2, f), f"planted case {n}")
