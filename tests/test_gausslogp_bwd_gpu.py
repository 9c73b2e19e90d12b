"""gaussian_logp_backward(), gaussian_logp(differentiable=True) and gaussian_forward_sum_loss() on the GPU against the
float64 oracle (tests/gausslogp_bwd_oracle.py, the direct (z - m) form).

The bound: per output element |got - oracle| <= 2^-14 S, S the magnitude of what the expanded sums add up on the raw
inputs over the valid cells (the oracle returns S_dz, S_dm, S_ds).  2^-14 is the forward's constant for the forward's
reason: three split bf16 products at ~2^-16 relative each -- a numpy simulation of the kernels' products stays below
2 * 2^-16 S on these input families (tests/test_gausslogp_bwd_host.py) -- and the rest for fp32 accumulation order and
exp in fp32.  Frames >= t_y, tokens >= t_x and empty utterances are +0.0 exactly.

Shapes sit at the edges of the kernels' structure: channels that are no multiple of 8, of the 32-channel tile or of the
three-tile channel group; the 16-token k-step and the 32-token tile; the 32-frame strip / chunk, T_mel % 4 != 0 (the
scalar tail of the row kernel's loads), and the frame split of the row kernel, frame_splits() below: SPLIT_ONE names
shapes swept by one workgroup per token tile, SPLIT_MANY shapes whose partial sums are added in split order."""
import functools

import numpy as np
import pytest
import torch

import gausslogp_bwd_oracle as BO
import gausslogp_oracle as GO
from aligner_amd import (forward_sum, forward_sum_loss, gaussian_forward_sum_loss, gaussian_logp, gaussian_logp_backward)
from aligner_amd.softattn import pitched_logp

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -14


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def frame_splits(B, C, Tx, Ty):
    """csrc/gausslogp_bwd.hip, gb_plan(): how many waves share the frame sweep of one token tile (the shape alone)."""
    ct = (C + 31) // 32
    waves = B * ((Tx + 31) // 32) * ((ct + 2) // 3)
    ns = (Ty + 31) // 32
    want = max(1, min(1536 // waves, (ns + 3) // 4))
    per = (ns + want - 1) // want
    return (ns + per - 1) // per


# a covering subset of C x T_text x T_mel (B = 3): every listed size of every axis at least once
EDGE_SHAPES = [(1, 1, 1), (7, 31, 15), (8, 32, 17), (17, 33, 33), (80, 65, 130), (192, 225, 257), (256, 33, 130),
               (8, 1024, 33), (7, 1, 1030), (80, 65, 1030)]
SPLIT_ONE = [(3, 7, 31, 15), (3, 17, 33, 33), (3, 8, 1024, 33)]
SPLIT_MANY = [(3, 80, 65, 130), (3, 192, 225, 257), (3, 80, 65, 1030), (2, 17, 65, 130), (2, 17, 65, 1030)]


def test_the_named_shapes_split_as_named():
    assert all(frame_splits(*s) == 1 for s in SPLIT_ONE)
    assert [frame_splits(*s) for s in SPLIT_MANY] == [2, 3, 9, 2, 9]


@functools.lru_cache(maxsize=None)
def make_case(B, C, Tx, Ty, lo=0.5, hi=1.5, mid_lengths=False):
    """Inputs of the forward tests' family with ragged lengths and a dense cotangent.  Cached and shared: never modified.
    B = 3: the first utterance at full size, one with t_x = 1, one with t_x = 0; mid_lengths: the others drawn in between."""
    rng = np.random.default_rng(200000 * C + 1000 * Tx + Ty + int(100 * lo) + 7 * B)
    ty = rng.integers(max(1, Ty // 2), Ty + 1, B).astype(np.int32)
    if mid_lengths:
        tx = rng.integers(1, Tx + 1, B).astype(np.int32)
    else:
        tx = np.array([Tx, 1, 0] + [Tx] * B, np.int32)[:B]
    tx[0], ty[0] = Tx, Ty
    z, m, s = GO.draw_inputs(rng, B, C, Tx, Ty, lo, hi, t_x=tx)
    return dict(z=z, mean=m, logstd=s, t_x=tx, t_y=ty, G=BO.dense_cotangent(rng, B, Tx, Ty))


def on(dev, case, *names):
    return [torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in names]


def run(case, dev, G=None, lengths=True, **kw):
    z, m, s, tx, ty = on(dev, case, "z", "mean", "logstd", "t_x", "t_y")
    if G is None:
        G = on(dev, case, "G")[0]
    return gaussian_logp_backward(G, z, m, s, tx if lengths else None, ty if lengths else None, **kw)


def check(case, got, G, tag, lengths=True, grad_scale=None):
    """got = (dz, dm, ds) tensors (None skipped) against the oracle on the cotangent G (numpy)."""
    o = BO.backward(G, case["z"], case["mean"], case["logstd"], case["t_x"] if lengths else None,
                    case["t_y"] if lengths else None, grad_scale)
    B, C, Ty = case["z"].shape
    Tx = case["mean"].shape[2]
    valid = BO.valid_cells(B, Tx, Ty, case["t_x"] if lengths else None, case["t_y"] if lengths else None)
    live = dict(dz=np.broadcast_to(valid.any(1)[:, None, :], (B, C, Ty)), dm=np.broadcast_to(valid.any(2)[:, None, :], (B, C, Tx)))
    live["ds"] = live["dm"]
    figures = []
    for name, t in zip(("dz", "dm", "ds"), got):
        if t is None:
            continue
        assert t.dtype == torch.float32 and tuple(t.shape) == o[name].shape and t.is_contiguous()
        a = t.cpu().numpy()
        assert np.isfinite(a).all(), (tag, name)
        err, S = np.abs(a.astype(np.float64) - o[name]), o["S_" + name]
        pos = S > 0
        figures.append(f"{name} {float((err[pos] / S[pos]).max()) * 2.0 ** 16 if pos.any() else 0.0:.3f}")
        assert (err <= BOUND * S).all(), (tag, name, float((err[pos] / S[pos]).max()) / BOUND if pos.any() else float(err.max()))
        masked = np.ascontiguousarray(a[~live[name]])
        assert not masked.view(np.uint32).any(), f"{tag}: {name} outside the lengths is not +0.0"
    print(f"{tag}: max |err| / S = {', '.join(figures)} (* 2^-16)")


def forward_sum_cotangent(case, dev):
    """d loss / d value from the project's forward_sum (plain form) on the oracle's values; utterances without an
    alignment (t_x > t_y) are given a zero cotangent."""
    value = GO.gaussian_logp(case["z"], case["mean"], case["logstd"], case["t_x"], case["t_y"])[0].astype(np.float32)
    tx, ty = on(dev, case, "t_x", "t_y")
    G = forward_sum(torch.from_numpy(value).to(dev), tx, ty)[1]
    return torch.nan_to_num(G, nan=0.0, posinf=0.0, neginf=0.0).contiguous()


@pytest.mark.parametrize("kind", ["dense", "forward_sum"])
@pytest.mark.parametrize("C,Tx,Ty", EDGE_SHAPES)
def test_gradients_at_the_structural_edges(dev, C, Tx, Ty, kind):
    case = make_case(3, C, Tx, Ty)
    G = on(dev, case, "G")[0] if kind == "dense" else forward_sum_cotangent(case, dev)
    check(case, run(case, dev, G=G), G.cpu().numpy(), f"[3,{C},{Tx},{Ty}] {kind} G, {frame_splits(3, C, Tx, Ty)} split(s)")


@pytest.mark.parametrize("B,C,Tx,Ty", [(2, 17, 65, 130), (2, 17, 65, 1030), (3, 80, 33, 17)])
def test_exact_on_small_integers(dev, B, C, Tx, Ty):
    """z, m in {-3..3}, s = 0 (w = 1), G in {-2..2}: every product is exact in bf16 and every partial sum an integer far
    below 2^24, so the result is the oracle's bit for bit -- one dropped, doubled or stale term fails.  [2,17,65,130]
    and [2,17,65,1030] are SPLIT_MANY shapes, [3,80,33,17] is swept by one workgroup per token tile."""
    rng = np.random.default_rng(B * 1000 + Ty)
    case = dict(z=rng.integers(-3, 4, (B, C, Ty)).astype(np.float32), mean=rng.integers(-3, 4, (B, C, Tx)).astype(np.float32),
                logstd=np.zeros((B, C, Tx), np.float32), G=rng.integers(-2, 3, (B, Tx, Ty)).astype(np.float32),
                t_x=np.array([Tx, Tx - 3, 1][:B], np.int32), t_y=np.array([Ty - 1, Ty, 5][:B], np.int32))
    o = BO.backward(case["G"], case["z"], case["mean"], case["logstd"], case["t_x"], case["t_y"])
    for name, t in zip(("dz", "dm", "ds"), run(case, dev)):
        assert torch.equal(t.cpu().double(), torch.from_numpy(o[name])), name
    # and without lengths
    o = BO.backward(case["G"], case["z"], case["mean"], case["logstd"])
    for name, t in zip(("dz", "dm", "ds"), run(case, dev, lengths=False)):
        assert torch.equal(t.cpu().double(), torch.from_numpy(o[name])), name


def test_small_sigma_family(dev):
    """sigma ~ U(0.05, 2): weights up to 400, where the expanded terms cancel hardest."""
    case = make_case(3, 16, 70, 200, 0.05, 2.0)
    check(case, run(case, dev), case["G"], "small sigma [3,16,70,200]")


@pytest.mark.parametrize("B,C,Tx,Ty", [(8, 80, 200, 130), (5, 80, 100, 257)])
def test_lengths_in_between_and_both_block_maps(dev, B, C, Tx, Ty):
    """Lengths strictly inside the extents, in a batch that is a multiple of 8 (an utterance's waves share an XCD) and in
    one that is not; then no lengths at all."""
    case = make_case(B, C, Tx, Ty, mid_lengths=True)
    check(case, run(case, dev), case["G"], f"[{B},{C},{Tx},{Ty}]")
    check(case, run(case, dev, lengths=False), case["G"], f"[{B},{C},{Tx},{Ty}] no lengths", lengths=False)


@pytest.mark.parametrize("C,Tx,Ty", [(80, 65, 130), (17, 33, 33), (7, 1, 1030)])
def test_poisoned_masked_cells_and_pitched_cotangent(dev, C, Tx, Ty):
    """NaN in grad_value outside the lengths and in the pad columns of a pitched buffer reaches no output; a contiguous
    and a pitched cotangent of the same values give the same bits."""
    case = make_case(3, C, Tx, Ty)
    clean = run(case, dev)
    valid = torch.from_numpy(BO.valid_cells(3, Tx, Ty, case["t_x"], case["t_y"])).to(dev)
    G = on(dev, case, "G")[0]
    poisoned = torch.where(valid, G, torch.full_like(G, float("nan")))
    assert torch.isnan(poisoned).any()
    for a, b in zip(clean, run(case, dev, G=poisoned)):
        assert torch.isfinite(b).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    buf = pitched_logp(3, Tx, Ty, dev, torch.float32)
    ld = buf.stride(1) if Tx > 1 else buf.stride(0)
    assert ld > Ty
    torch.as_strided(buf, (3, Tx, ld), (Tx * ld, ld, 1)).fill_(float("nan"))
    buf.copy_(G)
    for a, b in zip(clean, run(case, dev, G=buf)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    buf.copy_(poisoned)
    for a, b in zip(clean, run(case, dev, G=buf)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_grad_scale(dev):
    case = make_case(3, 80, 65, 130)
    scale = np.array([0.5, -3.0, 2.0], np.float32)
    got = run(case, dev, grad_scale=torch.from_numpy(scale).to(dev))
    check(case, got, case["G"], "grad_scale [3,80,65,130]", grad_scale=scale)
    pre = run(case, dev, G=on(dev, case, "G")[0] * torch.from_numpy(scale).to(dev).view(-1, 1, 1))
    for a, b in zip(got, pre):                              # the same fp32 products, scaled before or while they are read
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a zero scale: the utterance's rows are +0.0
    zero = run(case, dev, grad_scale=torch.tensor([0.0, 1.0, 1.0], device=dev))
    one = run(case, dev)
    for a, b in zip(zero, one):
        assert not a[0].view(torch.int32).any() and torch.equal(a[1:].view(torch.int32), b[1:].view(torch.int32))


def test_every_subset_of_outputs_has_the_same_bits(dev):
    case = make_case(3, 80, 65, 130)
    full = run(case, dev)
    for mask in range(1, 7):
        need = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
        got = run(case, dev, need_z=need[0], need_mean=need[1], need_logstd=need[2])
        for want, t, n in zip(full, got, need):
            assert (t is None) == (not n)
            if n:
                assert torch.equal(want.view(torch.int32), t.view(torch.int32))


def test_determinism_and_side_stream(dev):
    case = make_case(5, 80, 100, 257, mid_lengths=True)
    a = run(case, dev)
    b = run(case, dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c = run(case, dev)
    side.synchronize()
    for x, y, w in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), w.view(torch.int32))


def test_autograd_through_gaussian_logp(dev):
    case = make_case(3, 80, 65, 130)
    z, m, s, tx, ty, G = on(dev, case, "z", "mean", "logstd", "t_x", "t_y", "G")
    zr, mr, sr = (t.clone().requires_grad_() for t in (z, m, s))
    value = gaussian_logp(zr, mr, sr, tx, ty, differentiable=True)
    assert value.requires_grad and torch.equal(value.detach(), gaussian_logp(z, m, s, tx, ty))
    (value * G).sum().backward()                            # a random linear functional: its cotangent is G
    check(case, (zr.grad, mr.grad, sr.grad), case["G"], "autograd [3,80,65,130]")
    # needs_input_grad: a detached z gets no gradient tensor, the others the same bits
    m2, s2 = (t.clone().requires_grad_() for t in (m, s))
    (gaussian_logp(z, m2, s2, tx, ty, differentiable=True) * G).sum().backward()
    assert z.grad is None and torch.equal(m2.grad, mr.grad) and torch.equal(s2.grad, sr.grad)
    # gradients in each input's dtype
    z16, m64 = z.bfloat16().requires_grad_(), m.double().requires_grad_()
    (gaussian_logp(z16, m64, s, tx, ty, differentiable=True) * G).sum().backward()
    assert z16.grad.dtype == torch.bfloat16 and m64.grad.dtype == torch.float64
    assert torch.equal(m64.grad.float(), gaussian_logp_backward(G, z16, m64, s, tx, ty)[1])
    # the default stays out of autograd; differentiable=True without a tensor that requires grad as well
    assert not gaussian_logp(zr, mr, sr, tx, ty).requires_grad
    assert not gaussian_logp(z, m, s, tx, ty, differentiable=True).requires_grad


@functools.lru_cache(maxsize=None)
def planted0():
    return GO.planted_case(0)


def loss_case(dev, t_x=None):
    case = dict(planted0())
    if t_x is not None:
        case["t_x"] = np.asarray(t_x, np.int32)
    z, m, s, tx, ty = on(dev, case, "z", "mean", "logstd", "t_x", "t_y")
    return case, [t.clone().requires_grad_() for t in (z, m, s)], tx, ty


@pytest.mark.parametrize("options", [dict(), dict(reduction="none"), dict(length_normalize=True, reduction="sum")])
def test_gaussian_forward_sum_loss(dev, options):
    """[2,80,70,200], planted case 0: the loss is forward_sum_loss on gaussian_logp's tensor (plain form), the
    gradients are the oracle's for the G that forward_sum returned, scaled per utterance by what the options imply."""
    case, (z, m, s), tx, ty = loss_case(dev)
    loss = gaussian_forward_sum_loss(z, m, s, tx, ty, **options)
    value = gaussian_logp(z, m, s, tx, ty)
    want = forward_sum_loss(value, tx, ty, blank_logprob=None, **options)
    assert torch.equal(loss, want)
    G = forward_sum(value, tx, ty)[1]
    if options.get("reduction") == "none":
        cot = torch.tensor([0.75, -1.5], device=dev)
        (loss * cot).sum().backward()
        scale = cot.cpu().numpy()
    else:
        loss.backward()
        scale = np.full(2, 0.5, np.float32) if not options else 1.0 / case["t_x"].astype(np.float32)
    check(case, (z.grad, m.grad, s.grad), G.cpu().numpy(), f"gaussian_forward_sum_loss {options}", grad_scale=scale)


def test_gaussian_forward_sum_loss_zero_infinity(dev):
    """One utterance with t_x > t_y: with zero_infinity its loss is 0 and its gradients are zero, not NaN."""
    case, (z, m, s), tx, ty = loss_case(dev)
    ty = torch.tensor([200, 30], dtype=torch.int32, device=dev)          # t_x = [70, 52]
    assert torch.isinf(gaussian_forward_sum_loss(z, m, s, tx, ty, reduction="none")[1])
    loss = gaussian_forward_sum_loss(z, m, s, tx, ty, reduction="none", zero_infinity=True)
    assert torch.isfinite(loss).all() and loss[1] == 0
    loss.sum().backward()
    for g in (z.grad, m.grad, s.grad):
        assert torch.isfinite(g).all() and not g[1].any() and g[0].any()
    # the feasible utterance's gradients are the ones it gets on its own
    z1, m1, s1 = (t.detach()[:1].clone().requires_grad_() for t in (z, m, s))
    gaussian_forward_sum_loss(z1, m1, s1, tx[:1], ty[:1], reduction="sum").backward()
    case1 = {k: v[:1] for k, v in case.items() if k in ("z", "mean", "logstd", "t_x", "t_y")}
    G1 = forward_sum(gaussian_logp(z1, m1, s1, tx[:1], ty[:1]), tx[:1], ty[:1])[1]
    check(case1, (z.grad[:1].contiguous(), m.grad[:1].contiguous(), s.grad[:1].contiguous()), G1.cpu().numpy(), "zero_infinity, utterance 0")
