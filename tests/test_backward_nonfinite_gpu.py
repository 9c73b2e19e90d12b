"""Non-finite values in the backward passes of the front end (csrc/conv_bwd.hip, the input gradient through
csrc/convgemm.hip, csrc/softattn_bwd.hip): where a NaN or an infinity has to appear in a gradient, and where it must not.

Conv backward.  The oracle is the padded matrix-product reference of test_frontend_backward_splits.py in float64, with IEEE
semantics throughout: a 0 of the padding times NaN is NaN, as in the kernels' zero-filled halo.  The ReLU mask is
torch.relu's: dYpre = 0 where y <= 0, dY elsewhere, so a NaN y passes its cotangent.  One value is planted at a time (NaN,
+inf, -inf in x, w, dY; NaN in y; NaN in y and dY at the same cell, which is what a gradient scaler's overflow check has to
see) at an interior frame, frame 0, frame T - 1 and the last channel, always in utterance 1.  dYpre, dW and db must have the
reference's class (finite, NaN, +inf, -inf) in every element, dX must be non-finite exactly where the reference is (the
split-product forward turns +-inf into NaN: include/aligner_amd.h), dYpre must equal the reference bit for bit, and the
finite elements of dW, db and dX are held to REL of test_frontend_backward_gpu.py -- a planted value does not change the
arithmetic of the elements it does not reach.  With finite weights the other utterances' dX and dYpre keep the clean run's
bits.

Soft-attention backward.  NaN where nothing may read it (keys rows i >= t_x; dlogp, dsoft and the prior on those rows;
everything of an utterance with t_x = 0) changes no bit of any output.  One NaN in a valid cell of utterance 1 (k, q, dlogp,
dsoft, the prior, or a negative prior, whose log is NaN) reaches every cell the float64 autograd reference gives a NaN, no
other cell of that utterance, nothing of the other utterances, and, for every plant but the keys', no other frame's dQ.
The one rule the code forces: dK of a masked row i >= t_x is exactly 0, where the reference's 0 x NaN gives
NaN for a NaN in q."""
import functools

import pytest
import torch

from test_frontend_backward_gpu import REL, _case, _ref_grads
from test_frontend_backward_splits import _raw_backward_weight, _ref_conv_backward

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cls(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, per element."""
    t = t.double()
    return torch.isnan(t).long() + 2 * (t == INF).long() + 3 * (t == -INF).long()


# ---- conv backward ----
CONV_SHAPES = [(2, 33, 70, 129, 5), (3, 80, 160, 70, 3), (2, 160, 80, 40, 1)]
WHERE = ("interior", "frame 0", "frame T-1", "last channel")
PLANTS = [(t, v) for t in ("x", "w", "gy") for v in (NAN, INF, -INF)] + [("y", NAN), ("y+gy", NAN)]


def _at(name, shape, where):
    """The planted cell: of the [Cout,Cin,K] weight, or of a [B,C,T] activation (utterance 1)."""
    if name == "w":
        Co, Ci, K = shape
        return {"interior": (Co // 2, Ci // 2, K // 2), "frame 0": (0, 0, 0), "frame T-1": (Co // 3, Ci // 3, K - 1),
                "last channel": (Co - 1, Ci - 1, K // 2)}[where]
    _, C, T = shape
    return {"interior": (1, C // 2, T // 2), "frame 0": (1, 1, 0), "frame T-1": (1, C // 3, T - 1),
            "last channel": (1, C - 1, T // 3)}[where]


@functools.lru_cache(maxsize=None)
def _conv_clean(shape, relu):
    """Inputs of one (shape, relu) on the GPU, y from the package's own forward, and the clean run.  Never modified."""
    import aligner_amd
    B, Ci, Co, T, K = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 7 + Ci + K)
    x = torch.randn(B, Ci, T, generator=g).to(dev)
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).to(dev)
    b = torch.randn(Co, generator=g).to(dev)
    gy = torch.randn(B, Co, T, generator=g).to(dev)
    y = aligner_amd.conv1d(x, w, b, relu)
    out = _conv_run(x, w, y, gy, relu)
    assert all(torch.isfinite(t).all() for t in out) and torch.isfinite(y).all()
    if relu:
        assert (y == 0).any() and (y > 0).any()
    return (x, w, y, gy), out


def _conv_run(x, w, y, gy, relu):
    """(dYpre, dX, dW, db): dYpre, dW, db straight through the C ABI (guarded buffers), dX (and dW, db again, the same
    bits) through conv1d_backward."""
    import aligner_amd
    Co, _, K = w.shape
    gyp, gw_raw, gb_raw = _raw_backward_weight(x.device, x, y, gy, relu, Co, K, True, True)
    gyp, gw_raw, gb_raw = gyp.clone(), gw_raw.clone(), gb_raw.clone()
    gx, gw, gb = aligner_amd.conv1d_backward(x, w, y if relu else None, gy, relu)
    torch.cuda.synchronize()
    assert _bits_equal(gw, gw_raw) and _bits_equal(gb, gb_raw)
    return gyp, gx, gw, gb


# y is read with ReLU only
CONV_RUNS = [(s, r, t, v) for s in CONV_SHAPES for r in (True, False) for t, v in PLANTS if r or not t.startswith("y")]


@pytest.mark.parametrize("shape,relu,target,value", CONV_RUNS)
def test_conv_backward_nonfinite(dev, shape, relu, target, value):
    (x0, w0, y0, gy0), clean = _conv_clean(shape, relu)
    B = shape[0]
    others = [b for b in range(B) if b != 1]
    for where in WHERE:
        t = {"x": x0.clone(), "w": w0.clone(), "y": y0.clone(), "gy": gy0.clone()}
        for name in target.split("+"):
            t[name][_at(name, tuple(t[name].shape), where)] = value
        x, w, y, gy = t["x"], t["w"], t["y"], t["gy"]
        ref = _ref_conv_backward(x, w, y, gy, relu)                      # (dYpre, dX, dW, db), float64
        got = _conv_run(x, w, y, gy, relu)
        line, fails = [], []
        for name, g, r in zip(("dYpre", "dX", "dW", "db"), got, ref):
            bad_g, bad_r = ~torch.isfinite(g), ~torch.isfinite(r)
            lost, stray = int((bad_r & ~bad_g).sum()), int((bad_g & ~bad_r).sum())
            line.append(f"{name} {int(bad_r.sum())} expected {int(bad_g.sum())} found {lost} lost {stray} stray")
            if lost or stray:
                fails.append((name, "non-finite cells", lost, stray))
            if name != "dX":
                n = int((_cls(g) != _cls(r)).sum())
                if n:
                    fails.append((name, "class differs", n))
            fin = ~bad_g & ~bad_r
            if name == "dYpre":
                n = int((g.double()[fin] != r[fin]).sum())
                if n:
                    fails.append((name, "finite cells differ from the reference", n))
            elif fin.any():
                err = (g.double()[fin] - r[fin]).abs().max().item() / max(r[fin].abs().max().item(), 1e-300)
                line.append(f"rel err {err:.1e}")
                if err > REL:
                    fails.append((name, "finite cells", err))
        print(f"conv backward {shape} relu={int(relu)} {target}={value} at {where}: " + "; ".join(line))
        assert not fails, (where, fails)
        if target == "w":                                               # the weight kernel does not read w
            assert all(_bits_equal(g, c) for g, c in zip((got[0], got[2], got[3]), (clean[0], clean[2], clean[3])))
        else:                                                           # finite w: a clean utterance keeps its bits
            assert _bits_equal(got[0][others], clean[0][others]), "dYpre of a clean utterance changed"
            assert _bits_equal(got[1][others], clean[1][others]), "dX of a clean utterance changed"


def test_conv_nan_output_passes_its_cotangent_like_torch_relu(dev):
    """The rule itself against torch: relu(nan).backward(g) gives g; y = +0, -0 and y < 0 give 0."""
    from aligner_amd import conv1d_backward
    y = torch.tensor([NAN, 0.0, -0.0, -1.0, 2.0, INF, -INF]).requires_grad_()
    g = torch.tensor([1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5])
    torch.relu(y).backward(g)
    assert y.grad.tolist() == [1.5, 0.0, 0.0, 0.0, 5.5, 6.5, 0.0]
    # a 1 -> 1 channel k = 1 layer: dX = w dYpre
    x = torch.ones(1, 1, 7, device=dev)
    w = torch.full((1, 1, 1), 2.0, device=dev)
    gx, gw, gb = conv1d_backward(x, w, y.detach().to(dev).view(1, 1, 7), g.to(dev).view(1, 1, 7), True)
    torch.cuda.synchronize()
    assert gx.flatten().tolist() == [2 * v for v in y.grad.tolist()]
    assert gw.item() == y.grad.sum().item() and gb.item() == y.grad.sum().item()


# ---- soft-attention backward ----
SA_B, SA_C, SA_TX, SA_TY = 3, 80, 45, 70
SA_LEN = (45, 17, 0)
SA_CONFIGS = [(sim, temp, prior, gs) for sim, temp in (("l2", 0.0005), ("dot", 0.05)) for prior in (False, True)
              for gs in (False, True)]
SA_CELLS = ((41, 5, 33), (79, 16, 69))               # (c, i, j) in utterance 1: inside, and last channel / valid row / frame


@functools.lru_cache(maxsize=None)
def _sa_clean(sim, temp, prior, gs):
    dev = torch.device("cuda:0")
    k, q, _, pr, gl, gsv = _case(dev, SA_B, SA_C, SA_TX, SA_TY, False, seed=45 + 2 * prior + gs, with_prior=prior, with_gs=gs)
    t_x = torch.tensor(SA_LEN, dtype=torch.int32, device=dev)
    out = _sa_run(k, q, t_x, pr, gl, gsv, temp, sim)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    assert out[0][1, :, :17].abs().max() > 0 and not out[0][2].any() and not out[1][2].any()
    return (k, q, t_x, pr, gl, gsv), out


def _sa_run(k, q, t_x, pr, gl, gs, temp, sim):
    from aligner_amd import soft_attention_backward
    gk, gq = soft_attention_backward(k, q, gl, t_x=t_x, prior=pr, temperature=temp, sim=sim, grad_soft=gs)
    torch.cuda.synchronize()
    return gk, gq


def _clone(*ts):
    return [None if t is None else t.clone() for t in ts]


@pytest.mark.parametrize("sim,temp,prior,gs", SA_CONFIGS)
def test_softattn_backward_nan_where_nothing_reads_changes_no_bit(dev, sim, temp, prior, gs):
    (k0, q0, t_x, pr0, gl0, gs0), clean = _sa_clean(sim, temp, prior, gs)
    masked = (torch.arange(SA_TX, device=dev)[None, :] >= t_x.long()[:, None])          # [B,Tx]
    assert masked[1].any() and masked[2].all() and not masked[0].any()
    # keys rows i >= t_x
    k, = _clone(k0)
    k.masked_fill_(masked[:, None, :], NAN)
    got = _sa_run(k, q0, t_x, pr0, gl0, gs0, temp, sim)
    assert _bits_equal(got[0], clean[0]) and _bits_equal(got[1], clean[1]), "NaN in masked keys rows"
    # dlogp, dsoft, the prior on masked rows
    pr, gl, gsv = _clone(pr0, gl0, gs0)
    for t in (pr, gl, gsv):
        if t is not None:
            t.masked_fill_(masked[:, :, None], NAN)
    got = _sa_run(k0, q0, t_x, pr, gl, gsv, temp, sim)
    assert _bits_equal(got[0], clean[0]) and _bits_equal(got[1], clean[1]), "NaN in dlogp / dsoft / prior on masked rows"
    # everything of the utterance without text
    k, q, pr, gl, gsv = _clone(k0, q0, pr0, gl0, gs0)
    for t in (k, q, pr, gl, gsv):
        if t is not None:
            t[2] = NAN
    got = _sa_run(k, q, t_x, pr, gl, gsv, temp, sim)
    print(f"t_x = 0 utterance all NaN, {sim} prior={prior} gs={gs}: NaN in dK {int(torch.isnan(got[0]).sum())} "
          f"dQ {int(torch.isnan(got[1]).sum())}")
    assert _bits_equal(got[0], clean[0]) and _bits_equal(got[1], clean[1]), "NaN in the t_x = 0 utterance"


# a plant per operand the configuration passes
SA_PLANTS = [cfg + (pl,) for cfg in SA_CONFIGS for pl in ("k", "q", "gl", "gs", "prior", "negative prior")
             if (pl != "gs" or cfg[3]) and (not pl.endswith("prior") or cfg[2])]


@pytest.mark.parametrize("sim,temp,prior,gs,plant", SA_PLANTS)
def test_softattn_backward_one_nan_propagates_and_stays_put(dev, sim, temp, prior, gs, plant):
    (k0, q0, t_x, pr0, gl0, gs0), clean = _sa_clean(sim, temp, prior, gs)
    tx1 = SA_LEN[1]
    for c, i, j in SA_CELLS:
        assert i < tx1
        k, q, pr, gl, gsv = _clone(k0, q0, pr0, gl0, gs0)
        if plant == "k":
            k[1, c, i] = NAN
        elif plant == "q":
            q[1, c, j] = NAN
        elif plant == "gl":
            gl[1, i, j] = NAN
        elif plant == "gs":
            gsv[1, i, j] = NAN
        elif plant == "prior":
            pr[1, i, j] = NAN
        else:
            pr[1, i, j] = -0.5
        rk, rq = _ref_grads(k, q, t_x, pr, gl, gsv, temp, sim)
        gk, gq = _sa_run(k, q, t_x, pr, gl, gsv, temp, sim)
        # masked rows of dK: exactly zero by the kernel's rule, whatever the reference's 0 x NaN gives there
        assert not gk[1, :, tx1:].any(), "dK of a masked row is not exactly 0"
        want_k, want_q = torch.isnan(rk[1, :, :tx1]), torch.isnan(rq[1])
        got_k, got_q = torch.isnan(gk[1, :, :tx1]), torch.isnan(gq[1])
        ref_masked = int(torch.isnan(rk[1, :, tx1:]).sum())
        lost = int((want_k & ~got_k).sum()) + int((want_q & ~got_q).sum())
        stray = int((got_k & ~want_k).sum()) + int((got_q & ~want_q).sum())
        print(f"softattn backward {sim} prior={prior} gs={gs} NaN via {plant} at {(c, i, j)}: utterance 1 expected dK "
              f"{int(want_k.sum())} dQ {int(want_q.sum())}, found dK {int(got_k.sum())} dQ {int(got_q.sum())}, {lost} lost, "
              f"{stray} stray ({ref_masked} reference NaN on masked rows, 0 x NaN)")
        assert not torch.isinf(gk).any() and not torch.isinf(gq).any()
        assert lost == 0 and stray == 0
        if gs or not plant.endswith("prior"):             # (without dsoft the backward does not read the prior)
            assert want_q.any(), "the plant reached nothing in the reference"
        for b in (0, 2):
            assert _bits_equal(gk[b], clean[0][b]) and _bits_equal(gq[b], clean[1][b]), f"utterance {b} changed"
        if plant != "k":                                  # a frame's dQ depends on its own column only
            cols = torch.arange(SA_TY, device=dev) != j
            assert _bits_equal(gq[1][:, cols], clean[1][1][:, cols]), "dQ of another frame changed"
