"""Soft-attention backward (csrc/softattn_bwd.hip) at its template and tiling boundaries, against the float64 autograd
reference of test_frontend_backward_gpu.py.  Every check is per utterance (_rel_err_per_utterance): max|got - ref| <= REL
max|ref| of that utterance's own gradient, so one short utterance cannot hide under its neighbours' scale."""
import pytest
import torch

from test_frontend_backward_gpu import REL, _case, _ref_grads, _ref_soft_attention, _rel_err_per_utterance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _check(what, k, q, t_x, prior, gl, gs, temp, sim, bound=REL):
    """Both gradients against float64 autograd, per utterance; returns the kernel's (dK, dQ)."""
    from aligner_amd import soft_attention_backward
    gk, gq = soft_attention_backward(k, q, gl, t_x=t_x, prior=prior, temperature=temp, sim=sim, grad_soft=gs)
    rk, rq = _ref_grads(k, q, t_x, prior, gl, gs, temp, sim)
    torch.cuda.synchronize()
    assert gk.dtype == torch.float32 and gq.dtype == torch.float32
    assert torch.isfinite(gk).all() and torch.isfinite(gq).all()
    lens = torch.full((k.shape[0],), k.shape[2], device=k.device) if t_x is None else t_x.long()
    # an utterance without text has no log-probs at all (the reference's softmax over nothing is NaN): its gradient is zero
    rk[lens == 0] = 0.0
    rq[lens == 0] = 0.0
    assert torch.isfinite(rk).all() and torch.isfinite(rq).all()
    ek, eq = _rel_err_per_utterance(gk, rk, lens), _rel_err_per_utterance(gq, rq, lens)
    print(f"softattn backward {what}: per-utterance rel err dK {max(ek):.2e} dQ {max(eq):.2e}")
    assert max(ek) <= bound and max(eq) <= bound, (what, ek, eq)
    if t_x is not None:                                   # rows i >= t_x: exactly zero
        rows = torch.arange(k.shape[2], device=k.device)[None, None, :] >= t_x.long()[:, None, None]
        assert not (gk != 0)[rows.expand_as(gk)].any()
    return gk, gq


def _tx(dev, *vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


# one instantiation per NCT = 1, 2, 3, 4, 8, both sides of each boundary, and odd counts: the operand is indexed
# c = 2 s + half and guarded by c < C alone
@pytest.mark.parametrize("sim,temp", [("l2", 0.0005), ("dot", 0.05)])
@pytest.mark.parametrize("C", [1, 2, 31, 32, 33, 63, 64, 65, 81, 96, 97, 128, 129, 255, 256])
def test_channel_count_edges(dev, C, sim, temp):
    k, q, _, pr, gl, gs = _case(dev, 3, C, 45, 70, False, seed=77, with_prior=True, with_gs=True)
    _check(f"C={C} {sim}", k, q, _tx(dev, 45, 17, 33), pr, gl, gs, temp, sim)


@pytest.mark.parametrize("Tx", [1, 31, 32, 33])
@pytest.mark.parametrize("sim,temp", [("l2", 0.0005), ("dot", 0.05)])
def test_text_length_edges(dev, Tx, sim, temp):
    k, q, _, _, gl, gs = _case(dev, 3, 80, Tx, 70, False, seed=100 + Tx, with_gs=True)
    _check(f"Tx={Tx} {sim}", k, q, _tx(dev, Tx, (Tx + 1) // 2, Tx), None, gl, gs, temp, sim)
    _check(f"Tx={Tx} {sim} unmasked", k, q, None, None, gl, None, temp, sim)


@pytest.mark.parametrize("C", [16, 80])
def test_longest_text(dev, C):
    """Tx = 512, the entry point's limit: two staging groups in the column kernel even at NCT = 1."""
    k, q, _, pr, gl, gs = _case(dev, 2, C, 512, 130, False, seed=512 + C, with_prior=True, with_gs=True)
    _check(f"Tx=512 C={C}", k, q, _tx(dev, 512, 481), pr, gl, gs, 0.0005, "l2")
    _check(f"Tx=512 C={C} dot", k, q, None, None, gl, None, 0.05, "dot")


@pytest.mark.parametrize("sim,temp", [("l2", 0.0005), ("dot", 0.05)])
def test_text_lengths_on_tile_boundaries(dev, sim, temp):
    """t_x of exactly 32, 64, 1 and Tx, and t_x = 0 between full-length utterances."""
    k, q, _, _, gl, gs = _case(dev, 7, 80, 96, 150, False, seed=96, with_gs=True)
    t_x = _tx(dev, 96, 32, 0, 64, 1, 0, 96)
    gk, gq = _check(f"t_x on tile edges {sim}", k, q, t_x, None, gl, gs, temp, sim)
    for b in (2, 5):
        assert not gk[b].any() and not gq[b].any()


# Ty = 1 .. 129: 1, 1, 1, 2, 4, 4 and 5 strips of 32 frames; a wave of the row kernel takes every fourth strip, so with 2
# strips two waves take none, with exactly 4 each takes one, with 5 the first takes two
@pytest.mark.parametrize("Ty", [1, 31, 32, 33, 127, 128, 129])
@pytest.mark.parametrize("sim,temp", [("l2", 0.0005), ("dot", 0.05)])
def test_frame_count_edges(dev, Ty, sim, temp):
    k, q, _, pr, gl, gs = _case(dev, 2, 80, 50, Ty, False, seed=300 + Ty, with_prior=True, with_gs=True)
    _check(f"Ty={Ty} {sim}", k, q, _tx(dev, 50, 23), pr, gl, gs, temp, sim)


@pytest.mark.parametrize("C,Tx,Ty", [(256, 70, 100), (80, 200, 150)])
def test_grad_soft_with_prior(dev, C, Tx, Ty):
    """G_s with a prior where the mel operand is read again instead of kept in registers (C > 128), and where the column
    kernel stages the text in two groups (C = 80: 160 rows a group)."""
    k, q, t_x, pr, gl, gs = _case(dev, 3, C, Tx, Ty, True, seed=C + Tx, with_prior=True, with_gs=True)
    _check(f"G_s + prior C={C} Tx={Tx}", k, q, t_x, pr, gl, gs, 0.0005, "l2")
    _check(f"G_s + prior C={C} Tx={Tx} dot", k, q, t_x, pr, gl, gs, 0.02, "dot")


def test_prior_with_zeros_and_tiny_values(dev):
    """log(prior + 1e-8) at prior = 0 (-18.4) and 1e-6: soft is then far from softmax(logit)."""
    k, q, t_x, pr, gl, gs = _case(dev, 3, 80, 60, 130, True, seed=61, with_prior=True, with_gs=True)
    g = torch.Generator().manual_seed(62)
    u = torch.rand(pr.shape, generator=g).to(dev)
    pr = torch.where(u < 0.3, torch.zeros_like(pr), torch.where(u < 0.5, torch.full_like(pr, 1e-6), pr))
    assert (pr == 0).any() and (pr == 1e-6).any()
    _check("prior with zeros", k, q, t_x, pr, gl, gs, 0.0005, "l2")


def test_grad_soft_alone(dev):
    """Only `soft` is used: autograd hands _SoftAttention.backward no cotangent for logp, which builds a zero one."""
    import aligner_amd
    k, q, t_x, pr, gl, gs = _case(dev, 3, 80, 60, 130, True, seed=63, with_prior=True, with_gs=True)
    gk, gq = _check("G_s alone", k, q, t_x, pr, torch.zeros_like(gl), gs, 0.0005, "l2")
    kr, qr = k.clone().requires_grad_(), q.clone().requires_grad_()
    _, soft = aligner_amd.soft_attention(kr, qr, t_x=t_x, prior=pr, want_soft=True)
    (soft * gs).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(kr.grad, gk) and torch.equal(qr.grad, gq)


@pytest.mark.parametrize("sim,temp", [("l2", 0.3), ("dot", 0.5)])
def test_sharp_attention(dev, sim, temp):
    """Near-one-hot attention: every frame's query is one of its utterance's keys plus a little noise, at a temperature that
    puts more than 0.999 of the float64 softmax on that row for most frames (asserted, so the case cannot drift into being
    easy).  The logits span hundreds; their fp32 rounding, |logit| 2^-24, is a relative error of that size in p (about 1e-5 at
    |logit| = 200), still under REL: measured 4e-7 (dK) and 6e-7 (dQ) for both sims, log-probs spanning 307 and 273."""
    B, C, Tx, Ty = 3, 80, 90, 200
    g = torch.Generator().manual_seed(90)
    k = torch.randn(B, C, Tx, generator=g) * 2.0
    t_x = torch.tensor([Tx, 41, 64], dtype=torch.int32)
    row = (torch.rand(B, Ty, generator=g) * t_x[:, None]).long().clamp_(max=Tx - 1)
    q = torch.gather(k, 2, row[:, None, :].expand(B, C, Ty)) + 0.1 * torch.randn(B, C, Ty, generator=g)
    valid = (torch.arange(Tx)[None, :, None] < t_x.long()[:, None, None]).float()
    gl = torch.randn(B, Tx, Ty, generator=g) * valid
    gs = torch.randn(B, Tx, Ty, generator=g) * valid
    k, q, t_x, gl, gs = (t.to(dev) for t in (k, q, t_x, gl, gs))
    logp, soft = _ref_soft_attention(k.double(), q.double(), t_x, None, temp, sim)
    sharp = (soft.max(dim=1).values > 0.999).double().mean().item()
    fin = torch.isfinite(logp)
    span = (logp[fin].max() - logp[fin].min()).item()
    print(f"sharp {sim}: {sharp:.3f} of the frames above 0.999, log-probs span {span:.0f}")
    assert sharp > 0.9 and span > 100
    _check(f"sharp {sim}", k, q, t_x, None, gl, gs, temp, sim)


@pytest.mark.parametrize("sim,temp", [("l2", 0.0005), ("dot", 0.05)])
def test_cotangents_on_masked_rows_are_ignored(dev, sim, temp):
    """Finite non-zero G_l / G_s on rows i >= t_x (logp = -inf there, a constant): the same bits as with those rows zeroed."""
    from aligner_amd import soft_attention_backward
    k, q, t_x, pr, gl, gs = _case(dev, 4, 80, 70, 150, True, seed=70, with_prior=True, with_gs=True)
    t_x[1], t_x[2] = 33, 0
    g = torch.Generator().manual_seed(71)
    masked = (torch.arange(70, device=dev)[None, :, None] >= t_x.long()[:, None, None]).expand_as(gl)
    gl2 = (torch.randn(gl.shape, generator=g) * 3.0 + 0.5).to(dev)
    gs2 = (torch.randn(gs.shape, generator=g) * 3.0 - 0.5).to(dev)
    gl, gs = gl2.masked_fill(masked, 0.0), gs2.masked_fill(masked, 0.0)
    assert masked.any() and (gl2[masked] != 0).all() and (gs2[masked] != 0).all() and not gl[masked].any()
    gk, gq = _check(f"cotangents on masked rows {sim}", k, q, t_x, pr, gl2, gs2, temp, sim)
    gk0, gq0 = soft_attention_backward(k, q, gl, t_x=t_x, prior=pr, temperature=temp, sim=sim, grad_soft=gs)
    torch.cuda.synchronize()
    assert torch.equal(gk, gk0) and torch.equal(gq, gq0)
