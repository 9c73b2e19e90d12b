"""GPU tests of the front end's backward (soft attention and the conv encoders) against torch autograd through a float64
restatement of oracle/softattn_oracle.py (the oracle itself computes in fp32).  Tolerance: max|got - ref| <= 1e-4 max|ref|
per gradient tensor unless noted.  Cotangents on masked rows (i >= t_x: logp = -inf there, a constant) are zero, as any
loss of the log-probs gives them."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel_err(got, ref):
    got = got.detach().double().to(ref.device)
    scale = ref.abs().max().item()
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)


def _rel_err_per_utterance(got, ref, lengths=None):
    """_rel_err of every batch element against that element's OWN max|ref| (a list of B figures): a wrong gradient of one
    short utterance does not hide under its neighbours' scale.  lengths: the utterances' text lengths.  With fewer than two
    text rows the log-softmax over the text is constant, the true gradient identically zero and there is no scale of its
    own: such an utterance is held to the batch's largest (to 1 if that is zero too)."""
    got = got.detach().double().to(ref.device)
    err = (got - ref).abs().flatten(1).max(dim=1).values
    scale = ref.abs().flatten(1).max(dim=1).values
    if lengths is not None:
        scale = torch.where(lengths.to(ref.device) < 2, scale.max().expand_as(scale), scale)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return (err / scale).tolist()


def _ref_soft_attention(k, q, t_x=None, prior=None, temperature=0.0005, sim="l2"):
    """oracle/softattn_oracle.soft_attention in float64 (|q|^2 + |k|^2 - 2 k.q: no [B,C,Tx,Ty] temporary)."""
    if sim == "l2":
        d = (q * q).sum(1)[:, None, :] + (k * k).sum(1)[:, :, None] - 2.0 * torch.einsum("bci,bcj->bij", k, q)
        logit = -temperature * d
    else:
        logit = temperature * torch.einsum("bci,bcj->bij", k, q)
    B, Tx, Ty = logit.shape
    if t_x is not None:
        rows = torch.arange(Tx, device=k.device)[None, :, None] >= t_x.to(k.device, torch.long)[:, None, None]
        logit = logit.masked_fill(rows, float("-inf"))
    logp = torch.log_softmax(logit, dim=1)
    if prior is not None:
        logp = logp + torch.log(prior.double() + 1e-8)
    return logp, torch.softmax(logp, dim=1)


def _case(dev, B, C, Tx, Ty, ragged, seed, with_prior=False, with_gs=False):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, C, Tx, generator=g) * 2.0
    q = torch.randn(B, C, Ty, generator=g) * 2.0
    t_x = None
    if ragged:
        t_x = torch.randint(1, Tx + 1, (B,), generator=g, dtype=torch.int32)
        t_x[0] = Tx
    valid = torch.ones(B, Tx, 1)
    if t_x is not None:
        valid = (torch.arange(Tx)[None, :, None] < t_x.long()[:, None, None]).float()
    gl = torch.randn(B, Tx, Ty, generator=g) * valid
    gs = torch.randn(B, Tx, Ty, generator=g) * valid if with_gs else None
    prior = torch.rand(B, Tx, Ty, generator=g) + 0.05 if with_prior else None
    mv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    return mv(k), mv(q), mv(t_x), mv(prior), mv(gl), mv(gs)


def _ref_grads(k, q, t_x, prior, gl, gs, temperature, sim):
    kr = k.double().requires_grad_()
    qr = q.double().requires_grad_()
    logp, soft = _ref_soft_attention(kr, qr, t_x, prior, temperature, sim)
    fin = torch.isfinite(logp)
    obj = (torch.where(fin, logp, torch.zeros_like(logp)) * gl.double()).sum()
    if gs is not None:
        obj = obj + (soft * gs.double()).sum()
    obj.backward()
    return kr.grad, qr.grad


@pytest.mark.parametrize("B,C,Tx,Ty,sim,ragged,prior,gs,temp", [
    (2, 80, 50, 130, "l2", False, False, False, 0.0005),
    (3, 80, 200, 333, "l2", True, False, False, 0.0005),
    (2, 16, 7, 40, "dot", False, False, False, 0.05),
    (3, 80, 230, 130, "dot", True, False, False, 0.05),
    (1, 80, 500, 1000, "l2", False, True, False, 0.0005),
    (2, 128, 224, 257, "l2", True, True, True, 0.0005),
    (2, 128, 224, 257, "l2", False, False, True, 0.0005),
    (2, 256, 70, 100, "l2", True, False, False, 0.0005),
    (2, 200, 130, 64, "dot", False, False, True, 0.02),
    (2, 80, 60, 90, "l2", True, False, False, 0.05),          # sharp: the forward's exact-product form
    (64, 80, 200, 1000, "l2", False, False, False, 0.0005),   # bench shape
    (64, 80, 200, 1000, "l2", True, False, False, 0.0005),
])
def test_soft_attention_gradients_match_float64_autograd(dev, B, C, Tx, Ty, sim, ragged, prior, gs, temp):
    from aligner_amd import soft_attention_backward
    k, q, t_x, pr, gl, gsv = _case(dev, B, C, Tx, Ty, ragged, seed=B * 1000 + Tx, with_prior=prior, with_gs=gs)
    gk, gq = soft_attention_backward(k, q, gl, t_x=t_x, prior=pr, temperature=temp, sim=sim, grad_soft=gsv)
    rk, rq = _ref_grads(k, q, t_x, pr, gl, gsv, temp, sim)
    torch.cuda.synchronize()
    assert gk.dtype == torch.float32 and gq.dtype == torch.float32
    assert torch.isfinite(gk).all() and torch.isfinite(gq).all()
    ek, eq = _rel_err(gk, rk), _rel_err(gq, rq)
    assert ek <= REL and eq <= REL, (ek, eq)
    if B == 64:         # the bench shape: every utterance at its own scale as well
        pk, pq = _rel_err_per_utterance(gk, rk, t_x), _rel_err_per_utterance(gq, rq, t_x)
        print(f"softattn backward [64,80,200,1000] ragged={ragged}: per-utterance rel err dK {max(pk):.2e} dQ {max(pq):.2e}")
        assert max(pk) <= REL and max(pq) <= REL, (pk.index(max(pk)), max(pk), pq.index(max(pq)), max(pq))


def test_soft_attention_backward_edges(dev):
    from aligner_amd import soft_attention_backward
    k, q, _, _, gl, _ = _case(dev, 3, 80, 70, 150, False, seed=5)
    t_x = torch.tensor([70, 33, 0], dtype=torch.int32, device=dev)
    gl = gl.clone()
    gk, gq = soft_attention_backward(k, q, gl, t_x=t_x)
    torch.cuda.synchronize()
    assert torch.isfinite(gk).all() and torch.isfinite(gq).all()
    assert torch.equal(gk[1, :, 33:], torch.zeros_like(gk[1, :, 33:]))       # masked rows: exactly zero
    assert torch.equal(gk[2], torch.zeros_like(gk[2])) and torch.equal(gq[2], torch.zeros_like(gq[2]))   # t_x = 0
    assert gk[1, :, :33].abs().max() > 0
    # one side only: the same bits as that side of the full call
    gk1, gq1 = soft_attention_backward(k, q, gl, t_x=t_x, need_queries=False)
    gk2, gq2 = soft_attention_backward(k, q, gl, t_x=t_x, need_keys=False)
    torch.cuda.synchronize()
    assert gq1 is None and gk2 is None
    assert torch.equal(gk1, gk) and torch.equal(gq2, gq)
    # repeat: bit-identical
    gk3, gq3 = soft_attention_backward(k, q, gl, t_x=t_x)
    torch.cuda.synchronize()
    assert torch.equal(gk3, gk) and torch.equal(gq3, gq)


def _ref_conv_grads(x, w, y, gy, relu):
    gyp = gy.double() * (y > 0).double() if relu else gy.double()
    xr = x.double().requires_grad_()
    wr = w.double().requires_grad_()
    br = torch.zeros(w.shape[0], dtype=torch.float64, device=x.device, requires_grad=True)
    F.conv1d(xr, wr, br, padding=w.shape[-1] // 2).backward(gyp)
    return xr.grad, wr.grad, br.grad


@pytest.mark.parametrize("B,Ci,Co,T,K,relu", [
    (2, 80, 160, 300, 3, True), (2, 160, 80, 300, 1, False), (1, 33, 70, 129, 5, True), (2, 512, 1024, 50, 3, True),
    (2, 80, 160, 300, 3, False), (1, 40, 72, 77, 3, True), (1, 24, 16, 5, 5, False), (3, 64, 100, 61, 1, True),
])
def test_conv1d_backward_matches_float64_autograd(dev, B, Ci, Co, T, K, relu):
    import aligner_amd
    g = torch.Generator().manual_seed(B * 7 + Ci + K)
    x = torch.randn(B, Ci, T, generator=g).to(dev)
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).to(dev)
    b = torch.randn(Co, generator=g).to(dev)
    gy = torch.randn(B, Co, T, generator=g).to(dev)
    y = aligner_amd.conv1d(x, w, b, relu)
    gx, gw, gb = aligner_amd.conv1d_backward(x, w, y, gy, relu)
    rx, rw, rb = _ref_conv_grads(x, w, y, gy, relu)
    torch.cuda.synchronize()
    errs = (_rel_err(gx, rx), _rel_err(gw, rw), _rel_err(gb, rb))
    assert max(errs) <= REL, errs
    gx2, gw2, gb2 = aligner_amd.conv1d_backward(x, w, y, gy, relu)
    torch.cuda.synchronize()
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    # partial requests: the same bits
    gxa, gwa, gba = aligner_amd.conv1d_backward(x, w, y, gy, relu, need_w=False, need_b=False)
    _, gwb, gbb = aligner_amd.conv1d_backward(x, w, y, gy, relu, need_x=False)
    torch.cuda.synchronize()
    assert gwa is None and gba is None and torch.equal(gxa, gx) and torch.equal(gwb, gw) and torch.equal(gbb, gb)


def _ctc_mean_loss_f64(logp, t_x, t_y, blank=-1.0):
    """forward_sum_loss's CTC form, reduction "mean", in float64 torch (as tests/test_objective.py pins it)."""
    losses = []
    for b in range(logp.shape[0]):
        K, T = int(t_x[b]), int(t_y[b])
        lp = torch.cat([torch.full((1, T), blank, dtype=torch.float64, device=logp.device), logp[b, :K, :T]], dim=0)
        lp = torch.log_softmax(lp, dim=0).t().unsqueeze(1)
        losses.append(F.ctc_loss(lp.cpu(), torch.arange(1, K + 1).unsqueeze(0), torch.tensor([T]), torch.tensor([K]),
                                 blank=0, reduction="none", zero_infinity=False)[0])
    return torch.stack(losses).mean()


def test_training_step_end_to_end(dev):
    """alignment_encoder -> forward_sum_loss -> backward(): every parameter's gradient and the text's against the float64
    torch pipeline, 1e-3 of each tensor's max (fp32 through the whole chain).  The attention is made informative (inputs of
    a few units, temperature 0.002, still the forward's bf16x3 form): with near-uniform attention the last layers' bias
    gradients are sums that cancel to ~1/100 of the weights' (sum_i dlogit = 0 per frame), and their relative error is
    then set by the fp32 forward, not by the backward."""
    import aligner_amd
    params = aligner_amd.AlignmentEncoderParams.random(32, 40, 24, dev, seed=3)
    params.temperature = 0.002
    for w, b in params.key_proj + params.query_proj:
        w.requires_grad_()
        b.requires_grad_()
    g = torch.Generator().manual_seed(4)
    text = (torch.randn(2, 32, 20, generator=g) * 3.0).to(dev).requires_grad_()
    mel = (torch.randn(2, 40, 60, generator=g) * 3.0).to(dev)
    t_x = torch.tensor([20, 13], dtype=torch.int32, device=dev)
    t_y = torch.tensor([60, 41], dtype=torch.int32, device=dev)
    logp, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x)
    assert logp.grad_fn is not None
    loss = aligner_amd.forward_sum_loss(logp, t_x, t_y, blank_logprob=-1.0)
    loss.backward()
    torch.cuda.synchronize()
    # float64 torch pipeline
    leaves = [(w.detach().double().requires_grad_(), b.detach().double().requires_grad_()) for w, b in params.key_proj + params.query_proj]
    nk = len(params.key_proj)
    tr = text.detach().double().requires_grad_()

    def enc(x, stack):
        for n, (w, b) in enumerate(stack):
            x = F.conv1d(x, w, b, padding=w.shape[-1] // 2)
            x = torch.relu(x) if n + 1 < len(stack) else x
        return x
    lp, _ = _ref_soft_attention(enc(tr, leaves[:nk]), enc(mel.double(), leaves[nk:]), t_x, None, params.temperature)
    want = _ctc_mean_loss_f64(lp, t_x.cpu(), t_y.cpu())
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-3 * abs(want.item())
    assert _rel_err(text.grad, tr.grad) <= 1e-3
    for (w, b), (wr, br) in zip(params.key_proj + params.query_proj, leaves):
        assert w.grad is not None and b.grad is not None
        assert _rel_err(w.grad, wr.grad) <= 1e-3 and _rel_err(b.grad, br.grad) <= 1e-3


def test_training_step_at_real_widths(dev):
    """The same step with the encoders' real widths (512 text, 80 mel, 80 attention channels), B = 8, ragged t_x <= 60 and
    t_y <= 300: the weight-gradient kernel then walks several chunks a split (80 units on the mel layers; 16 units over 6
    splits on the 512 -> 1024 text layer), where the small step above gives it one.  Same CTC-form loss, same float64
    pipeline, same 1e-3 of each tensor's max, for every weight and bias and for text.grad and mel.grad.
    As above the attention must not be near-uniform (the last layers' bias gradients would cancel to ~1/50 of their weights'
    at inputs of unit scale and temperature 0.0005, and their relative error would be the fp32 forward's): inputs of a few
    units and temperature 0.01, and the float64 reference is asserted to give every bias gradient a max of at least a tenth
    of its weight's (it gives 0.16 to 0.60), so the relative bound means something for each tensor."""
    import aligner_amd
    params = aligner_amd.AlignmentEncoderParams.random(512, 80, 80, dev, seed=5)
    params.temperature = 0.01
    for w, b in params.key_proj + params.query_proj:
        w.requires_grad_()
        b.requires_grad_()
    g = torch.Generator().manual_seed(6)
    text = (torch.randn(8, 512, 60, generator=g) * 3.0).to(dev).requires_grad_()
    mel = (torch.randn(8, 80, 300, generator=g) * 3.0).to(dev).requires_grad_()
    t_x = torch.tensor([60, 13, 47, 32, 60, 5, 33, 59], dtype=torch.int32, device=dev)
    t_y = torch.tensor([300, 70, 255, 160, 289, 64, 200, 300], dtype=torch.int32, device=dev)
    logp, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x)
    loss = aligner_amd.forward_sum_loss(logp, t_x, t_y, blank_logprob=-1.0)
    loss.backward()
    torch.cuda.synchronize()
    leaves = [(w.detach().double().requires_grad_(), b.detach().double().requires_grad_()) for w, b in params.key_proj + params.query_proj]
    nk = len(params.key_proj)
    tr = text.detach().double().requires_grad_()
    mr = mel.detach().double().requires_grad_()

    def enc(x, stack):
        for n, (w, b) in enumerate(stack):
            x = F.conv1d(x, w, b, padding=w.shape[-1] // 2)
            x = torch.relu(x) if n + 1 < len(stack) else x
        return x
    lp, _ = _ref_soft_attention(enc(tr, leaves[:nk]), enc(mr, leaves[nk:]), t_x, None, params.temperature)
    want = _ctc_mean_loss_f64(lp, t_x.cpu(), t_y.cpu())
    want.backward()
    for wr, br in leaves:
        assert br.grad.abs().max().item() >= 0.1 * wr.grad.abs().max().item() > 0
    assert tr.grad.abs().max().item() > 0 and mr.grad.abs().max().item() > 0
    errs = {"loss": abs(loss.item() - want.item()) / abs(want.item()), "text": _rel_err(text.grad, tr.grad),
            "mel": _rel_err(mel.grad, mr.grad)}
    for n, ((w, b), (wr, br)) in enumerate(zip(params.key_proj + params.query_proj, leaves)):
        assert w.grad is not None and b.grad is not None
        errs[f"w{n}"], errs[f"b{n}"] = _rel_err(w.grad, wr.grad), _rel_err(b.grad, br.grad)
    print("training step at real widths: rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-3, errs


def test_no_grad_path_is_unchanged(dev):
    import aligner_amd
    from aligner_amd.softattn import encode
    params = aligner_amd.AlignmentEncoderParams.random(64, 80, 80, dev, seed=1)
    g = torch.Generator().manual_seed(9)
    text = torch.randn(2, 64, 40, generator=g).to(dev)
    mel = torch.randn(2, 80, 168, generator=g).to(dev)
    t_x = torch.tensor([40, 25], dtype=torch.int32, device=dev)
    lp, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x, pitched=True)
    with torch.no_grad():
        lp0, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x, pitched=True)
    k = encode(text, params.key_proj)
    q = encode(mel, params.query_proj)
    sa, soft = aligner_amd.soft_attention(k, q, t_x=t_x, want_soft=True)
    with torch.no_grad():
        sa0, soft0 = aligner_amd.soft_attention(k, q, t_x=t_x, want_soft=True)
    # the grad path runs the same forward kernel: same bits
    sag, softg = aligner_amd.soft_attention(k.clone().requires_grad_(), q, t_x=t_x, want_soft=True)
    torch.cuda.synchronize()
    assert lp.grad_fn is None and sa.grad_fn is None and soft.grad_fn is None
    assert torch.equal(lp, lp0) and torch.equal(sa, sa0) and torch.equal(soft, soft0)
    assert sag.grad_fn is not None and torch.equal(sag.detach(), sa) and torch.equal(softg.detach(), soft)
    with pytest.raises(ValueError, match="out="):
        aligner_amd.soft_attention(k.clone().requires_grad_(), q, out=torch.empty_like(sa))
    with pytest.raises(ValueError, match="prior"):
        aligner_amd.soft_attention(k.clone().requires_grad_(), q, prior=torch.rand_like(sa).requires_grad_())


def test_bf16_logp_with_grad(dev):
    import aligner_amd
    k, q, t_x, _, gl, _ = _case(dev, 2, 80, 50, 130, True, seed=12)
    kr = k.clone().requires_grad_()
    qr = q.clone().requires_grad_()
    lp, _ = aligner_amd.soft_attention(kr, qr, t_x=t_x, logp_dtype=torch.bfloat16)
    assert lp.dtype == torch.bfloat16
    (torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp)).float() * gl).sum().backward()
    gk, gq = aligner_amd.soft_attention_backward(k, q, gl.bfloat16().float(), t_x=t_x)    # the cotangent arrives as bf16
    torch.cuda.synchronize()
    assert kr.grad.dtype == torch.float32 and torch.equal(kr.grad, gk) and torch.equal(qr.grad, gq)


def test_backward_entry_points_replay_in_a_hip_graph(dev):
    import aligner_amd
    k, q, t_x, _, gl, _ = _case(dev, 4, 80, 120, 300, True, seed=21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(4, 128, 120, generator=g).to(dev)
    w = (torch.randn(256, 128, 3, generator=g) / 20.0).to(dev)
    bias = torch.randn(256, generator=g).to(dev)
    y = aligner_amd.conv1d(x, w, bias, relu=True)
    gy = torch.randn(4, 256, 120, generator=g).to(dev)

    def run():
        gk, gq = aligner_amd.soft_attention_backward(k, q, gl, t_x=t_x)
        gx, gw, gb = aligner_amd.conv1d_backward(x, w, y, gy, True)
        return gk, gq, gx, gw, gb

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = run()
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = run()
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
