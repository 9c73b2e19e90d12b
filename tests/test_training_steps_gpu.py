"""What only a training run exercises: weights that change between calls.

aligner_amd/softattn.py keeps a prepared image of every conv weight (`_prepared`, and `_prepared_t` for the transposed image
of the input gradient), keyed by the caller's tensor and refreshed when torch's version counter moves.  A stale image leaves
the forward on old weights while the optimizer goes on, and no single-call test notices.  Here the weights move:

 (a) three optimizer steps, every step compared with the float64 pipeline of test_training_step_end_to_end started from
     the GPU's own weights of that step (errors do not compound: that test's bound, 1e-3 of each tensor's max), the
     reference loss asserted to move by at least 20 loss tolerances a step, so a forward on the previous step's image
     fails by a wide margin.  Adam(fused=True) did: torch's fused optimizers leave the version counter where it was, so
     a weight that requires grad is now prepared on every call (two tests below the steps pin the cause and the rule);
 (b) the no-grad encode(), in one C-ABI call and layer by layer, after in-place updates and after the documented bypass
     (`p.data.copy_()` + invalidate_prepared());
 (c) aliases: detach(), one tensor as two layers, a slice of a larger parameter updated through its base;
 (d) weights the kernels cannot read as they are (a bf16 parameter, a strided fp32 view): the bits of the fp32 contiguous
     call, no memory retained call after call, and more weights than the cache holds;
 (e) two streams;  (f) a captured graph replayed after an update.

"The same bits" is always against the same call on FRESH copies of the weights (new addresses: nothing cached)."""
import pytest
import torch
import torch.nn.functional as F

from test_frontend_backward_gpu import _ctc_mean_loss_f64, _ref_soft_attention, _rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3                     # test_training_step_end_to_end's bound: of |loss|, and of each gradient tensor's max


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- (a) optimizer steps ----
# At these weights the loss is flat (max |grad| 0.0033) and stiff: the single SGD step that moves it by 2 % multiplies the
# gradient by 700, and with one rate for all steps the float64 pipeline either moves the loss by 0.3 % or reaches 1e10
# at the second step.  The rate is therefore set per step, as a scheduler sets it (param_groups[...]["lr"]).  Float64
# pipeline on the CPU with these rates: SGD 64.74 -> 69.70 -> 62.71 -> 59.31 (7.1 %, 10.0 %, 5.4 % a step), Adam
# 64.74 -> 68.91 -> 60.39 -> 52.47 (6.1 %, 12.4 %, 13.1 %); required 20 TOL = 2 %.
SGD_RATES = (180.0, 0.01, 0.02)
ADAM_RATES = (0.12, 0.02, 0.02)


def _enc64(x, stack):
    for n, (w, b) in enumerate(stack):
        x = F.conv1d(x, w, b, padding=w.shape[-1] // 2)
        x = torch.relu(x) if n + 1 < len(stack) else x
    return x


@pytest.mark.parametrize("optimizer", ["sgd", "sgd_foreach", "adam_fused", "sub_loop"])
def test_three_optimizer_steps_match_float64(dev, optimizer):
    import aligner_amd
    params = aligner_amd.AlignmentEncoderParams.random(32, 40, 24, dev, seed=3)
    params.temperature = 0.002
    layers = params.key_proj + params.query_proj
    leaves = [t.requires_grad_() for wb in layers for t in wb]
    nk = len(params.key_proj)
    g = torch.Generator().manual_seed(4)
    text = (torch.randn(2, 32, 20, generator=g) * 3.0).to(dev).requires_grad_()
    mel = (torch.randn(2, 40, 60, generator=g) * 3.0).to(dev)
    t_x = torch.tensor([20, 13], dtype=torch.int32, device=dev)
    t_y = torch.tensor([60, 41], dtype=torch.int32, device=dev)
    rates = ADAM_RATES if optimizer == "adam_fused" else SGD_RATES
    opt = None
    if optimizer in ("sgd", "sgd_foreach"):
        opt = torch.optim.SGD(leaves, lr=rates[0], foreach=(optimizer == "sgd_foreach"))
    elif optimizer == "adam_fused":
        try:
            opt = torch.optim.Adam(leaves, lr=rates[0], fused=True)
        except (RuntimeError, ValueError, TypeError) as e:
            pytest.skip(f"this torch build refuses Adam(fused=True) for these tensors: {e}")
    prev = None
    for s in range(len(rates) + 1):
        for p in leaves + [text]:
            p.grad = None
        logp, _ = aligner_amd.alignment_encoder(text, mel, params, t_x=t_x)
        loss = aligner_amd.forward_sum_loss(logp, t_x, t_y, blank_logprob=-1.0)
        loss.backward()
        torch.cuda.synchronize()
        # the float64 pipeline from the GPU's weights of this step (fp32 -> float64 is exact)
        ref = [(w.detach().double().requires_grad_(), b.detach().double().requires_grad_()) for w, b in layers]
        tr = text.detach().double().requires_grad_()
        lp, _ = _ref_soft_attention(_enc64(tr, ref[:nk]), _enc64(mel.double(), ref[nk:]), t_x, None, params.temperature)
        want = _ctc_mean_loss_f64(lp, t_x.cpu(), t_y.cpu())
        want.backward()
        want = want.item()
        if prev is not None:
            moved = abs(want - prev) / max(abs(want), abs(prev))
            print(f"{optimizer} step {s}: reference loss {prev:.4f} -> {want:.4f}, moved {moved:.4f} (required {20 * TOL})")
            assert moved >= 20 * TOL, "the reference loss did not move enough for a stale image to show"
        prev = want
        errs = {"loss": abs(loss.item() - want) / abs(want), "text": _rel_err(text.grad, tr.grad)}
        for n, ((w, b), (wr, br)) in enumerate(zip(layers, ref)):
            assert w.grad is not None and b.grad is not None
            errs[f"w{n}"], errs[f"b{n}"] = _rel_err(w.grad, wr.grad), _rel_err(b.grad, br.grad)
        print(f"{optimizer} step {s}: loss {loss.item():.4f}, rel err " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= TOL, (s, errs)
        if s == len(rates):
            break
        if opt is None:
            with torch.no_grad():
                for p in leaves:
                    p.sub_(rates[s] * p.grad)
        else:
            for group in opt.param_groups:
                group["lr"] = rates[s]
            try:
                opt.step()
            except (RuntimeError, NotImplementedError) as e:
                if optimizer == "adam_fused" and s == 0:
                    pytest.skip(f"this torch build refuses Adam(fused=True) for these tensors: {e}")
                raise


def test_fused_optimizers_do_not_move_the_version_counter():
    """Why a weight that requires grad is never served from the cache: torch's fused optimizers update it in place and
    leave `_version` where it was (the foreach and single-tensor forms move it).  If this ever stops holding, the rule
    in aligner_amd/softattn.py may be relaxed; until then adam_fused above depends on it."""
    moved = {}
    for name, kw in (("fused", dict(fused=True)), ("foreach", dict(foreach=True))):
        p = torch.ones(4, 4, requires_grad=True)
        p.grad = torch.ones(4, 4)
        try:
            torch.optim.SGD([p], lr=0.5, **kw).step()
        except (RuntimeError, ValueError, TypeError) as e:
            pytest.skip(f"this torch build refuses SGD({name}=True) on the CPU: {e}")
        assert torch.equal(p.detach(), torch.full((4, 4), 0.5))
        moved[name] = p._version
    print(f"_version after one step: {moved}")
    assert moved["foreach"] > 0


def test_a_weight_that_requires_grad_is_prepared_on_every_call(dev):
    """An update the version counter does not see (as a fused optimizer's; here through .data) on a weight that requires
    grad, no invalidate_prepared(): the direct calls under no_grad and the autograd path both run on the new values."""
    import aligner_amd
    x, w, b, gy = _layer(dev, 80, 160, 3)
    w.requires_grad_()
    xr = x.clone().requires_grad_()

    def through_autograd(wt):
        xr.grad = None
        y = aligner_amd.conv1d(xr, wt, b, relu=True)
        y.backward(gy)
        return y.detach(), xr.grad

    before, before_ag = _fwd_bwd(x, w, b, gy), through_autograd(w)
    version = w._version
    w.data.mul_(0.75).add_(0.01)
    assert w._version == version
    after, after_ag = _fwd_bwd(x, w, b, gy), through_autograd(w)
    torch.cuda.synchronize()
    want = _fwd_bwd(x, _fresh(w), b, gy)
    assert _same(after, want), "a direct call ran on a stale image of a weight that requires grad"
    assert _same(after_ag, want), "the autograd path ran on a stale image"
    assert _same(before_ag, before) and not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


# ---- helpers of (b) .. (f): one layer, forward and input gradient (both tables) ----
def _layer(dev, Ci, Co, K, B=2, T=70, seed=0):
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + K + seed)
    x = torch.randn(B, Ci, T, generator=g).to(dev)
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).to(dev)
    b = (torch.randn(Co, generator=g) * 0.1).to(dev)
    gy = torch.randn(B, Co, T, generator=g).to(dev)
    return x, w, b, gy


def _fwd_bwd(x, w, b, gy):
    """(y, dX) of a ReLU layer: the forward image and the transposed one."""
    import aligner_amd
    with torch.no_grad():
        y = aligner_amd.conv1d(x, w, b, relu=True)
        gx, _, _ = aligner_amd.conv1d_backward(x, w, y, gy, True, need_w=False, need_b=False)
    return y, gx


def _fresh(w):
    """The weight's values as a new fp32 contiguous tensor: a new address, nothing cached for it."""
    return w.detach().float().contiguous().clone()


def _same(got, want):
    return all(_bits_equal(a, b) for a, b in zip(got, want))


def _update(*ts):
    with torch.no_grad():
        for t in ts:
            t.mul_(0.75).add_(0.01)


# ---- (b) the no-grad encode() ----
STACKS = {"one_call": ((80, 160, 80, 80), (3, 1, 1)), "layer_by_layer": ((8, 40, 16), (3, 1))}


@pytest.mark.parametrize("kind", sorted(STACKS))
def test_no_grad_encode_follows_the_weights(dev, kind):
    from aligner_amd import _lib
    from aligner_amd.softattn import encode, invalidate_prepared
    chans, ks = STACKS[kind]
    B, T = 2, 70
    g = torch.Generator().manual_seed(len(kind))
    x = torch.randn(B, chans[0], T, generator=g).to(dev)
    stack = [((torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5).to(dev), (torch.randn(co, generator=g) * 0.1).to(dev))
             for ci, co, k in zip(chans[:-1], chans[1:], ks)]
    arr = (_lib.ConvLayer * len(stack))(*[_lib.ConvLayer(None, None, w.shape[1], w.shape[0], w.shape[2], 0) for w, _ in stack])
    nws = _lib.load().aligner_conv_stack_workspace_bytes(arr, len(stack), B, T)
    assert (nws != 0) == (kind == "one_call"), nws
    fresh = lambda: encode(x, [(_fresh(w), b.clone()) for w, b in stack])  # noqa: E731
    y0 = encode(x, stack)
    assert _bits_equal(y0, fresh())
    # in place: the version counter moves
    _update(*[t for wb in stack for t in wb])
    y1 = encode(x, stack)
    invalidate_prepared()
    y2 = encode(x, stack)
    torch.cuda.synchronize()
    assert _bits_equal(y1, y2) and _bits_equal(y1, fresh()), "encode() ran on a stale image after an in-place update"
    assert not torch.equal(y1, y0)
    # the documented bypass and its documented remedy
    for w, _ in stack:
        w.data.copy_(w.data * 0.5 - 0.02)
    invalidate_prepared()
    y3 = encode(x, stack)
    torch.cuda.synchronize()
    assert _bits_equal(y3, fresh()), "encode() ran on a stale image after p.data.copy_() + invalidate_prepared()"
    assert not torch.equal(y3, y1)


# ---- (c) aliases ----
def test_detached_alias_sees_the_update(dev):
    x, w, b, gy = _layer(dev, 80, 160, 3)
    before = _fwd_bwd(x, w.detach(), b, gy)
    assert _same(before, _fwd_bwd(x, _fresh(w), b, gy))
    _update(w)
    after = _fwd_bwd(x, w.detach(), b, gy)
    torch.cuda.synchronize()
    assert _same(after, _fwd_bwd(x, _fresh(w), b, gy)), "a detach() alias ran on a stale image"
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


@pytest.mark.parametrize("K", [1, 3])
def test_one_tensor_as_two_layers(dev, K):
    from aligner_amd.softattn import encode
    x, w, b, _ = _layer(dev, 80, 80, K)
    y0 = encode(x, [(w, b), (w, b)])
    assert _bits_equal(y0, encode(x, [(_fresh(w), b), (_fresh(w), b)]))
    _update(w)
    y1 = encode(x, [(w, b), (w, b)])
    torch.cuda.synchronize()
    assert _bits_equal(y1, encode(x, [(_fresh(w), b), (_fresh(w), b)])), "a layer of the shared weight ran on a stale image"
    assert not torch.equal(y1, y0)


def test_slice_of_a_larger_parameter_updated_through_its_base(dev):
    x, w0, b, gy = _layer(dev, 80, 160, 3)
    base = torch.cat([w0 * 2.0, w0, w0 * 3.0]).contiguous()           # [3 Cout, Cin, K]
    w = base[160:320]
    assert w.is_contiguous() and w.data_ptr() != base.data_ptr() and w._base is base
    before = _fwd_bwd(x, w, b, gy)
    assert _same(before, _fwd_bwd(x, _fresh(w0), b, gy))
    _update(base)
    after = _fwd_bwd(x, w, b, gy)
    torch.cuda.synchronize()
    assert _same(after, _fwd_bwd(x, _fresh(base[160:320]), b, gy)), "a slice ran on a stale image after its base moved"
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


# ---- (d) weights that have to be converted ----
def _converted(dev, kind):
    x, w32, b, gy = _layer(dev, 80, 160, 3)
    if kind == "bf16":
        w = w32.bfloat16()
    else:                                                            # every other input channel of a wider tensor
        wide = torch.randn(160, 160, 3, generator=torch.Generator().manual_seed(5)).to(dev) / 16.0
        w = wide[:, ::2, :]
        assert not w.is_contiguous() and w.dtype == torch.float32
    return x, w, b, gy


@pytest.mark.parametrize("kind", ["bf16", "strided"])
def test_converted_weights_give_the_fp32_contiguous_bits_and_follow_updates(dev, kind):
    x, w, b, gy = _converted(dev, kind)
    before = _fwd_bwd(x, w, b, gy)
    assert _same(before, _fwd_bwd(x, _fresh(w), b, gy))
    _update(w)
    after = _fwd_bwd(x, w, b, gy)
    torch.cuda.synchronize()
    assert _same(after, _fwd_bwd(x, _fresh(w), b, gy)), "ran on a stale image of a converted weight"
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


@pytest.mark.parametrize("kind", ["bf16", "strided"])
def test_converted_weights_retain_no_memory_call_after_call(dev, kind):
    """memory_allocated() after the 40th identical call (forward, input gradient, and the same through autograd) equals the
    value after the 3rd: no fp32 copy of the weight, and no image of one, is kept per call."""
    import aligner_amd
    x, w, b, gy = _converted(dev, kind)
    p = w.clone().requires_grad_() if kind == "bf16" else None       # a bf16 parameter, through autograd
    xr = x.clone().requires_grad_()
    seen = {}
    for n in range(1, 41):
        out = _fwd_bwd(x, w, b, gy)
        if p is not None:
            y = aligner_amd.conv1d(xr, p, b, relu=True)
            y.backward(gy)
            assert p.grad.dtype == torch.bfloat16 and xr.grad is not None
            p.grad = xr.grad = None
            del y
        del out
        torch.cuda.synchronize()
        if n in (3, 40):
            seen[n] = torch.cuda.memory_allocated(dev)
    print(f"{kind}: memory_allocated after call 3 {seen[3]}, after call 40 {seen[40]} ({seen[40] - seen[3]:+d} bytes)")
    assert seen[40] == seen[3]


@pytest.mark.parametrize("keep_alive", [True, False])
def test_more_weights_than_the_cache_holds(dev, keep_alive):
    """300 distinct [4,4,1] weights (the tables hold 256), then the first again; with keep_alive False each weight is
    dropped after its call, so the allocator hands its address to a later one.  Every result inside the conv kernels' bound
    (tests/conv_oracle.py: 3 * 2^-16 A for the split products, the fp32 sum of 4 terms well below 2^-16 A more; A = sum
    |w| |x| + |b|), the first weight's second result the bits of its first."""
    import aligner_amd
    from aligner_amd import softattn
    g = torch.Generator().manual_seed(300)
    x = torch.randn(2, 4, 33, generator=g).to(dev)
    ws = torch.randn(300, 4, 4, 1, generator=g).to(dev)
    held, first, worst = [], None, 0.0
    for n in list(range(300)) + [0]:
        w = ws[n].clone()
        y = aligner_amd.conv1d(x, w, None, relu=False)
        want = torch.einsum("oi,bit->bot", w[:, :, 0].double(), x.double())
        A = torch.einsum("oi,bit->bot", w[:, :, 0].double().abs(), x.double().abs())
        worst = max(worst, ((y.double() - want).abs() / (4 * 2.0 ** -16 * A)).max().item())
        if first is None:
            first = y
        if keep_alive:
            held.append(w)
    torch.cuda.synchronize()
    print(f"keep_alive={keep_alive}: largest error / bound over 301 calls {worst:.3f}, table size {len(softattn._prepared)}")
    assert worst <= 1.0
    assert _bits_equal(y, first)
    assert len(softattn._prepared) <= 256


# ---- (e) two streams ----
def test_two_streams_both_see_the_update(dev):
    x, w, b, gy = _layer(dev, 80, 160, 3)
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    sa.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(sa):
        before = _fwd_bwd(x, w, b, gy)
    torch.cuda.synchronize()
    _update(w)
    torch.cuda.synchronize()
    with torch.cuda.stream(sb):
        on_b = _fwd_bwd(x, w, b, gy)
    with torch.cuda.stream(sa):
        on_a = _fwd_bwd(x, w, b, gy)
    torch.cuda.synchronize()
    want = _fwd_bwd(x, _fresh(w), b, gy)
    torch.cuda.synchronize()
    assert _same(on_b, want), "the second stream ran on a stale image"
    assert _same(on_a, want), "the first stream ran on a stale image"
    assert not torch.equal(on_a[0], before[0]) and not torch.equal(on_a[1], before[1])


# ---- (f) a captured graph ----
def test_a_captured_graph_follows_weight_updates(dev):
    """conv1d and conv1d_backward warmed up on the capture stream (the caches are hot), then captured: one side stream, a
    linear graph.  The replay equals the eager run; after an in-place update outside the graph, the replay equals an eager
    run on the new weights, bit for bit -- the graph owns its prepare launches."""
    import aligner_amd
    g = torch.Generator().manual_seed(22)
    x = torch.randn(4, 128, 120, generator=g).to(dev)
    w = (torch.randn(256, 128, 3, generator=g) / 20.0).to(dev)
    bias = torch.randn(256, generator=g).to(dev)
    gy = torch.randn(4, 256, 120, generator=g).to(dev)

    def run(wt):
        y = aligner_amd.conv1d(x, wt, bias, relu=True)
        gx, gw, gb = aligner_amd.conv1d_backward(x, wt, y, gy, True)
        return y, gx, gw, gb

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = run(w)
        run(w)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = run(w)
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(outs, eager)
    _update(w)
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want = run(_fresh(w))
    torch.cuda.synchronize()
    assert not torch.equal(want[0], eager[0]) and not torch.equal(want[1], eager[1])
    assert _same(outs, want), "the replay ran on the image of the weights it was captured with"
    # and the eager path after the capture: its cache entry is its own
    assert _same(run(w), want)
