"""Soft-attention front end (OTA-style alignment encoder) on the HIP path.

Build-defined spec (the reference snapshot only links the paper,
README.md:50):

    K = Conv1d(C_text -> 2 C_text, k=3) -> ReLU -> Conv1d(2 C_text -> C_att, k=1)      text [B,C_text,T_text]
    Q = Conv1d(C_mel -> 2 C_mel, k=3) -> ReLU -> Conv1d(2 C_mel -> C_mel, k=1) -> ReLU
          -> Conv1d(C_mel -> C_att, k=1)                                                mel  [B,C_mel,T_mel]
    logit[b,i,j] = -temperature * sum_c (Q[b,c,j] - K[b,c,i])^2
    logp = log_softmax over the text axis i (+ log(prior + 1e-8));  layout [B,T_text,T_mel]
    hard = maximum_path(logp, mask)

All arithmetic runs in libaligner_amd.so; torch only owns the buffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._operands import f32c, ptr, stream


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    return f32c(t)


def _chk_weight(w: torch.Tensor) -> None:
    if not w.is_cuda:
        raise ValueError("weight must be a GPU tensor")
    if w.dim() != 3:
        raise ValueError("weight must be [Cout,Cin,K]")


_workspaces = _lib.StreamWorkspaces(zero=False)
_conv_workspaces = _lib.StreamWorkspaces(zero=False)      # split activations of the wide conv layers
_prepared: dict = {}          # (weight ptr, dtype, shape, strides, device, stream) -> (version, prepared weights, weight)
_prepared_t: dict = {}        # the same for the transposed weights (the input gradient's convolution)
_bwd_workspaces = _lib.StreamWorkspaces(zero=False)       # the backward passes' column statistics / weight-gradient partials


def _workspace(device, nbytes: int) -> torch.Tensor:
    return _workspaces.get(device, nbytes)             # one per (device, stream)


def _prepared_image(table: dict, weight: torch.Tensor, device, transposed: bool, fresh: bool = False) -> torch.Tensor:
    """The prepared image of `weight` (or of its transpose) from `table`, written when it is missing or stale.

    An entry belongs to the CALLER's tensor: the key is its address, dtype, shape, strides, device and the current stream
    (no cross-stream ordering), the entry records torch's version counter and holds the tensor, so its address is not
    reused while the entry lives.  A weight the kernels cannot read as it is (bf16, a non-contiguous view) is converted for
    the prepare launch alone, once per update: the fp32 copy is dropped again, the cache never sees it.  In-place updates
    (optimizers, `p.sub_()`, through a view or `detach()` alias: one shared counter) move the counter and the image is
    re-prepared into the same buffer, so a training loop does not grow the cache.  Updates that bypass the counter
    (`p.data.copy_()`, EMA through `.data`) are NOT seen: call invalidate_prepared() after them.

    Fused optimizers (`Adam(fused=True)`, `SGD(fused=True)`, ...) update the parameters WITHOUT moving the counter, so the
    image of a weight that is being trained is never trusted: with `fresh` (the autograd path, when the weight gets a
    gradient) or `weight.requires_grad` the image is prepared again on every call, into the entry's buffer.  Only an alias
    of such a parameter that does not require grad itself (`p.detach()`) still needs invalidate_prepared() after a fused step.

    While the stream is capturing, the cache is neither read nor written: the image is prepared into a buffer allocated
    inside the capture, so the graph owns its prepare launch and its image, and every replay reads the weights as they are
    then (a cached image would freeze the weights of capture time into the graph, and could be evicted under it)."""
    lib = _lib.load()
    Cout, Cin, K = weight.shape
    nprep = lib.aligner_conv1d_prepared_bytes(Cin, Cout, K) if transposed else lib.aligner_conv1d_prepared_bytes(Cout, Cin, K)
    if nprep == 0:
        raise ValueError(f"kernel size {K} not supported (1, 3, 5)")
    prepare = lib.aligner_conv1d_prepare_transposed_f32 if transposed else lib.aligner_conv1d_prepare_f32
    if torch.cuda.is_current_stream_capturing():
        prep = torch.empty(nprep, dtype=torch.uint8, device=device)
        wf = f32c(weight)
        _lib.check(prepare(wf.data_ptr(), prep.data_ptr(), nprep, Cout, Cin, K, stream(device)))
        return prep
    key = (weight.data_ptr(), weight.dtype, tuple(weight.shape), tuple(weight.stride()), device, stream(device))
    ent = table.get(key)
    if ent is not None and ent[0] == weight._version and not (fresh or weight.requires_grad):
        return ent[1]
    prep = ent[1] if ent is not None else torch.empty(nprep, dtype=torch.uint8, device=device)
    wf = f32c(weight)                                  # a copy only for bf16 / strided weights, dropped on return
    _lib.check(prepare(wf.data_ptr(), prep.data_ptr(), nprep, Cout, Cin, K, stream(device)))
    if ent is None and len(table) >= 256:
        table.pop(next(iter(table)))                   # oldest entry only
    table[key] = (weight._version, prep, weight)
    return prep


def _prepared_weights(weight: torch.Tensor, device, fresh: bool = False) -> torch.Tensor:
    """weights -> split bf16 halves in the matrix cores' fragment order (aligner_conv1d_prepare_f32, a few
    microseconds), cached per weight tensor: _prepared_image()."""
    return _prepared_image(_prepared, weight, device, False, fresh)


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def conv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """y = act(conv1d(x, weight, bias, padding=K//2)); x [B,Cin,T], weight [Cout,Cin,K], K in {1,3,5}.
    Differentiable (conv1d_backward()) when grad is enabled and x, weight or bias requires grad."""
    if _needs_grad(x, weight, bias):
        return _Conv1d.apply(x, weight, bias, relu)
    return _conv1d(x, weight, bias, relu)


def _conv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool, fresh: bool = False) -> torch.Tensor:
    _lib.require_gpu()
    x = _chk(x, "x"); _chk_weight(weight)              # the weight stays the caller's tensor: the cache is keyed on it
    bias = _chk(bias, "bias") if bias is not None else None
    B, Cin, T = x.shape
    Cout, Cin2, K = weight.shape
    if Cin2 != Cin:
        raise ValueError("channel mismatch")
    y = torch.empty((B, Cout, T), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        prep = _prepared_weights(weight, x.device, fresh)
        # wide layers split their activations into a workspace first (csrc/convgemm.hip); narrow ones need none
        nws = lib.aligner_conv1d_workspace_bytes(B, Cin, Cout, T, K)
        ws = _conv_workspaces.get(x.device, nws) if nws else None
        _lib.check(lib.aligner_conv1d_prepared_ws_f32(x.data_ptr(), prep.data_ptr(),
                                                      ptr(bias), y.data_ptr(), ptr(ws), nws,
                                                      B, Cin, Cout, T, K, int(relu), stream(x.device)))
    return y


def _prepared_weights_transposed(weight: torch.Tensor, device, fresh: bool = False) -> torch.Tensor:
    """The prepared image of w'[i,o,k] = w[o,i,K-1-k] (aligner_conv1d_prepare_transposed_f32): the input gradient of the
    layer is the forward convolution of its output gradient with it.  Cached like _prepared_weights(), in a table of its
    own."""
    return _prepared_image(_prepared_t, weight, device, True, fresh)


def conv1d_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, relu: bool,
                    need_x: bool = True, need_w: bool = True, need_b: bool = True, _fresh: bool = False
                    ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Gradients of y = act(conv1d(x, weight, bias)) (act = ReLU when relu) given grad_y = dL/dy: (grad_x [B,Cin,T],
    grad_w [Cout,Cin,K], grad_b [Cout]), fp32, None where not asked for.  y (the layer's output) is needed with relu only.
    The ReLU mask is torch.relu's: the cotangent is 0 where y <= 0 and passes elsewhere, so a NaN y passes it (a NaN
    cotangent at a NaN activation reaches grad_w / grad_b, where a gradient scaler's overflow check looks for it).
    grad_w / grad_b: aligner_conv1d_backward_weight_f32; grad_x: the forward convolution of the masked grad_y with the
    transposed weights (aligner_conv1d_prepare_transposed_f32 + aligner_conv1d_prepared_ws_f32)."""
    _lib.require_gpu()
    x = _chk(x, "x"); _chk_weight(weight); gy = _chk(grad_y, "grad_y")
    B, Cin, T = x.shape
    Cout, Cin2, K = weight.shape
    if Cin2 != Cin or tuple(gy.shape) != (B, Cout, T):
        raise ValueError("shape mismatch")
    if relu:
        if y is None:
            raise ValueError("relu needs the layer's output y")
        y = _chk(y, "y")
        if tuple(y.shape) != (B, Cout, T):
            raise ValueError("y must be [B,Cout,T]")
    dev = x.device
    lib = _lib.load()
    gx = gw = gb = None
    with torch.cuda.device(dev):
        gyp = gy
        if relu and need_x:
            gyp = torch.empty_like(gy)
        if need_w:
            gw = torch.empty((Cout, Cin, K), dtype=torch.float32, device=dev)
        if need_b:
            gb = torch.empty((Cout,), dtype=torch.float32, device=dev)
        if need_w or need_b or (relu and need_x):
            nws = lib.aligner_conv1d_backward_workspace_bytes(B, Cin, Cout, T, K)
            ws = _bwd_workspaces.get(dev, nws) if (need_w or need_b) and nws else None
            _lib.check(lib.aligner_conv1d_backward_weight_f32(
                x.data_ptr(), y.data_ptr() if relu else None, gy.data_ptr(), gyp.data_ptr() if (relu and need_x) else None,
                ptr(gw), ptr(gb), ptr(ws), 0 if ws is None else ws.numel(), B, Cin, Cout, T, K, int(relu), stream(dev)))
        if need_x:
            prep = _prepared_weights_transposed(weight, dev, _fresh)
            gx = torch.empty((B, Cin, T), dtype=torch.float32, device=dev)
            nws = lib.aligner_conv1d_workspace_bytes(B, Cout, Cin, T, K)
            ws = _conv_workspaces.get(dev, nws) if nws else None
            _lib.check(lib.aligner_conv1d_prepared_ws_f32(gyp.data_ptr(), prep.data_ptr(), None, gx.data_ptr(),
                                                          ptr(ws), nws, B, Cout, Cin, T, K, 0, stream(dev)))
    return gx, gw, gb


class _Conv1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        ctx.set_materialize_grads(False)
        xf = _chk(x, "x")
        y = _conv1d(xf, weight, bias, relu, fresh=ctx.needs_input_grad[1])     # a weight in training: never a cached image
        ctx.relu = relu
        ctx.dtypes = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(xf, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return None, None, None, None
        x, w, y = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        gx, gw, gb = conv1d_backward(x, w, y, gy, ctx.relu, need_x=nx, need_w=nw, need_b=nb, _fresh=nw)
        dx, dw, db = ctx.dtypes
        return (None if gx is None else gx.to(dx), None if gw is None else gw.to(dw), None if gb is None else gb.to(db), None)


def invalidate_prepared() -> None:
    """Drop every prepared (split-bf16) weight image: call after weight updates that bypass torch's version
    counter (`p.data.copy_()`, EMA through `.data`, writes through a storage alias)."""
    _prepared.clear()
    _prepared_t.clear()


def soft_attention(keys_enc: torch.Tensor, queries_enc: torch.Tensor, t_x: Optional[torch.Tensor] = None,
                   prior: Optional[torch.Tensor] = None, temperature: float = 0.0005, sim: str = "l2",
                   want_soft: bool = False, out: Optional[torch.Tensor] = None,
                   logp_dtype: torch.dtype = torch.float32, pitched: bool = False
                   ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """logp[b,i,j] (and optionally softmax over text of it) from encoded text/mel.

    pitched: return the log-probs as a [B,T_text,T_mel] VIEW of a buffer whose rows start on whole 128-byte lines
    (pitched_logp(): what align() reads fastest; not contiguous unless T_mel already is a multiple of 128 bytes) where
    the kernel form has a row pitch of its own, contiguous otherwise.

    keys_enc [B,C,T_text], queries_enc [B,C,T_mel] fp32 (channel-major, as the conv
    encoders emit).  Rows i >= t_x[b] are masked to -inf.  logp_dtype torch.bfloat16 writes the log-probs as
    bf16 (half the traffic; align() / maximum_path() read them as they are).

    Differentiable in keys_enc / queries_enc (soft_attention_backward(), through logp and soft) when grad is enabled and
    either requires grad; the prior gets no gradient (a prior that requires grad, and `out`, are refused then)."""
    if _needs_grad(keys_enc, queries_enc) or (torch.is_grad_enabled() and prior is not None and prior.requires_grad):
        if out is not None:
            raise ValueError("out= is not supported with autograd (keys_enc / queries_enc require grad)")
        if prior is not None and prior.requires_grad:
            raise ValueError("the prior gets no gradient: pass prior.detach()")
        if logp_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("logp_dtype must be torch.float32 or torch.bfloat16")
        logp, soft = _SoftAttention.apply(keys_enc, queries_enc, t_x, prior, float(temperature), sim, want_soft, logp_dtype,
                                          pitched)
        return logp, soft
    return _soft_attention(keys_enc, queries_enc, t_x, prior, temperature, sim, want_soft, out, logp_dtype, pitched)


def _soft_attention(keys_enc, queries_enc, t_x, prior, temperature, sim, want_soft, out, logp_dtype, pitched):
    _lib.require_gpu()
    k = _chk(keys_enc, "keys_enc"); q = _chk(queries_enc, "queries_enc")
    B, C, Tx = k.shape
    B2, C2, Ty = q.shape
    if B != B2 or C != C2:
        raise ValueError("keys/queries shape mismatch")
    dev = k.device
    if t_x is not None:
        t_x = t_x.to(device=dev, dtype=torch.int32).contiguous()
    if prior is not None:
        prior = _chk(prior, "prior")
        if tuple(prior.shape) != (B, Tx, Ty):
            raise ValueError("prior must be [B,T_text,T_mel]")
    if out is not None:
        logp_dtype = out.dtype
    if logp_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("logp_dtype must be torch.float32 or torch.bfloat16")
    if out is None and pitched and prior is None and not want_soft and Tx <= 224 and C in (80, 128) and Ty % 4 == 0:
        try:
            return _soft_attention(k, q, t_x, None, temperature, sim, False, pitched_logp(B, Tx, Ty, dev, logp_dtype), logp_dtype,
                                   False)
        except _lib.AlignerError as e:          # (a sharp temperature: the exact-product kernel has no row pitch)
            if e.code != _lib.EDOM:
                raise
    logp = out if out is not None else torch.empty((B, Tx, Ty), dtype=logp_dtype, device=dev)
    # `out` may carry a row pitch of its own (a view [:, :, :T_mel] of a [B,T_text,ld] buffer: pitched_logp())
    ld = Ty
    if tuple(logp.shape) == (B, Tx, Ty):
        ld = int(logp.stride(1)) if Tx > 1 else int(logp.stride(0)) if B > 1 else Ty
    if tuple(logp.shape) != (B, Tx, Ty) or logp.stride(2) != 1 or ld < Ty or (B > 1 and logp.stride(0) != Tx * ld):
        raise ValueError("out must be a [B,T_text,T_mel] tensor, contiguous or with a row pitch (pitched_logp())")
    soft = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_soft else None
    simc = {"l2": _lib.SIM_L2, "dot": _lib.SIM_DOT}[sim]
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _workspace(dev, lib.aligner_softattn_workspace_bytes(B, C, Tx))
        _lib.check(lib.aligner_softattn_ld(
            k.data_ptr(), q.data_ptr(), ptr(t_x), ptr(prior), logp.data_ptr(),
            _lib.DT_BF16 if logp_dtype == torch.bfloat16 else _lib.DT_F32, ld,
            ptr(soft), ws.data_ptr(), ws.numel(), B, C, Tx, Ty, float(temperature), simc, stream(dev)))
    return logp, soft


def soft_attention_backward(keys_enc: torch.Tensor, queries_enc: torch.Tensor, grad_logp: torch.Tensor,
                            t_x: Optional[torch.Tensor] = None, prior: Optional[torch.Tensor] = None,
                            temperature: float = 0.0005, sim: str = "l2", grad_soft: Optional[torch.Tensor] = None,
                            need_keys: bool = True, need_queries: bool = True
                            ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Gradients of soft_attention()'s logp (and soft) w.r.t. keys_enc [B,C,T_text] and queries_enc [B,C,T_mel], given
    grad_logp = dL/dlogp and optionally grad_soft = dL/dsoft ([B,T_text,T_mel]) and the forward's own t_x / prior /
    temperature / sim (aligner_softattn_backward_f32: the logits are recomputed, not read).  Returns (grad_keys,
    grad_queries) in fp32, None where not asked for.  Masked rows get a zero gradient; the prior gets none."""
    _lib.require_gpu()
    if not (need_keys or need_queries):
        return None, None
    k = _chk(keys_enc, "keys_enc"); q = _chk(queries_enc, "queries_enc")
    B, C, Tx = k.shape
    B2, C2, Ty = q.shape
    if B != B2 or C != C2:
        raise ValueError("keys/queries shape mismatch")
    gl = _chk(grad_logp, "grad_logp")
    if tuple(gl.shape) != (B, Tx, Ty):
        raise ValueError("grad_logp must be [B,T_text,T_mel]")
    gs = None
    if grad_soft is not None:
        gs = _chk(grad_soft, "grad_soft")
        if tuple(gs.shape) != (B, Tx, Ty):
            raise ValueError("grad_soft must be [B,T_text,T_mel]")
    dev = k.device
    if t_x is not None:
        t_x = t_x.to(device=dev, dtype=torch.int32).contiguous()
    if prior is not None:
        prior = _chk(prior, "prior")
        if tuple(prior.shape) != (B, Tx, Ty):
            raise ValueError("prior must be [B,T_text,T_mel]")
    simc = {"l2": _lib.SIM_L2, "dot": _lib.SIM_DOT}[sim]
    gk = torch.empty((B, C, Tx), dtype=torch.float32, device=dev) if need_keys else None
    gq = torch.empty((B, C, Ty), dtype=torch.float32, device=dev) if need_queries else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _bwd_workspaces.get(dev, lib.aligner_softattn_backward_workspace_bytes(B, C, Tx, Ty))
        _lib.check(lib.aligner_softattn_backward_f32(
            k.data_ptr(), q.data_ptr(), ptr(t_x), ptr(prior), gl.data_ptr(), ptr(gs), ptr(gk), ptr(gq),
            ws.data_ptr(), ws.numel(), B, C, Tx, Ty, float(temperature), simc, stream(dev)))
    return gk, gq


class _SoftAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keys_enc, queries_enc, t_x, prior, temperature, sim, want_soft, logp_dtype, pitched):
        ctx.set_materialize_grads(False)
        k, q = _chk(keys_enc, "keys_enc"), _chk(queries_enc, "queries_enc")
        if prior is not None:
            prior = _chk(prior, "prior")
        logp, soft = _soft_attention(k, q, t_x, prior, temperature, sim, want_soft, None, logp_dtype, pitched)
        ctx.temperature, ctx.sim = temperature, sim
        ctx.dtypes = (keys_enc.dtype, queries_enc.dtype)
        ctx.save_for_backward(k, q, t_x if isinstance(t_x, torch.Tensor) else None, prior)
        return logp, soft

    @staticmethod
    def backward(ctx, g_logp, g_soft):
        nk, nq = ctx.needs_input_grad[:2]
        if (g_logp is None and g_soft is None) or not (nk or nq):
            return (None,) * 9
        k, q, t_x, prior = ctx.saved_tensors
        if g_logp is None:
            g_logp = torch.zeros((k.shape[0], k.shape[2], q.shape[2]), dtype=torch.float32, device=k.device)
        gk, gq = soft_attention_backward(k, q, g_logp, t_x=t_x, prior=prior, temperature=ctx.temperature, sim=ctx.sim,
                                         grad_soft=g_soft, need_keys=nk, need_queries=nq)
        dk, dq = ctx.dtypes
        return (None if gk is None else gk.to(dk), None if gq is None else gq.to(dq)) + (None,) * 7


def pitched_logp(B: int, T_text: int, T_mel: int, device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """A [B,T_text,T_mel] tensor whose rows start on 128-byte lines (row pitch = T_mel rounded up to 128 bytes): the
    pipeline's own intermediate between soft_attention(out=...) and align().  With T_mel = 1000 fp32 a row is 4000 bytes and
    three quarters of the 128-byte runs the similarity kernel stores (and the search's loaders fetch) straddle two lines; at a
    pitch of 1024 elements none does.  The extra columns are never touched."""
    per = 128 // torch.empty((), dtype=dtype).element_size()
    ld = (T_mel + per - 1) // per * per
    return torch.empty((B, T_text, ld), dtype=dtype, device=device)[:, :, :T_mel]


@dataclass
class AlignmentEncoderParams:
    """Weights of the two conv stacks: lists of (weight [Cout,Cin,K], bias [Cout])."""
    key_proj: List[Tuple[torch.Tensor, torch.Tensor]]
    query_proj: List[Tuple[torch.Tensor, torch.Tensor]]
    temperature: float = 0.0005

    @staticmethod
    def random(c_text: int, c_mel: int, c_att: int, device, seed: int = 0) -> "AlignmentEncoderParams":
        g = torch.Generator(device="cpu").manual_seed(seed)

        def layer(co, ci, k):
            bound = (1.0 / (ci * k)) ** 0.5
            w = (torch.rand((co, ci, k), generator=g) * 2 - 1) * bound
            b = (torch.rand((co,), generator=g) * 2 - 1) * bound
            return w.to(device), b.to(device)

        return AlignmentEncoderParams(
            key_proj=[layer(2 * c_text, c_text, 3), layer(c_att, 2 * c_text, 1)],
            query_proj=[layer(2 * c_mel, c_mel, 3), layer(c_mel, 2 * c_mel, 1), layer(c_att, c_mel, 1)],
        )


def encode(x: torch.Tensor, stack: List[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
    """A conv stack (ReLU between the layers) -- in ONE call of the C ABI when every layer has a GEMM form
    (aligner_conv_stack_f32: the input is split once, every k = 1 layer reads the split image its producer wrote; no fp32
    round trip between layers), layer by layer otherwise.  With grad (x or a weight / bias requires grad) always layer by
    layer through the differentiable conv1d(), which keeps each layer's input and output for the backward."""
    if _needs_grad(x, *[t for wb in stack for t in wb]):
        for n, (w, b) in enumerate(stack):
            x = conv1d(x, w, b, relu=(n + 1 < len(stack)))
        return x
    _lib.require_gpu()
    lib = _lib.load()
    x = _chk(x, "x")
    B, Cin, T = x.shape
    dev = x.device
    layers = (_lib.ConvLayer * len(stack))()
    keep = []
    c = Cin
    with torch.cuda.device(dev):
        for n, (w, b) in enumerate(stack):
            _chk_weight(w)
            b = _chk(b, "bias") if b is not None else None
            if w.shape[1] != c:
                raise ValueError("channel mismatch")
            prep = _prepared_weights(w, dev)
            keep += [w, b, prep]
            layers[n] = _lib.ConvLayer(prep.data_ptr(), ptr(b), int(w.shape[1]), int(w.shape[0]),
                                       int(w.shape[2]), int(n + 1 < len(stack)))
            c = int(w.shape[0])
        nws = lib.aligner_conv_stack_workspace_bytes(layers, len(stack), B, T) if B > 0 and len(stack) > 0 else 0
        if nws:
            y = torch.empty((B, c, T), dtype=torch.float32, device=dev)
            ws = _conv_workspaces.get(dev, nws)
            _lib.check(lib.aligner_conv_stack_f32(x.data_ptr(), layers, len(stack), y.data_ptr(), ws.data_ptr(), nws, B, T,
                                                  stream(dev)))
            return y
    for n, (w, b) in enumerate(stack):
        x = conv1d(x, w, b, relu=(n + 1 < len(stack)))
    return x


def alignment_encoder(text_emb: torch.Tensor, mel: torch.Tensor, params: AlignmentEncoderParams,
                      t_x: Optional[torch.Tensor] = None, prior: Optional[torch.Tensor] = None,
                      want_soft: bool = False, pitched: bool = False):
    """text_emb [B,C_text,T_text], mel [B,C_mel,T_mel] -> (logp [B,T_text,T_mel], soft or None).  pitched: see soft_attention().
    Differentiable in the inputs and every weight / bias of `params` that requires grad (encode(), soft_attention())."""
    k = encode(text_emb, params.key_proj)
    q = encode(mel, params.query_proj)
    return soft_attention(k, q, t_x=t_x, prior=prior, temperature=params.temperature, want_soft=want_soft, pitched=pitched)
