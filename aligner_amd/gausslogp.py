"""Glow-TTS / VITS log-likelihood front end on the HIP path (csrc/gausslogp.hip).

Both models search the alignment on the log-density of every latent frame under every token's diagonal Gaussian,

    value[b,i,j] = sum_c ( -1/2 ln 2pi - s[b,c,i] - 1/2 (z[b,c,j] - m[b,c,i])^2 exp(-2 s[b,c,i]) )

with m, s [B,C,T_text] the text encoder's mean and log-std and z [B,C,T_mel] the flow's output, computed under no_grad
(the loss goes through the expanded m and s: regulate()).  gaussian_logp() is that tensor in one fused kernel;
gaussian_align() is the whole `logp = ...; attn = maximum_path(logp, mask)` block of a training step.

Models that train the tensor softly (AlignTTS's mixture-density loss, soft-alignment variants of Glow-TTS / VITS) need
its gradient: gaussian_logp_backward() is the vector-Jacobian product (csrc/gausslogp_bwd.hip),
gaussian_logp(differentiable=True) attaches it to autograd, and gaussian_forward_sum_loss() is the marginal likelihood
over all monotonic alignments of the Gaussian scores as one autograd function.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._operands import f32c, gaussian_shapes, lengths, one_gpu, per_utterance, ptr, stream
from .maxpath import Alignment, align
from .objective import forward_sum
from .softattn import pitched_logp

_workspaces = _lib.StreamWorkspaces(zero=False)


def gaussian_logp(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, t_x: Optional[torch.Tensor] = None,
                  t_y: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
                  out_dtype: torch.dtype = torch.float32, pitched: bool = False,
                  differentiable: bool = False) -> torch.Tensor:
    """value[b,i,j] = log N(z[b,:,j]; mean[b,:,i], exp(logstd[b,:,i])^2), [B,T_text,T_mel].

    z [B,C,T_mel], mean and logstd [B,C,T_text]: GPU tensors, channel-major as both models hold them (other dtypes than
    fp32 are cast, non-contiguous ones copied).  t_x / t_y [B]: cells with i >= t_x[b] or j >= t_y[b] are written as 0.0
    (Glow-TTS's `logp * attn_mask`); None = the full extent.  out_dtype torch.bfloat16 rounds the fp32 result to bf16 (half
    the traffic; align() / maximum_path() read it as it is).  pitched: return a [B,T_text,T_mel] VIEW of a buffer whose
    rows start on whole 128-byte lines (pitched_logp(): what align() reads fastest).  out: write into the caller's
    tensor, contiguous or such a view (its dtype decides); the columns >= T_mel of a pitched buffer are never touched.
    No gradient by default: the result never requires grad.  differentiable=True: when z, mean or logstd requires grad
    the result is attached to autograd (the same forward kernel; the three inputs are saved, not the value; backward is
    gaussian_logp_backward() for the inputs that need it, gradients in each input's dtype); out_dtype must then be fp32
    and `out` is refused.  Asynchronous on the current stream."""
    if differentiable:
        if out is not None:
            raise ValueError("differentiable=True cannot write into `out`")
        if out_dtype != torch.float32:
            raise ValueError("differentiable=True needs out_dtype torch.float32")
        if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (z, mean, logstd)) and torch.is_grad_enabled():
            return _GaussianLogp.apply(z, mean, logstd, t_x, t_y, pitched)
    B, C, Tx, Ty = gaussian_shapes(z, mean, logstd)
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("out_dtype must be torch.float32 or torch.bfloat16")
    ld = Ty
    if out is not None:
        # `out` may carry a row pitch of its own (a view [:, :, :T_mel] of a [B,T_text,ld] buffer: pitched_logp())
        if tuple(out.shape) == (B, Tx, Ty):
            ld = int(out.stride(1)) if Tx > 1 else int(out.stride(0)) if B > 1 else Ty
        if (tuple(out.shape) != (B, Tx, Ty) or (Ty > 1 and out.stride(2) != 1) or ld < Ty or (B > 1 and out.stride(0) != Tx * ld)
                or (ld != Ty and (ld * out.element_size()) % 16 != 0)):
            raise ValueError("out must be a [B,T_text,T_mel] tensor, contiguous or with a row pitch (pitched_logp())")
    dev = one_gpu(((z, "z"), (mean, "mean"), (logstd, "logstd")), "z, mean, logstd and out")
    if out is not None and out.device != dev:
        raise ValueError("z, mean, logstd and out must be on the same device")
    per_utterance(t_x, B, "t_x")
    per_utterance(t_y, B, "t_y")
    _lib.require_gpu()
    with torch.no_grad(), torch.cuda.device(dev):
        zc, mc, sc = f32c(z), f32c(mean), f32c(logstd)
        t_x, t_y = lengths(t_x, B, dev, "t_x"), lengths(t_y, B, dev, "t_y")
        if out is None:
            out = pitched_logp(B, Tx, Ty, dev, out_dtype) if pitched else torch.empty((B, Tx, Ty), dtype=out_dtype, device=dev)
            if pitched:
                per = 128 // out.element_size()
                ld = (Ty + per - 1) // per * per               # pitched_logp()'s row pitch
        if B == 0 or Tx == 0 or Ty == 0:
            return out
        lib = _lib.load()
        nws = lib.aligner_gauss_logp_workspace_bytes(B, C, Tx)
        ws = _workspaces.get(dev, max(nws, 1))
        _lib.check(lib.aligner_gauss_logp(
            zc.data_ptr(), mc.data_ptr(), sc.data_ptr(), ptr(t_x), ptr(t_y), out.data_ptr(),
            _lib.DT_BF16 if out_dtype == torch.bfloat16 else _lib.DT_F32, ld, ws.data_ptr(), ws.numel(),
            B, C, Tx, Ty, stream(dev)))
    return out


def gaussian_align(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor, *,
                   logp_dtype: torch.dtype = torch.float32, **align_kwargs) -> Alignment:
    """The Glow-TTS / VITS step's `with torch.no_grad(): logp = ...; attn = maximum_path(logp, mask)` in one call:
    gaussian_logp() into the pipeline's own pitched intermediate (pitched_logp(), logp_dtype fp32 or bf16), then align()
    on it with the same lengths; align_kwargs go to align() (path_dtype, want_tok, want_durations, ...).  Returns its
    Alignment(path, tok, durations)."""
    if t_x is None or t_y is None:
        raise ValueError("gaussian_align needs the lengths t_x and t_y")
    logp = gaussian_logp(z, mean, logstd, t_x, t_y, out_dtype=logp_dtype, pitched=True)
    return align(logp, t_x, t_y, **align_kwargs)


def _grad_layout(g: torch.Tensor, B: int, Tx: int, Ty: int):
    """grad_value as the kernel reads it: (fp32 tensor, row pitch).  Contiguous, or pitched_logp()'s view, is read in
    place; anything else is copied."""
    g = g.detach()
    if g.dtype == torch.float32 and g.stride(2) == 1 and Ty > 1 and Tx > 1:
        ld = int(g.stride(1))
        if ld >= Ty and (B == 1 or g.stride(0) == Tx * ld) and (ld == Ty or (ld * 4) % 16 == 0):
            return g, ld
    return g.float().contiguous(), Ty


def gaussian_logp_backward(grad_value: torch.Tensor, z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor,
                           t_x: Optional[torch.Tensor] = None, t_y: Optional[torch.Tensor] = None, *,
                           grad_scale: Optional[torch.Tensor] = None, need_z: bool = True, need_mean: bool = True,
                           need_logstd: bool = True):
    """The vector-Jacobian product of gaussian_logp(): (dz [B,C,T_mel], dmean, dlogstd [B,C,T_text]) for the cotangent
    grad_value [B,T_text,T_mel] (fp32; contiguous or at pitched_logp()'s row pitch, read in place), fp32, None where
    need_* is False.  t_x / t_y as in the forward: cells outside the lengths contribute nothing (whatever grad_value
    holds there), frames >= t_y and tokens >= t_x get 0.0.  grad_scale [B]: grad_value[b] is read as
    grad_scale[b] * grad_value[b] (forward_sum()'s stored gradient with a per-utterance cotangent, no scaling pass).
    Deterministic (no atomics).  Asynchronous on the current stream."""
    B, C, Tx, Ty = gaussian_shapes(z, mean, logstd, also=((grad_value, "grad_value must be a [B,T_text,T_mel] tensor"),))
    if tuple(grad_value.shape) != (B, Tx, Ty):
        raise ValueError(f"grad_value {tuple(grad_value.shape)} must be [B,T_text,T_mel] = {(B, Tx, Ty)}")
    if not (need_z or need_mean or need_logstd):
        raise ValueError("at least one of need_z, need_mean, need_logstd must be set")
    dev = one_gpu(((grad_value, "grad_value"), (z, "z"), (mean, "mean"), (logstd, "logstd")), "grad_value, z, mean and logstd")
    for t, name in ((t_x, "t_x"), (t_y, "t_y"), (grad_scale, "grad_scale")):
        per_utterance(t, B, name)
    _lib.require_gpu()
    with torch.no_grad(), torch.cuda.device(dev):
        zc, mc, sc = f32c(z), f32c(mean), f32c(logstd)
        g, ld = _grad_layout(grad_value, B, Tx, Ty)
        t_x, t_y = lengths(t_x, B, dev, "t_x"), lengths(t_y, B, dev, "t_y")
        if grad_scale is not None:
            grad_scale = grad_scale.detach().to(device=dev, dtype=torch.float32).contiguous()
        dz = torch.empty((B, C, Ty), dtype=torch.float32, device=dev) if need_z else None
        dm = torch.empty((B, C, Tx), dtype=torch.float32, device=dev) if need_mean else None
        ds = torch.empty((B, C, Tx), dtype=torch.float32, device=dev) if need_logstd else None
        if B == 0 or Tx == 0 or Ty == 0:
            for t in (dz, dm, ds):
                if t is not None:
                    t.zero_()
            return dz, dm, ds
        lib = _lib.load()
        nws = lib.aligner_gauss_logp_backward_workspace_bytes(B, C, Tx, Ty)
        ws = _workspaces.get(dev, max(nws, 1))
        _lib.check(lib.aligner_gauss_logp_backward_f32(
            g.data_ptr(), ld, ptr(grad_scale), zc.data_ptr(), mc.data_ptr(), sc.data_ptr(), ptr(t_x), ptr(t_y),
            ptr(dz), ptr(dm), ptr(ds), ws.data_ptr(), ws.numel(), B, C, Tx, Ty, stream(dev)))
    return dz, dm, ds


def _typed(t: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    return None if t is None else t.to(like.dtype)


class _GaussianLogp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, mean, logstd, t_x, t_y, pitched):
        ctx.save_for_backward(z, mean, logstd)              # the inputs only: the value is not needed for its gradient
        ctx.lengths = (t_x, t_y)
        return gaussian_logp(z, mean, logstd, t_x, t_y, pitched=pitched)

    @staticmethod
    def backward(ctx, g):
        z, mean, logstd = ctx.saved_tensors
        nz, nm, ns = ctx.needs_input_grad[:3]
        if g is None or not (nz or nm or ns):
            return None, None, None, None, None, None
        t_x, t_y = ctx.lengths
        dz, dm, ds = gaussian_logp_backward(g, z, mean, logstd, t_x, t_y, need_z=nz, need_mean=nm, need_logstd=ns)
        return _typed(dz, z), _typed(dm, mean), _typed(ds, logstd), None, None, None


class _GaussianForwardSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, mean, logstd, t_x, t_y, blank_logprob, zero_infinity):
        need = any(ctx.needs_input_grad[:3])
        value = gaussian_logp(z, mean, logstd, t_x, t_y)
        loss, grad = forward_sum(value, t_x, t_y, want_grad=need, blank_logprob=blank_logprob)
        del value
        if zero_infinity:
            dead = torch.isinf(loss)
            loss = torch.where(dead, torch.zeros_like(loss), loss)
            # an utterance without an alignment: zero gradients whatever forward_sum left in its block of G
            t_x = torch.where(dead, torch.zeros_like(dead, dtype=torch.int32),
                              torch.as_tensor(t_x).to(device=loss.device, dtype=torch.int32))
        if need:
            ctx.save_for_backward(z, mean, logstd, grad)    # z, m, s and G: no other [B,T_text,T_mel] tensor is kept
        ctx.lengths = (t_x, t_y)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        nz, nm, ns = ctx.needs_input_grad[:3]
        if g_loss is None or not (nz or nm or ns):
            return (None,) * 7
        z, mean, logstd, grad = ctx.saved_tensors
        t_x, t_y = ctx.lengths
        dz, dm, ds = gaussian_logp_backward(grad, z, mean, logstd, t_x, t_y, grad_scale=g_loss.reshape(-1),
                                            need_z=nz, need_mean=nm, need_logstd=ns)
        return _typed(dz, z), _typed(dm, mean), _typed(ds, logstd), None, None, None, None


def gaussian_forward_sum_loss(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, t_x: torch.Tensor,
                              t_y: torch.Tensor, *, blank_logprob: Optional[float] = None, reduction: str = "mean",
                              zero_infinity: bool = False, length_normalize: bool = False) -> torch.Tensor:
    """-log of the likelihood of z summed over ALL monotonic alignments of the tokens' Gaussians -- AlignTTS's
    mixture-density alignment loss (blank_logprob=None, the plain monotonic form), the soft replacement or warm start of
    the hard search in Glow-TTS / VITS -- as one autograd function: gaussian_logp() -> forward_sum() forward, one
    gaussian_logp_backward() backward whose grad_scale carries the per-utterance cotangent (the incoming gradient, the
    1/B of "mean", 1/t_x with length_normalize, 0 for an utterance zeroed by zero_infinity).  Only z, mean, logstd and
    forward_sum's gradient tensor are kept for backward.  The options are forward_sum_loss()'s; gradients come back in
    each input's dtype."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    if t_x is None or t_y is None:
        raise ValueError("gaussian_forward_sum_loss needs the lengths t_x and t_y")
    loss = _GaussianForwardSum.apply(z, mean, logstd, t_x, t_y, blank_logprob, bool(zero_infinity))
    if length_normalize:
        loss = loss / torch.as_tensor(t_x).to(device=loss.device, dtype=loss.dtype).clamp_min(1)
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss
