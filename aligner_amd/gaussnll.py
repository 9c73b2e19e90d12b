"""Glow-TTS / VITS likelihood loss on the hard path (csrc/gaussnll.hip): what those models train on once
gaussian_align() has found the durations.

Token x of utterance b owns the frames ends[x-1] <= y < ends[x], ends = cumsum(max(durations[b], 0)) -- the segments of
regulate(); a frame counts when it has an owner, y < T_mel and y < t_y[b].  With w = exp(-2 s[b,c,x]) and
d = z[b,c,y] - m[b,c,x] on a counting frame,

    nll[b]   = sum over the counting frames and the channels of ( 1/2 ln 2pi + s[b,c,x] + 1/2 d^2 w )
    count[b] = number of counting frames

and the gradient goes to the flow's output z, the text encoder's mean m and its log-std s.  gaussian_nll() is the raw
call, gaussian_nll_loss() its autograd face.  Glow-TTS's loss is sum(nll) / (C sum(count)) (reduction="mean").  A VITS
KL term is this nll minus quantities that do not depend on the alignment -- the posterior's sum of logs_q, and constants
times C count -- so it is the caller's two extra [B] terms, not a kernel of its own.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._operands import f32c, gaussian_shapes, lengths, one_gpu, per_utterance, ptr, stream
from .maxpath import Alignment

_workspaces = _lib.StreamWorkspaces(zero=False)


def _check(z, mean, logstd, durations, t_y) -> Tuple[int, int, int, int, torch.Tensor]:
    B, C, Tx, Ty = gaussian_shapes(z, mean, logstd)
    if isinstance(durations, Alignment):
        if durations.durations is None:
            raise ValueError("the Alignment holds no durations (align(..., want_durations=True))")
        durations = durations.durations
    durations = torch.as_tensor(durations)
    if durations.is_floating_point() or durations.is_complex() or durations.dtype == torch.bool:
        raise ValueError("durations must be an integer tensor")
    if tuple(durations.shape) != (B, Tx):
        raise ValueError(f"durations must be [B,T_text] = [{B},{Tx}]")
    per_utterance(t_y, B, "t_y")
    one_gpu(((z, "z"), (mean, "mean"), (logstd, "logstd")), "z, mean and logstd")
    return B, C, Tx, Ty, durations


def _run(zc, mc, sc, dur, ty, scale, want_loss: bool, want_grad: bool):
    """One C-ABI call on prepared operands (fp32 contiguous, int32 durations / t_y, fp32 scale): the outputs asked for."""
    B, C, Ty = zc.shape
    Tx = mc.shape[2]
    dev = zc.device
    lib = _lib.load()
    nll = torch.empty((B,), dtype=torch.float32, device=dev) if want_loss else None
    count = torch.empty((B,), dtype=torch.int32, device=dev) if want_loss else None
    dz = torch.empty_like(zc) if want_grad else None
    dm = torch.empty_like(mc) if want_grad else None
    ds = torch.empty_like(sc) if want_grad else None
    # (0 bytes: a shape outside the domain; the call itself reports which limit, as an AlignerError of code EDOM)
    ws = _workspaces.get(dev, max(lib.aligner_gauss_nll_workspace_bytes(B, C, Tx), 1))
    _lib.check(lib.aligner_gauss_nll_f32(zc.data_ptr(), mc.data_ptr(), sc.data_ptr(), dur.data_ptr(), ptr(ty), ptr(scale),
                                         ptr(nll), ptr(count), ptr(dz), ptr(dm), ptr(ds), ws.data_ptr(), ws.numel(),
                                         B, C, Tx, Ty, stream(dev)))
    return nll, count, dz, dm, ds


def gaussian_nll(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, durations: Union[torch.Tensor, Alignment],
                 t_y: Optional[torch.Tensor] = None, *, want_grad: bool = False, scale: Optional[torch.Tensor] = None):
    """(nll [B] fp32, count [B] int32) and, with want_grad, (nll, count, dz [B,C,T_mel], dm [B,C,T_text], ds [B,C,T_text]):
    the loss of the module text and d sum_b(scale[b] nll[b]) / d(z, mean, logstd), fp32, without autograd.

    z [B,C,T_mel], mean and logstd [B,C,T_text]: GPU tensors (other dtypes than fp32 are cast, non-contiguous ones
    copied).  durations: an integer [B,T_text] tensor, or an Alignment whose .durations is set (gaussian_align()'s
    result); a negative entry counts as 0, a sum past T_mel is clipped.  t_y [B]: frames y >= t_y[b] do not count (None:
    the full extent).  scale [B]: the upstream gradient of nll (None: 1).  dz is +0.0 on a frame that does not count, dm
    and ds are +0.0 for a token without a counting frame.  No atomics: the same bits on every call.  Empty shapes return
    zeros without a launch.  Asynchronous on the current stream."""
    B, C, Tx, Ty, durations = _check(z, mean, logstd, durations, t_y)
    dev = z.device
    per_utterance(scale, B, "scale")
    _lib.require_gpu()
    with torch.no_grad(), torch.cuda.device(dev):
        if B == 0 or Tx == 0 or Ty == 0:
            out = (torch.zeros((B,), dtype=torch.float32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
            if want_grad:
                out += (torch.zeros((B, C, Ty), dtype=torch.float32, device=dev),
                        torch.zeros((B, C, Tx), dtype=torch.float32, device=dev),
                        torch.zeros((B, C, Tx), dtype=torch.float32, device=dev))
            return out
        dur = durations.detach().to(device=dev, dtype=torch.int32).contiguous()
        ty = lengths(t_y, B, dev, "t_y")
        sc = None if scale is None else torch.as_tensor(scale).detach().to(device=dev, dtype=torch.float32).reshape(B).contiguous()
        nll, count, dz, dm, ds = _run(f32c(z), f32c(mean), f32c(logstd), dur, ty, sc, True, want_grad)
    return (nll, count, dz, dm, ds) if want_grad else (nll, count)


class _GaussNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, mean, logstd, dur, ty):
        # (operands checked and converted by gaussian_nll_loss(): straight to the loss-only kernel)
        with torch.no_grad(), torch.cuda.device(z.device):
            nll, count, _, _, _ = _run(f32c(z), f32c(mean), f32c(logstd), dur, ty, None, True, False)
        ctx.save_for_backward(z, mean, logstd, dur, ty)
        ctx.mark_non_differentiable(count)
        return nll, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_nll, _g_count):
        z, mean, logstd, dur, ty = ctx.saved_tensors
        if g_nll is None or not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None
        # the gradient form with scale = g_nll: z is read a second time and dz written once, already scaled
        with torch.no_grad(), torch.cuda.device(z.device):
            sc = g_nll.detach().to(torch.float32).contiguous()
            _, _, dz, dm, ds = _run(f32c(z), f32c(mean), f32c(logstd), dur, ty, sc, False, True)
        need = ctx.needs_input_grad
        return (dz.to(z.dtype) if need[0] else None, dm.to(mean.dtype) if need[1] else None,
                ds.to(logstd.dtype) if need[2] else None, None, None)


def gaussian_nll_loss(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, durations: Union[torch.Tensor, Alignment],
                      t_y: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """gaussian_nll() with its gradient attached: the Glow-TTS / VITS likelihood loss of a training step, after
    gaussian_align() (the search runs under no_grad; the loss goes through here instead of through the expanded mean and
    log-std).  The forward pass runs the loss-only kernel; backward() runs the gradient form once, with the upstream
    gradient as its scale, and hands each input that requires grad its gradient in its own dtype (bf16 / fp16 inputs are
    cast to fp32 on the way in).  reduction: "mean" = sum(nll) / max(C sum(count), 1), the Glow-TTS form (per counting
    frame and channel); "sum"; "none" = nll [B].  A VITS KL term: reduction="none", minus the posterior's terms (module
    text)."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    B, C, Tx, Ty, dur = _check(z, mean, logstd, durations, t_y)
    dev = z.device
    if B == 0 or Tx == 0 or Ty == 0:
        nll, count = gaussian_nll(z, mean, logstd, dur, t_y)
        nll = nll + 0.0 * (z.sum() + mean.sum() + logstd.sum()).to(nll.dtype)        # (keeps the graph: zero gradients)
    else:
        _lib.require_gpu()
        dur = dur.detach().to(device=dev, dtype=torch.int32).contiguous()
        ty = lengths(t_y, B, dev, "t_y")
        nll, count = _GaussNLL.apply(z, mean, logstd, dur, ty)
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return nll.sum() / (C * count.sum()).clamp_min(1).to(nll.dtype)
