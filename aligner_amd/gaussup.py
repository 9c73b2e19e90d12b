"""Gaussian upsampling (csrc/gaussup.hip): the differentiable length regulator of JETS, Non-Attentive Tacotron, Parallel
Tacotron and ESPnet's GaussianUpsampling, where regulate() is the hard one.

Frame y of utterance b sits at tau_y = y + frame_offset and takes a softmax-weighted mix of the token encodings, the
weights Gaussians in the distance between the frame and each token's centre:

    e[b,y,x]   = log_weight[b,x] - precision[b,x] (tau_y - centres[b,x])^2        x < t_x[b]
    p[b,y,.]   = softmax over those x
    out[b,:,y] = sum_x p[b,y,x] h[b,:,x]                                           y < t_y[b]; 0 beyond

so the output is differentiable in the centres -- in float durations -- and in a learned width.  gaussian_upsample_at() is
the raw operation on centres and precisions, gaussian_upsample() the model face on durations.  The weights are never
stored: a token whose energy is more than 30 (ALIGNER_GAUSS_UP_CUT) below a frame's largest may count as zero, so with
centres in order the kernels touch a band of tokens per tile of frames; backward recomputes the weights.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._operands import f32c, lengths, ptr, stream

_workspaces = _lib.StreamWorkspaces(zero=False)


def _forward(h, c, a, g, tx, ty, off: float, Ty: int) -> torch.Tensor:
    """One forward C-ABI call on prepared operands (fp32 contiguous, int32 lengths)."""
    B, C, Tx = h.shape
    dev = h.device
    lib = _lib.load()
    out = torch.empty((B, C, Ty), dtype=torch.float32, device=dev)
    # (0 bytes: a shape outside the domain; the call itself reports which limit, as an AlignerError of code EDOM)
    ws = _workspaces.get(dev, max(lib.aligner_gauss_upsample_workspace_bytes(B, C, Tx, Ty), 1))
    _lib.check(lib.aligner_gauss_upsample_f32(h.data_ptr(), c.data_ptr(), a.data_ptr(), ptr(g), ptr(tx), ptr(ty), off,
                                              out.data_ptr(), ws.data_ptr(), ws.numel(), B, C, Tx, Ty,
                                              stream(dev)))
    return out


def _backward(h, c, a, g, tx, ty, off: float, gout, want_h: bool, want_c: bool, want_a: bool, want_g: bool):
    """One backward C-ABI call: (dh, dcentres, dprecision, dlog_weight), None for an output that was not asked for."""
    B, C, Tx = h.shape
    Ty = gout.shape[2]
    dev = h.device
    lib = _lib.load()
    dh = torch.empty_like(h) if want_h else None
    dc, da, dg = (torch.empty((B, Tx), dtype=torch.float32, device=dev) if w else None for w in (want_c, want_a, want_g))
    ws = _workspaces.get(dev, max(lib.aligner_gauss_upsample_backward_workspace_bytes(B, C, Tx, Ty), 1))
    _lib.check(lib.aligner_gauss_upsample_backward_f32(h.data_ptr(), c.data_ptr(), a.data_ptr(), ptr(g), ptr(tx), ptr(ty),
                                                       off, gout.data_ptr(), ptr(dh), ptr(dc), ptr(da), ptr(dg),
                                                       ws.data_ptr(), ws.numel(), B, C, Tx, Ty,
                                                       stream(dev)))
    return dh, dc, da, dg


class _GaussUp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, c, a, g, tx, ty, off, Ty):
        # (operands checked by gaussian_upsample_at(); a and g already have the centres' shape)
        with torch.no_grad(), torch.cuda.device(h.device):
            out = _forward(f32c(h), f32c(c), f32c(a), None if g is None else f32c(g), tx, ty, off, Ty)
        ctx.save_for_backward(h, c, a, g, tx, ty)
        ctx.off = off
        return out if h.dtype == torch.float32 else out.to(h.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        h, c, a, g, tx, ty = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_g = g is not None and need[3]
        if not (need[0] or need[1] or need[2] or need_g):
            return (None,) * 8
        with torch.no_grad(), torch.cuda.device(h.device):
            dh, dc, da, dg = _backward(f32c(h), f32c(c), f32c(a), None if g is None else f32c(g), tx, ty, ctx.off,
                                       f32c(gout), need[0], need[1], need[2], need_g)
        return (None if dh is None else dh.to(h.dtype), None if dc is None else dc.to(c.dtype),
                None if da is None else da.to(a.dtype), None if dg is None else dg.to(g.dtype), None, None, None, None)


def _row_operand(t, like: torch.Tensor, name: str) -> torch.Tensor:
    """precision / log_weight: a [B,T_text] tensor, or a scalar (a number or a 0-dim tensor) spread over the tokens."""
    if not isinstance(t, torch.Tensor):
        return torch.full(like.shape, float(t), dtype=torch.float32, device=like.device)
    if t.dim() == 0:
        return t.to(like.device).expand(like.shape)
    if tuple(t.shape) != tuple(like.shape):
        raise ValueError(f"{name} must be a scalar or [B,T_text] = {list(like.shape)}")
    if t.device != like.device:
        raise ValueError(f"{name} must be on the device of centres")
    return t


def gaussian_upsample_at(h: torch.Tensor, centres: torch.Tensor, precision, log_weight=None, T_mel: Optional[int] = None,
                         t_x: Optional[torch.Tensor] = None, t_y: Optional[torch.Tensor] = None,
                         frame_offset: float = 0.0) -> torch.Tensor:
    """out [B,C,T_mel] of the module text, in h's dtype.

    h [B,C,T_text] and centres [B,T_text]: GPU tensors; precision >= 0 and log_weight (None: 0): [B,T_text] tensors or
    scalars.  A negative precision is the caller's error and is not checked.  T_mel: the number of frames (required).
    t_x / t_y [B]: tokens x >= t_x[b] do not exist, frames y >= t_y[b] are 0 (None: the full extent); an utterance with
    t_x = 0 is all zeros.  Attached to autograd when any of h, centres, precision, log_weight requires grad; backward
    computes only the gradients that are needed and hands each back in its input's dtype (bf16 / fp16 inputs are cast to
    fp32 on the way in).  Non-contiguous inputs are copied.  Centres in non-decreasing order over x < t_x take the banded
    kernels; any other order takes the full token range: slower, the same definition.  No atomics: the same bits on
    every call.  Empty shapes return zeros without a launch.  Asynchronous on the current stream."""
    if not isinstance(h, torch.Tensor) or h.dim() != 3:
        raise ValueError("h must be a [B,C,T_text] tensor")
    B, C, Tx = h.shape
    if not isinstance(centres, torch.Tensor) or tuple(centres.shape) != (B, Tx):
        raise ValueError(f"centres must be [B,T_text] = [{B},{Tx}]")
    if T_mel is None or int(T_mel) < 0:
        raise ValueError("T_mel (the number of frames, >= 0) is required")
    Ty = int(T_mel)
    if not h.is_floating_point() or not centres.is_floating_point():
        raise ValueError("h and centres must be floating-point tensors")
    if not h.is_cuda:
        raise ValueError("h must be a GPU tensor")
    if centres.device != h.device:
        raise ValueError("h and centres must be on the same device")
    a = _row_operand(precision, centres, "precision")
    g = None if log_weight is None else _row_operand(log_weight, centres, "log_weight")
    dev = h.device
    tx = lengths(t_x, B, dev, "t_x")
    ty = lengths(t_y, B, dev, "t_y")
    if B == 0 or C == 0 or Tx == 0 or Ty == 0:
        out = torch.zeros((B, C, Ty), dtype=h.dtype, device=dev)
        live = [t for t in (h, centres, a, g) if isinstance(t, torch.Tensor) and t.requires_grad]
        return out + sum(0.0 * t.sum().to(out.dtype) for t in live) if live else out       # (keeps the graph: zero gradients)
    _lib.require_gpu()
    return _GaussUp.apply(h, centres, a, g, tx, ty, float(frame_offset), Ty)


def gaussian_upsample(h: torch.Tensor, durations: torch.Tensor, T_mel: int, t_x: Optional[torch.Tensor] = None,
                      t_y: Optional[torch.Tensor] = None, delta: float = 0.1, sigma: Optional[torch.Tensor] = None,
                      frame_offset: float = 0.0) -> torch.Tensor:
    """Gaussian upsampling of h [B,C,T_text] to [B,C,T_mel] by durations [B,T_text] (float or integer; a negative entry
    counts as 0, as everywhere in this package).  centres = cumsum(d) - d / 2 is computed in torch on the [B,T_text]
    tensor, so autograd carries the centres' gradient back to float durations.

    sigma=None: the ESPnet / JETS form, e = -delta (tau - centre)^2.  sigma [B,T_text] > 0: the Non-Attentive Tacotron
    form, the weights normal densities N(tau; centre, sigma^2): precision = 1 / (2 sigma^2), log_weight = -ln sigma, again
    in torch so that sigma gets its gradient.  t_x, t_y, frame_offset: gaussian_upsample_at() (ESPnet's frames sit at
    0, 1, ...: frame_offset 0; 0.5 puts a frame at the middle of its interval).

    One deliberate difference from ESPnet's GaussianUpsampling: ESPnet computes a value for masked frames as well (its
    softmax runs over the tokens whatever the frame mask says); here the frames y >= t_y[b] are 0."""
    if not isinstance(h, torch.Tensor) or h.dim() != 3:
        raise ValueError("h must be a [B,C,T_text] tensor")
    B, _, Tx = h.shape
    durations = torch.as_tensor(durations)
    if tuple(durations.shape) != (B, Tx):
        raise ValueError(f"durations must be [B,T_text] = [{B},{Tx}]")
    if durations.is_complex() or durations.dtype == torch.bool:
        raise ValueError("durations must be a float or integer tensor")
    if not h.is_cuda:
        raise ValueError("h must be a GPU tensor")
    d = durations.to(h.device)
    if not d.is_floating_point():
        d = d.to(torch.float32)
    d = d.clamp_min(0)
    centres = torch.cumsum(d, dim=1) - 0.5 * d
    if sigma is None:
        return gaussian_upsample_at(h, centres, float(delta), None, T_mel, t_x, t_y, frame_offset)
    if not isinstance(sigma, torch.Tensor) or tuple(sigma.shape) != (B, Tx):
        raise ValueError(f"sigma must be [B,T_text] = [{B},{Tx}]")
    sigma = sigma.to(h.device)
    return gaussian_upsample_at(h, centres, 0.5 / (sigma * sigma), -torch.log(sigma), T_mel, t_x, t_y, frame_offset)
