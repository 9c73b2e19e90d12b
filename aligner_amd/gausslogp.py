"""Glow-TTS / VITS log-likelihood front end on the HIP path (csrc/gausslogp.hip).

Both models search the alignment on the log-density of every latent frame under every token's diagonal Gaussian,

    value[b,i,j] = sum_c ( -1/2 ln 2pi - s[b,c,i] - 1/2 (z[b,c,j] - m[b,c,i])^2 exp(-2 s[b,c,i]) )

with m, s [B,C,T_text] the text encoder's mean and log-std and z [B,C,T_mel] the flow's output, computed under no_grad
(the loss goes through the expanded m and s: regulate()).  gaussian_logp() is that tensor in one fused kernel;
gaussian_align() is the whole `logp = ...; attn = maximum_path(logp, mask)` block of a training step.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .maxpath import Alignment, align
from .softattn import pitched_logp

_workspaces = _lib.StreamWorkspaces(zero=False)


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def gaussian_logp(z: torch.Tensor, mean: torch.Tensor, logstd: torch.Tensor, t_x: Optional[torch.Tensor] = None,
                  t_y: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
                  out_dtype: torch.dtype = torch.float32, pitched: bool = False) -> torch.Tensor:
    """value[b,i,j] = log N(z[b,:,j]; mean[b,:,i], exp(logstd[b,:,i])^2), [B,T_text,T_mel].

    z [B,C,T_mel], mean and logstd [B,C,T_text]: GPU tensors, channel-major as both models hold them (other dtypes than
    fp32 are cast, non-contiguous ones copied).  t_x / t_y [B]: cells with i >= t_x[b] or j >= t_y[b] are written as 0.0
    (Glow-TTS's `logp * attn_mask`); None = the full extent.  out_dtype torch.bfloat16 rounds the fp32 result to bf16 (half
    the traffic; align() / maximum_path() read it as it is).  pitched: return a [B,T_text,T_mel] VIEW of a buffer whose
    rows start on whole 128-byte lines (pitched_logp(): what align() reads fastest).  out: write into the caller's
    tensor, contiguous or such a view (its dtype decides); the columns >= T_mel of a pitched buffer are never touched.
    No gradient: the result never requires grad.  Asynchronous on the current stream."""
    for t, name in ((z, "z"), (mean, "mean"), (logstd, "logstd")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{name} must be a [B,C,T] tensor")
    B, C, Ty = z.shape
    B2, C2, Tx = mean.shape
    if B2 != B or C2 != C:
        raise ValueError(f"z {tuple(z.shape)} and mean {tuple(mean.shape)} disagree in B or C")
    if tuple(logstd.shape) != tuple(mean.shape):
        raise ValueError(f"logstd {tuple(logstd.shape)} must have mean's shape {tuple(mean.shape)}")
    if C < 1:
        raise ValueError("C must be at least 1")
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
    for t, name in ((z, "z"), (mean, "mean"), (logstd, "logstd")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor")
    dev = z.device
    if mean.device != dev or logstd.device != dev or (out is not None and out.device != dev):
        raise ValueError("z, mean, logstd and out must be on the same device")
    for t, name in ((t_x, "t_x"), (t_y, "t_y")):
        if t is not None and t.numel() != B:
            raise ValueError(f"{name} must have one entry per utterance")
    _lib.require_gpu()
    with torch.no_grad(), torch.cuda.device(dev):
        zc, mc, sc = _f32(z), _f32(mean), _f32(logstd)
        if t_x is not None:
            t_x = t_x.to(device=dev, dtype=torch.int32).contiguous()
        if t_y is not None:
            t_y = t_y.to(device=dev, dtype=torch.int32).contiguous()
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
            zc.data_ptr(), mc.data_ptr(), sc.data_ptr(), None if t_x is None else t_x.data_ptr(),
            None if t_y is None else t_y.data_ptr(), out.data_ptr(),
            _lib.DT_BF16 if out_dtype == torch.bfloat16 else _lib.DT_F32, ld, ws.data_ptr(), ws.numel(),
            B, C, Tx, Ty, torch.cuda.current_stream(dev).cuda_stream))
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
