"""Operand preparation shared by the modules that call the C ABI: tensors as the kernels read them, nullable pointers,
the current stream's handle, the per-utterance lengths, and the checks of the Gaussian front end's (z, mean, logstd).
The C-ABI calls themselves stay written out in their modules."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


def f32c(t: torch.Tensor) -> torch.Tensor:
    """t as a kernel reads it: detached, fp32, contiguous (a cast or a copy only where needed)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def ptr(t: Optional[torch.Tensor]):
    """The C ABI's nullable pointer."""
    return None if t is None else t.data_ptr()


def stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def per_utterance(t, B: int, name: str) -> None:
    """The argument check of a [B] operand that may be None: one entry per utterance."""
    if t is not None and torch.as_tensor(t).numel() != B:
        raise ValueError(f"{name} must have one entry per utterance")


def lengths(t, B: int, device, name: str) -> Optional[torch.Tensor]:
    """t_x / t_y as the kernels read them: int32 [B], contiguous, on `device`; None (the full extent) passes through."""
    per_utterance(t, B, name)
    if t is None:
        return None
    return torch.as_tensor(t).detach().to(device=device, dtype=torch.int32).reshape(B).contiguous()


def gaussian_shapes(z, mean, logstd, also=()) -> Tuple[int, int, int, int]:
    """(B, C, T_text, T_mel) of z [B,C,T_mel] and mean, logstd [B,C,T_text].  also: (tensor, message) pairs of further
    operands that must be 3-D tensors, tested before the shapes are compared."""
    for t, message in ((z, "z must be a [B,C,T] tensor"), (mean, "mean must be a [B,C,T] tensor"),
                       (logstd, "logstd must be a [B,C,T] tensor"), *also):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(message)
    B, C, Ty = z.shape
    B2, C2, Tx = mean.shape
    if B2 != B or C2 != C:
        raise ValueError(f"z {tuple(z.shape)} and mean {tuple(mean.shape)} disagree in B or C")
    if tuple(logstd.shape) != tuple(mean.shape):
        raise ValueError(f"logstd {tuple(logstd.shape)} must have mean's shape {tuple(mean.shape)}")
    if C < 1:
        raise ValueError("C must be at least 1")
    return B, C, Tx, Ty


def one_gpu(named, names: str) -> torch.device:
    """The device of the (tensor, name) pairs: GPU tensors all, on one device (`names`: how the error lists them)."""
    for t, name in named:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor")
    dev = named[0][0].device
    if any(t.device != dev for t, _ in named):
        raise ValueError(f"{names} must be on the same device")
    return dev


def penalty(warp_penalty) -> float:
    """The warp penalty of the DTW calls as a float, checked."""
    warp_penalty = float(warp_penalty)
    if not (warp_penalty >= 0.0 and math.isfinite(warp_penalty)):
        raise ValueError("warp_penalty must be finite and not negative")
    return warp_penalty


def dp_parameters(gamma, warp_penalty) -> Tuple[float, float]:
    """Soft-DTW's (gamma, warp_penalty) as floats, checked."""
    gamma = float(gamma)
    if not (gamma > 0.0 and math.isfinite(gamma)):
        raise ValueError("gamma must be positive and finite")
    return gamma, penalty(warp_penalty)


def pred_target_shapes(pred, target, scale) -> Tuple[int, int, int, int, float]:
    """(B, C, N, M, scale) of the L1 cost's pred [B,C,N] and target [B,C,M], checked."""
    for t, name in ((pred, "pred"), (target, "target")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{name} must be a [B,C,T] tensor")
        if not t.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor")
    B, C, N = pred.shape
    if target.shape[0] != B or target.shape[1] != C:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} disagree in B or C")
    if C < 1:
        raise ValueError("C must be at least 1")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite")
    return B, C, N, target.shape[2], scale


def check_reduction(reduction: str) -> None:
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")


def reduced(value: torch.Tensor, reduction: str, zero_infinity: bool) -> torch.Tensor:
    """The per-utterance losses reduced: "mean", "sum" or "none"; zero_infinity: +inf (no alignment) counts as 0."""
    if zero_infinity:
        value = torch.where(torch.isinf(value), torch.zeros_like(value), value)
    if reduction == "mean":
        return value.mean()
    if reduction == "sum":
        return value.sum()
    return value
