"""Operand preparation shared by the modules that call the C ABI: tensors as the kernels read them, nullable pointers,
the current stream's handle, the per-utterance lengths, and the checks of the Gaussian front end's (z, mean, logstd).
The C-ABI calls themselves stay written out in their modules."""
from __future__ import annotations

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
