"""Soft-DTW (csrc/softdtw.hip): the alignment loss between two frame sequences of different lengths, where either axis
may stall -- Cuturi & Blondel 2017; the loss Parallel Tacotron 2 trains on (L1 cost, a warp penalty, a diagonal band)
and the usual differentiable loss of a predicted mel against a target of another length.

For utterance b take D = cost[b, :n[b], :m[b]], gamma > 0, a warp penalty p >= 0 and an optional band w:

    softmin_g(a,b,c) = -gamma log(exp(-a/gamma) + exp(-b/gamma) + exp(-c/gamma))
    R[i,j] = D[i,j] + softmin_g(R[i-1,j-1], R[i-1,j] + p, R[i,j-1] + p)       R[-1,-1] = 0, every other border cell +inf
    value  = R[n-1,m-1]          E[i,j] = d value / d D[i,j]    (the expected alignment matrix, Mensch & Blondel 2018)

Cell (i,j) exists iff |i - j| <= w.  A +inf cost is a forbidden cell; an utterance without a finite path (|n - m| > w, a
length below 1, +inf costs across every path) has value +inf and an all-zero E, the "no alignment" convention of
forward_sum().  The L1 cost comes from l1_cost() (l1cost.py), built only where cells exist; soft_dtw_l1_loss() is the
two as one autograd function.  Any other cost is the caller's to build.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._operands import check_reduction, dp_parameters, f32c, lengths, ptr, reduced, stream

_workspaces = _lib.StreamWorkspaces(zero=False)


def _checked(cost, gamma, warp_penalty, bandwidth) -> Tuple[float, float, int]:
    if not isinstance(cost, torch.Tensor) or cost.dim() != 3:
        raise ValueError("cost must be a [B,N,M] tensor")
    if not cost.is_floating_point():
        raise ValueError("cost must be a floating-point tensor")
    gamma, warp_penalty = dp_parameters(gamma, warp_penalty)
    if bandwidth is not None and int(bandwidth) < 0:
        raise ValueError("bandwidth must be None (no band) or at least 0")
    if not cost.is_cuda:
        raise ValueError("cost must be a GPU tensor")
    return gamma, warp_penalty, -1 if bandwidth is None else min(int(bandwidth), 2 ** 30)


def soft_dtw(cost: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None, gamma: float = 1.0,
             warp_penalty: float = 0.0, bandwidth: Optional[int] = None, want_grad: bool = True
             ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(value [B], E [B,N,M] or None) of the module text, fp32.

    cost [B,N,M]: a GPU tensor (bf16 / fp16 are cast to fp32, a non-contiguous one is copied); n / m [B]: the
    utterances' lengths (None: N / M; larger values are clamped).  E is exactly 0 at and past n or m and outside the band.
    N <= 1024, B <= 65535, N*M < 2^29 (an AlignerError of code EDOM beyond).  One workgroup per utterance, no atomics:
    the same bits on every call.  Not attached to autograd (soft_dtw_loss() is).  Empty shapes return without a launch:
    value +inf.  Asynchronous on the current stream."""
    gamma, warp_penalty, band = _checked(cost, gamma, warp_penalty, bandwidth)
    B, N, M = cost.shape
    dev = cost.device
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0 or M == 0:
        return (torch.full((B,), float("inf"), dtype=torch.float32, device=dev),
                torch.zeros((B, N, M), dtype=torch.float32, device=dev) if want_grad else None)
    _lib.require_gpu()
    lib = _lib.load()
    c = f32c(cost)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty((B, N, M), dtype=torch.float32, device=dev) if want_grad else None
    with torch.cuda.device(dev):
        # (0 bytes: a shape outside the domain; the call itself reports which limit, as an AlignerError of code EDOM)
        ws = _workspaces.get(dev, max(lib.aligner_soft_dtw_workspace_bytes(B, N, M, int(want_grad)), 1))
        _lib.check(lib.aligner_soft_dtw_f32(c.data_ptr(), ptr(nn), ptr(mm), gamma, warp_penalty, band, value.data_ptr(),
                                            ptr(grad), ws.data_ptr(), ws.numel(), B, N, M, stream(dev)))
    return value, grad


class _SoftDtwLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, n, m, gamma, warp_penalty, bandwidth):
        need = ctx.needs_input_grad[0]
        value, E = soft_dtw(cost.detach(), n, m, gamma, warp_penalty, bandwidth, want_grad=need)
        ctx.save_for_backward(E if need else None)
        ctx.in_dtype = cost.dtype                   # (the kernels compute in fp32; a bf16 / fp16 cost gets its gradient back in its dtype)
        return value

    @staticmethod
    def backward(ctx, g_value):
        (E,) = ctx.saved_tensors
        if E is None or g_value is None:
            return None, None, None, None, None, None
        return (E * g_value.to(E.dtype).view(-1, 1, 1)).to(ctx.in_dtype), None, None, None, None, None


def soft_dtw_loss(cost: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                  gamma: float = 1.0, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                  reduction: str = "mean", zero_infinity: bool = False) -> torch.Tensor:
    """soft_dtw() as an autograd function: value and E come from one call in the forward pass, backward() only scales, so
    `soft_dtw_loss(torch.cdist(pred, target, p=1), n, m).backward()` reaches pred.  Parallel Tacotron 2 is gamma 0.05,
    warp_penalty 128 and bandwidth 60 on the summed L1 cost.  reduction: "mean" (a plain mean over the batch), "sum"
    or "none".  zero_infinity: an utterance without an alignment (value +inf) contributes 0 and no gradient instead of
    making the batch loss +inf.  No gradient for gamma or the penalty."""
    check_reduction(reduction)
    return reduced(_SoftDtwLoss.apply(cost, n, m, gamma, warp_penalty, bandwidth), reduction, zero_infinity)
