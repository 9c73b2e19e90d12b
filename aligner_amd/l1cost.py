"""The L1 cost table of Soft-DTW and its gradient (csrc/l1cost.hip), and the loss in one piece: what
`soft_dtw_loss(torch.cdist(pred.transpose(1, 2), target.transpose(1, 2), p=1) * scale, ...)` computes, built only where
soft_dtw's cells exist and without the cdist graph.  Channels come first: pred [B,C,N], target [B,C,M].

    cost[b,i,j] = scale sum_c |pred[b,c,i] - target[b,c,j]|      i < n[b], j < m[b], |i - j| <= bandwidth
                = +inf                                           i < n[b], j < m[b], |i - j| >  bandwidth
                = 0                                              at or past n[b] or m[b]

    dpred[b,c,i]   =  g[b] scale sum_j G[b,i,j] sign(pred[b,c,i] - target[b,c,j])
    dtarget[b,c,j] = -g[b] scale sum_i G[b,i,j] sign(pred[b,c,i] - target[b,c,j])       over existing cells, sign(0) = 0

+inf is soft_dtw's forbidden cell, so the table carries the band with it.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._operands import check_reduction, f32c, lengths, one_gpu, pred_target_shapes, ptr, reduced, stream
from .softdtw import soft_dtw


def _checked(pred, target, bandwidth, scale, also=()) -> Tuple[int, int, int, int, int, float, torch.device]:
    """(B, C, N, M, the band as the C ABI takes it, scale, device).  also: (tensor, name) of a further [B,N,M] operand."""
    B, C, N, _, scale = pred_target_shapes(pred, target, scale)
    if bandwidth is not None and int(bandwidth) < 0:
        raise ValueError("bandwidth must be None (no band) or at least 0")
    for t, name in also:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, N, target.shape[2]):
            raise ValueError(f"{name} must be a [B,N,M] = {(B, N, target.shape[2])} tensor")
    named = ((pred, "pred"), (target, "target"), *also)
    dev = one_gpu(named, ", ".join(name for _, name in named))
    return B, C, N, target.shape[2], -1 if bandwidth is None else min(int(bandwidth), 2 ** 30), scale, dev


# The kinds of the cost: L1, and the two Euclidean ones of l2cost.py.  The wrappers of both modules are these helpers
# with the kind fixed.
L1, L2, L2_ROOT = "l1", "l2", "l2root"


def _cost(kind, pred, target, n, m, bandwidth, scale) -> torch.Tensor:
    """l1_cost() / l2_cost(): the [B,N,M] table of `kind`."""
    B, C, N, M, band, scale, dev = _checked(pred, target, bandwidth, scale)
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0 or M == 0:
        return torch.zeros((B, N, M), dtype=torch.float32, device=dev)
    _lib.require_gpu()
    lib = _lib.load()
    p, t = f32c(pred), f32c(target)
    cost = torch.empty((B, N, M), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if kind == L1:
            rc = lib.aligner_l1_cost_f32(p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), band, scale, cost.data_ptr(),
                                         B, C, N, M, stream(dev))
        else:
            rc = lib.aligner_l2_cost_f32(p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), band, scale, int(kind == L2),
                                         cost.data_ptr(), B, C, N, M, stream(dev))
        _lib.check(rc)
    return cost


def l1_cost(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
            bandwidth: Optional[int] = None, scale: float = 1.0) -> torch.Tensor:
    """cost [B,N,M] of the module text, fp32; every cell is written.

    pred [B,C,N], target [B,C,M]: GPU tensors (bf16 / fp16 are cast to fp32, non-contiguous ones copied); n / m [B]: the
    utterances' lengths (None: N / M; larger values are clamped).  B <= 65535, C <= 4096, N*M < 2^29 (an AlignerError of
    code EDOM beyond).  Not attached to autograd (soft_dtw_l1_loss() is).  Empty shapes return without a launch.
    Asynchronous on the current stream."""
    return _cost(L1, pred, target, n, m, bandwidth, scale)


def _cost_backward(kind, grad_cost, pred, target, n, m, bandwidth, scale, row_scale, want):
    """l1_cost_backward() / l2_cost_backward(): (dpred, dtarget) of `kind` (L1 or L2)."""
    if kind not in (L1, L2):
        raise ValueError("the root of the Euclidean cost has no gradient: train on the squared cost")
    B, C, N, M, band, scale, dev = _checked(pred, target, bandwidth, scale, also=((grad_cost, "grad_cost"),))
    want_p, want_t = bool(want[0]), bool(want[1])
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    rs = None
    if row_scale is not None:
        if torch.as_tensor(row_scale).numel() != B:
            raise ValueError("row_scale must have one entry per utterance")
        rs = torch.as_tensor(row_scale).detach().to(device=dev, dtype=torch.float32).reshape(B).contiguous()
    if not (want_p or want_t):
        return None, None
    empty = B == 0 or N == 0 or M == 0
    new = torch.zeros if empty else torch.empty
    dpred = new((B, C, N), dtype=torch.float32, device=dev) if want_p else None
    dtarget = new((B, C, M), dtype=torch.float32, device=dev) if want_t else None
    if empty:
        return dpred, dtarget
    _lib.require_gpu()
    lib = _lib.load()
    g, p, t = f32c(grad_cost), f32c(pred), f32c(target)
    with torch.cuda.device(dev):
        fn = lib.aligner_l1_cost_backward_f32 if kind == L1 else lib.aligner_l2_cost_backward_f32
        _lib.check(fn(g.data_ptr(), p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), band, scale, ptr(rs), ptr(dpred), ptr(dtarget),
                      B, C, N, M, stream(dev)))
    return dpred, dtarget


def l1_cost_backward(grad_cost: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                     m: Optional[torch.Tensor] = None, bandwidth: Optional[int] = None, scale: float = 1.0,
                     row_scale: Optional[torch.Tensor] = None, want: Tuple[bool, bool] = (True, True)
                     ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(dpred [B,C,N] or None, dtarget [B,C,M] or None) of the module text, fp32, with G = grad_cost [B,N,M].

    row_scale [B]: the per-utterance factor g (None: 1), so that nobody scales G in a pass of its own.  G is never read
    as a value where a cell does not exist.  One owner per output element and no atomics: the same bits on every call,
    and each output has the same bits whether or not the other is asked for.  Domain and lengths as in l1_cost()."""
    return _cost_backward(L1, grad_cost, pred, target, n, m, bandwidth, scale, row_scale, want)


class _SoftDtwCostLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale):
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        # the cost table lives for these two lines: the DP's backward reads R only, and E overwrites R in place
        cost = _cost(kind, pred, target, n, m, bandwidth, scale)
        value, E = soft_dtw(cost, n, m, gamma, warp_penalty, bandwidth, want_grad=need)
        del cost
        if need:
            ctx.save_for_backward(pred, target, E)
        ctx.lengths = (n, m)
        ctx.kind, ctx.band, ctx.scale = kind, bandwidth, scale
        return value

    @staticmethod
    def backward(ctx, g_value):
        want = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if not (want[0] or want[1]) or g_value is None:
            return (None,) * 9
        pred, target, E = ctx.saved_tensors
        n, m = ctx.lengths
        # (an utterance without an alignment has E = 0 and with it zero gradients, whatever its g)
        dpred, dtarget = _cost_backward(ctx.kind, E, pred, target, n, m, ctx.band, ctx.scale, g_value, want)
        return (None, None if dpred is None else dpred.to(pred.dtype), None if dtarget is None else dtarget.to(target.dtype),
                None, None, None, None, None, None)


def _soft_dtw_cost_loss(kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity):
    check_reduction(reduction)
    value = _SoftDtwCostLoss.apply(kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale)
    return reduced(value, reduction, zero_infinity)


def soft_dtw_l1_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                     m: Optional[torch.Tensor] = None, gamma: float = 1.0, warp_penalty: float = 0.0,
                     bandwidth: Optional[int] = None, scale: float = 1.0, reduction: str = "mean",
                     zero_infinity: bool = False) -> torch.Tensor:
    """Soft-DTW on the L1 cost of pred [B,C,N] against target [B,C,M] as one autograd function: l1_cost() and soft_dtw()
    in the forward pass, one l1_cost_backward() call on the saved E in the backward pass.  The cost table is dropped
    after the forward pass and no cdist graph is kept: what is saved is pred, target, E and the lengths.  Gradients come
    back in the inputs' dtypes, None for an input that does not require one.  reduction and zero_infinity as in
    soft_dtw_loss(); soft_dtw()'s domain (N <= 1024).  Parallel Tacotron 2: gamma 0.05, warp_penalty 128, bandwidth 60."""
    return _soft_dtw_cost_loss(L1, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity)
