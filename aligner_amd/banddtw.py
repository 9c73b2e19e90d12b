"""Soft-DTW in band storage (csrc/banddtw.hip): the loss of softdtw.py / l1cost.py with cost, R and E kept as [B,N,W]
tensors, W = 2 w + 1, instead of [B,N,M] -- O(N w) memory, no limit on N, and a DP that walks the anti-diagonals of
the band (at most w + 1 cells each) in one wave per utterance.

    xb[b, i, d]  is cell  (i, j = i + d - w)              |i - j| <= w by construction, 0 <= w <= 127
    the cell exists  iff  i < n[b]  and  0 <= j < m[b]     n clamped to [0,N], m to [0,N+w] (to M where there is a target)

value and E are those of soft_dtw() on the dense image with bandwidth w (the same per-cell arithmetic: the forward
value has the same bits), cost and its gradient those of l1_cost() / l1_cost_backward().  Elements whose cell does not
exist are never read as values and are written as exactly 0 by every output, the cost table included.  The dense
functions remain the path for unbanded problems and for bandwidth > 127.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._operands import (check_reduction, dp_parameters, f32c, lengths, one_gpu, pred_target_shapes, ptr, reduced,
                        stream)
from .l1cost import L1, L2

MAX_BANDWIDTH = 127

_workspaces = _lib.StreamWorkspaces(zero=False)


def _band_index(N: int, M: int, w: int, device):
    """(j [N,W], inside [N,W]) of the index map j = i + d - w."""
    i = torch.arange(N, device=device).view(N, 1)
    d = torch.arange(2 * w + 1, device=device).view(1, -1)
    j = i + d - w
    return j, (j >= 0) & (j < M)


def _bandwidth(bandwidth) -> int:
    w = int(bandwidth)
    if w < 0:
        raise ValueError("bandwidth must be at least 0")
    if w > MAX_BANDWIDTH:
        raise ValueError(f"bandwidth must be at most {MAX_BANDWIDTH} in band storage: soft_dtw() / l1_cost() / "
                         "soft_dtw_l1_loss() take any band")
    return w


def dense_to_band(x: torch.Tensor, bandwidth: int, fill: float = 0.0) -> torch.Tensor:
    """x [B,N,M] -> [B,N,W]: element [b,i,d] = x[b,i,i+d-w], `fill` where that column is outside [0,M).  Plain torch
    indexing, for inspection and tests; CPU tensors too."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("x must be a [B,N,M] tensor")
    w = _bandwidth(bandwidth)
    B, N, M = x.shape
    j, inside = _band_index(N, M, w, x.device)
    out = torch.full((B, N, 2 * w + 1), fill, dtype=x.dtype, device=x.device)
    if M > 0:
        out[:, inside] = x[:, torch.arange(N, device=x.device).view(N, 1).expand_as(j)[inside], j[inside]]
    return out


def band_to_dense(xb: torch.Tensor, M: int, fill: float = 0.0) -> torch.Tensor:
    """xb [B,N,W] -> [B,N,M]: the inverse of dense_to_band() on the band, `fill` elsewhere (band elements whose
    column is outside [0,M) are dropped)."""
    if not isinstance(xb, torch.Tensor) or xb.dim() != 3 or xb.shape[2] % 2 == 0:
        raise ValueError("xb must be a [B,N,W] tensor with an odd W = 2 bandwidth + 1")
    B, N, W = xb.shape
    w = (W - 1) // 2
    M = int(M)
    j, inside = _band_index(N, M, w, xb.device)
    out = torch.full((B, N, M), fill, dtype=xb.dtype, device=xb.device)
    if M > 0:
        out[:, torch.arange(N, device=xb.device).view(N, 1).expand_as(j)[inside], j[inside]] = xb[:, inside]
    return out


def _checked_dp(cost_band, gamma, warp_penalty) -> Tuple[float, float, int]:
    if not isinstance(cost_band, torch.Tensor) or cost_band.dim() != 3:
        raise ValueError("cost_band must be a [B,N,W] tensor")
    if not cost_band.is_floating_point():
        raise ValueError("cost_band must be a floating-point tensor")
    if cost_band.shape[2] % 2 == 0:
        raise ValueError("cost_band must have an odd last dimension W = 2 bandwidth + 1")
    w = _bandwidth((cost_band.shape[2] - 1) // 2)
    gamma, warp_penalty = dp_parameters(gamma, warp_penalty)
    if not cost_band.is_cuda:
        raise ValueError("cost_band must be a GPU tensor")
    return gamma, warp_penalty, w


def soft_dtw_banded(cost_band: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                    gamma: float = 1.0, warp_penalty: float = 0.0, want_grad: bool = True
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(value [B], E_band [B,N,W] or None) of the module text, fp32.

    cost_band [B,N,W]: a GPU tensor in band storage (bf16 / fp16 are cast to fp32, a non-contiguous one is copied); the
    bandwidth is (W - 1) / 2.  n / m [B]: the utterances' lengths (None: N; n is clamped to N, m to N + w).  E_band is
    exactly 0 where no cell exists.  bandwidth <= 127, B <= 65535, N*W < 2^29 (an AlignerError of code EDOM beyond) and
    no other limit on N.  One workgroup per utterance, no atomics: the same bits on every call.  Not attached to
    autograd (soft_dtw_banded_loss() is).  Empty shapes return without a launch: value +inf.  Asynchronous on the
    current stream."""
    gamma, warp_penalty, w = _checked_dp(cost_band, gamma, warp_penalty)
    B, N, W = cost_band.shape
    dev = cost_band.device
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0:
        return (torch.full((B,), float("inf"), dtype=torch.float32, device=dev),
                torch.zeros((B, N, W), dtype=torch.float32, device=dev) if want_grad else None)
    _lib.require_gpu()
    lib = _lib.load()
    c = f32c(cost_band)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty((B, N, W), dtype=torch.float32, device=dev) if want_grad else None
    with torch.cuda.device(dev):
        ws = _workspaces.get(dev, max(lib.aligner_soft_dtw_banded_workspace_bytes(B, N, w, int(want_grad)), 1))
        _lib.check(lib.aligner_soft_dtw_banded_f32(c.data_ptr(), ptr(nn), ptr(mm), gamma, warp_penalty, w, value.data_ptr(),
                                                   ptr(grad), ws.data_ptr(), ws.numel(), B, N, stream(dev)))
    return value, grad


class _SoftDtwBandedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost_band, n, m, gamma, warp_penalty):
        need = ctx.needs_input_grad[0]
        value, E = soft_dtw_banded(cost_band.detach(), n, m, gamma, warp_penalty, want_grad=need)
        ctx.save_for_backward(E if need else None)
        ctx.in_dtype = cost_band.dtype
        return value

    @staticmethod
    def backward(ctx, g_value):
        (E,) = ctx.saved_tensors
        if E is None or g_value is None:
            return None, None, None, None, None
        return (E * g_value.to(E.dtype).view(-1, 1, 1)).to(ctx.in_dtype), None, None, None, None


def soft_dtw_banded_loss(cost_band: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                         gamma: float = 1.0, warp_penalty: float = 0.0, reduction: str = "mean",
                         zero_infinity: bool = False) -> torch.Tensor:
    """soft_dtw_banded() as an autograd function, the counterpart of soft_dtw_loss(): value and E_band come from one
    call in the forward pass, backward() only scales.  reduction: "mean", "sum" or "none"; zero_infinity: an utterance
    without an alignment contributes 0 and no gradient.  No gradient for gamma or the penalty."""
    check_reduction(reduction)
    return reduced(_SoftDtwBandedLoss.apply(cost_band, n, m, gamma, warp_penalty), reduction, zero_infinity)


def _checked_cost(pred, target, bandwidth, scale, also=()):
    """(B, C, N, M, w, scale, device).  also: (tensor, name) of a further [B,N,W] operand."""
    B, C, N, _, scale = pred_target_shapes(pred, target, scale)
    w = _bandwidth(bandwidth)
    for t, name in also:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, N, 2 * w + 1):
            raise ValueError(f"{name} must be a [B,N,W] = {(B, N, 2 * w + 1)} tensor")
    named = ((pred, "pred"), (target, "target"), *also)
    dev = one_gpu(named, ", ".join(name for _, name in named))
    return B, C, N, target.shape[2], w, scale, dev


def _cost_banded(kind, pred, target, n, m, bandwidth, scale) -> torch.Tensor:
    """l1_cost_banded() / l2_cost_banded(): the [B,N,W] table of `kind` (l1cost.py names the kinds)."""
    B, C, N, M, w, scale, dev = _checked_cost(pred, target, bandwidth, scale)
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0 or M == 0:
        return torch.zeros((B, N, 2 * w + 1), dtype=torch.float32, device=dev)
    _lib.require_gpu()
    lib = _lib.load()
    p, t = f32c(pred), f32c(target)
    cost = torch.empty((B, N, 2 * w + 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if kind == L1:
            rc = lib.aligner_l1_cost_banded_f32(p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), w, scale, cost.data_ptr(),
                                                B, C, N, M, stream(dev))
        else:
            rc = lib.aligner_l2_cost_banded_f32(p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), w, scale, int(kind == L2),
                                                cost.data_ptr(), B, C, N, M, stream(dev))
        _lib.check(rc)
    return cost


def l1_cost_banded(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                   m: Optional[torch.Tensor] = None, bandwidth: int = 60, scale: float = 1.0) -> torch.Tensor:
    """cost_band [B,N,W], fp32: scale sum_c |pred[b,c,i] - target[b,c,j]| on the cells that exist, exactly 0 elsewhere;
    every element is written.

    pred [B,C,N], target [B,C,M]: GPU tensors (bf16 / fp16 are cast, non-contiguous ones copied); n / m [B]: the lengths
    (None: N / M; m is clamped to M and to N + w).  bandwidth <= 127, B <= 65535, C <= 4096, N*W < 2^29 (an AlignerError
    of code EDOM beyond).  Not attached to autograd.  Empty shapes return without a launch.  Asynchronous."""
    return _cost_banded(L1, pred, target, n, m, bandwidth, scale)


def _cost_banded_backward(kind, grad_band, pred, target, n, m, scale, row_scale, want):
    """l1_cost_banded_backward() / l2_cost_banded_backward(): (dpred, dtarget) of `kind` (L1 or L2)."""
    if kind not in (L1, L2):
        raise ValueError("the root of the Euclidean cost has no gradient: train on the squared cost")
    if not isinstance(grad_band, torch.Tensor) or grad_band.dim() != 3 or grad_band.shape[2] % 2 == 0:
        raise ValueError("grad_band must be a [B,N,W] tensor with an odd W = 2 bandwidth + 1")
    B, C, N, M, w, scale, dev = _checked_cost(pred, target, (grad_band.shape[2] - 1) // 2, scale, also=((grad_band, "grad_band"),))
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
    g, p, t = f32c(grad_band), f32c(pred), f32c(target)
    with torch.cuda.device(dev):
        fn = lib.aligner_l1_cost_banded_backward_f32 if kind == L1 else lib.aligner_l2_cost_banded_backward_f32
        _lib.check(fn(g.data_ptr(), p.data_ptr(), t.data_ptr(), ptr(nn), ptr(mm), w, scale, ptr(rs), ptr(dpred), ptr(dtarget),
                      B, C, N, M, stream(dev)))
    return dpred, dtarget


def l1_cost_banded_backward(grad_band: torch.Tensor, pred: torch.Tensor, target: torch.Tensor,
                            n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None, scale: float = 1.0,
                            row_scale: Optional[torch.Tensor] = None, want: Tuple[bool, bool] = (True, True)
                            ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(dpred [B,C,N] or None, dtarget [B,C,M] or None) of l1_cost_backward() with G = grad_band [B,N,W] in band storage
    (the bandwidth is (W - 1) / 2).  row_scale [B]: the per-utterance factor (None: 1).  G is never read as a value
    where no cell exists.  One owner per output element, no atomics: the same bits on every call, and each output has
    the same bits whether or not the other is asked for."""
    return _cost_banded_backward(L1, grad_band, pred, target, n, m, scale, row_scale, want)


def _dp_columns(m, pred, target):
    """m as the band-storage DP needs it: the cost knows the target's M, the DP is told through m."""
    if m is not None:
        return torch.as_tensor(m).clamp(max=target.shape[2])
    return torch.full((pred.shape[0],), target.shape[2], dtype=torch.int32, device=pred.device)


class _SoftDtwCostBandedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale):
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        # the band cost tensor lives for these lines: the DP's backward reads R only, and E overwrites R in place
        cost = _cost_banded(kind, pred, target, n, m, bandwidth, scale)
        m = _dp_columns(m, pred, target)
        value, E = soft_dtw_banded(cost, n, m, gamma, warp_penalty, want_grad=need)
        del cost
        if need:
            ctx.save_for_backward(pred, target, E)
        ctx.lengths = (n, m)
        ctx.kind, ctx.scale = kind, scale
        return value

    @staticmethod
    def backward(ctx, g_value):
        want = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if not (want[0] or want[1]) or g_value is None:
            return (None,) * 9
        pred, target, E = ctx.saved_tensors
        n, m = ctx.lengths
        dpred, dtarget = _cost_banded_backward(ctx.kind, E, pred, target, n, m, ctx.scale, g_value, want)
        return (None, None if dpred is None else dpred.to(pred.dtype), None if dtarget is None else dtarget.to(target.dtype),
                None, None, None, None, None, None)


def _soft_dtw_cost_banded_loss(kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity):
    check_reduction(reduction)
    _bandwidth(bandwidth)
    value = _SoftDtwCostBandedLoss.apply(kind, pred, target, n, m, gamma, warp_penalty, bandwidth, scale)
    return reduced(value, reduction, zero_infinity)


def soft_dtw_l1_banded_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                            m: Optional[torch.Tensor] = None, gamma: float = 1.0, warp_penalty: float = 0.0,
                            bandwidth: int = 60, scale: float = 1.0, reduction: str = "mean",
                            zero_infinity: bool = False) -> torch.Tensor:
    """soft_dtw_l1_loss() in band storage, as one autograd function: l1_cost_banded() and soft_dtw_banded() in the
    forward pass, one l1_cost_banded_backward() call on the saved E_band with the upstream gradient as row_scale in the
    backward pass.  The band cost tensor is dropped after the DP; what is saved is pred, target, E_band and the
    lengths: [B,N,2w+1] where the dense function keeps [B,N,M].  Gradients come back in the inputs' dtypes, None for
    an input that does not require one.  Any N (no 1024-row limit); bandwidth <= 127, beyond which soft_dtw_l1_loss()
    is the path.  Parallel Tacotron 2: gamma 0.05, warp_penalty 128, bandwidth 60."""
    return _soft_dtw_cost_banded_loss(L1, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity)
