"""The cost kinds along a warping path (csrc/pathcost.hip): the cells of l1_cost() / l2_cost() evaluated on the pairs of
a path instead of on a table, forward and backward, and with them the hard-DTW losses -- the gamma -> 0 limit of the
soft losses, which those cannot take.

A path is what dtw_path() / dtw_path_banded() return: path [B,L,2] int32 pairs (i,j) in ascending order, -1 past
length [B]; L is whatever the buffer has (N+M-1 dense, 2N+w-1 from band storage).  pred [B,C,N] and target [B,C,M] are
channel-major and need not be the features the path was found on; `kind` is "l1", "l2" (squared) or "l2root".

    pair_cost[b,k] = the cell (i_k, j_k) of l1_cost() / l2_cost(squared=...) with the same scale, bit for bit;
                     +inf for a pair outside [0,n[b]) x [0,m[b]); 0 for k >= length[b]
    total[b]       = the sum of the length[b] pair costs in a fixed order; +inf for a length below 1
    mean[b]        = total[b] / length[b]

    with weights w_k (pair_weight, or 1), g = row_scale (or 1) and d_k,c = pred[b,c,i_k] - target[b,c,j_k]:
    dpred[b,c,i]   =  factor sum over the pairs k of row i's run     of  w_k s(d_k,c)
    dtarget[b,c,j] = -factor sum over the pairs k of column j's run  of  w_k s(d_k,c)
    l1: s = sign(d), factor = scale g      l2: s = d, factor = 2 scale g      l2root: s = d / dist_k, factor = scale g
                                                                              (s = 0 where the distance dist_k is 0)

Along a path the root kind has a gradient: only the K distances of the path are needed, not a finished table.  The
gradient of the losses is that of the value with the path held fixed: the derivative of the hard-DTW value wherever the
optimal path is unique, a subgradient at ties.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._operands import check_reduction, f32c, lengths, one_gpu, penalty, pred_target_shapes, ptr, reduced, stream
from .l1cost import L1, L2, L2_ROOT
from .l2cost import MCD_SCALE, _cost_and_path, _kind

_KINDS = {L1: _lib.COST_L1, L2: _lib.COST_L2, L2_ROOT: _lib.COST_L2_ROOT}
_workspaces = _lib.StreamWorkspaces(zero=False)


class PathRuns(NamedTuple):
    row_start: torch.Tensor             # [B,N] int32: the index k of the first pair with row i, -1 for a row not on the path
    row_count: torch.Tensor             # [B,N] int32: how many pairs have row i (the target frames this frame covers)
    col_start: torch.Tensor             # [B,M] int32
    col_count: torch.Tensor             # [B,M] int32
    valid: torch.Tensor                 # [B] int32: 1 for a warping path, 0 otherwise (then every count is 0)


def _checked_path(path, length) -> Tuple[int, int]:
    """(B, L) of path [B,L,2] and length [B], checked."""
    if not isinstance(path, torch.Tensor) or path.dim() != 3 or path.shape[2] != 2:
        raise ValueError("path must be a [B,L,2] tensor")
    if path.is_floating_point() or path.dtype == torch.bool:
        raise ValueError("path must be an integer tensor")
    B, L, _ = path.shape
    if not isinstance(length, torch.Tensor) or length.numel() != B:
        raise ValueError("length must be a tensor with one entry per utterance")
    return B, L


def _kind_code(kind) -> int:
    if kind not in _KINDS:
        raise ValueError("kind must be 'l1', 'l2' or 'l2root'")
    return _KINDS[kind]


def _i32c(t: torch.Tensor, dev, shape) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.int32).reshape(shape).contiguous()


def path_runs(path: torch.Tensor, length: torch.Tensor, N: int, M: int) -> PathRuns:
    """PathRuns of path [B,L,2], length [B] on an N x M table (module text), all int32; every element is written.

    The pairs of a warping path with row i are consecutive in k, and so are those with column j: row_start / row_count
    and col_start / col_count name those runs.  An utterance is valid iff 0 <= length <= L, every pair inside the
    length lies in [0,N) x [0,M) and every step is (1,1), (1,0) or (0,1); one that is not has valid 0, every start -1
    and every count 0, and is treated as one without an alignment.  path must be a GPU tensor.  One workgroup per
    utterance, one writer per element.  B <= 65535, L < 2^24.  Empty shapes return without a launch.  Asynchronous."""
    B, L = _checked_path(path, length)
    N, M = int(N), int(M)
    if N < 0 or M < 0:
        raise ValueError("N and M must not be negative")
    if not path.is_cuda:
        raise ValueError("path must be a GPU tensor")
    dev = path.device
    ln = _i32c(length, dev, (B,))
    if B == 0 or L == 0 or N == 0 or M == 0:
        neg = lambda T: torch.full((B, T), -1, dtype=torch.int32, device=dev)         # noqa: E731
        zero = lambda T: torch.zeros((B, T), dtype=torch.int32, device=dev)          # noqa: E731
        return PathRuns(neg(N), zero(N), neg(M), zero(M), (ln == 0).to(torch.int32))
    _lib.require_gpu()
    lib = _lib.load()
    p = _i32c(path, dev, (B, L, 2))
    out = [torch.empty((B, T), dtype=torch.int32, device=dev) for T in (N, N, M, M)]
    valid = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.aligner_path_runs(p.data_ptr(), ln.data_ptr(), *(t.data_ptr() for t in out), valid.data_ptr(),
                                         B, L, N, M, stream(dev)))
    return PathRuns(*out, valid)


def _checked(pred, target, path, length, kind, scale, also=()):
    """(B, C, N, M, L, the kind's code, scale, device).  also: (tensor, name) of a further [B,L] operand."""
    B, C, N, M, scale = pred_target_shapes(pred, target, scale)
    B2, L = _checked_path(path, length)
    if B2 != B:
        raise ValueError(f"path {tuple(path.shape)} must have pred's batch size {B}")
    code = _kind_code(kind)
    for t, name in also:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, L):
            raise ValueError(f"{name} must be a [B,L] = {(B, L)} tensor")
    named = ((pred, "pred"), (target, "target"), (path, "path"), *also)
    dev = one_gpu(named, ", ".join(name for _, name in named))
    return B, C, N, M, L, code, scale, dev


def path_cost(pred: torch.Tensor, target: torch.Tensor, path: torch.Tensor, length: torch.Tensor,
              n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None, kind: str = "l1",
              scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(pair_cost [B,L], total [B]) of the module text, fp32; every element is written.

    pred [B,C,N], target [B,C,M]: GPU tensors (bf16 / fp16 are cast to fp32, non-contiguous ones copied) of any channel
    count of their own, equal to each other: F0-RMSE along an MCD path is path_cost(f0_pred, f0_target, r.path,
    r.length, kind="l2") on the path of dtw_path_l2().  n / m [B]: the lengths (None: N / M; clamped).  The mean is
    total / length.  One lane per pair, one workgroup per utterance for the total, no atomics: the same bits on every
    call.  B <= 65535, C <= 4096, L < 2^24 (an AlignerError of code EDOM beyond).  Not attached to autograd
    (dtw_l1_loss() / dtw_l2_loss() are).  Empty shapes return without a launch.  Asynchronous on the current stream."""
    B, C, N, M, L, code, scale, dev = _checked(pred, target, path, length, kind, scale)
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    ln = _i32c(length, dev, (B,))
    if B == 0 or L == 0 or N == 0 or M == 0:
        on = torch.arange(L, device=dev).view(1, L) < ln.view(B, 1)
        inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
        return torch.where(on, inf, torch.zeros_like(inf)), torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
    _lib.require_gpu()
    lib = _lib.load()
    p, t, ij = f32c(pred), f32c(target), _i32c(path, dev, (B, L, 2))
    pair = torch.empty((B, L), dtype=torch.float32, device=dev)
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.aligner_path_cost_f32(p.data_ptr(), t.data_ptr(), ij.data_ptr(), ln.data_ptr(), ptr(nn), ptr(mm), code,
                                             scale, pair.data_ptr(), total.data_ptr(), B, C, N, M, L, stream(dev)))
    return pair, total


def path_cost_backward(pair_weight: Optional[torch.Tensor], pred: torch.Tensor, target: torch.Tensor, path: torch.Tensor,
                       length: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                       kind: str = "l1", scale: float = 1.0, row_scale: Optional[torch.Tensor] = None,
                       want: Tuple[bool, bool] = (True, True)) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(dpred [B,C,N] or None, dtarget [B,C,M] or None) of the module text, fp32: the gradient of
    sum_k pair_weight[b,k] pair_cost[b,k] times row_scale[b], all three kinds.

    pair_weight [B,L] (None: all 1) is never read at k >= length[b]; row_scale [B]: the per-utterance factor g (None: 1).
    Pairs are read only inside [0,n) x [0,m).  Rows, columns and utterances without pairs -- an utterance whose path is
    not a warping path (path_runs(): valid 0) among them -- get exactly 0 whatever row_scale holds.  The root kind
    divides by the pair's distance and contributes 0 where that is 0.  One owner per output element, no atomics: the
    same bits on every call, and each output has the same bits whether or not the other is asked for.  Domain and
    operands as in path_cost()."""
    also = () if pair_weight is None else ((pair_weight, "pair_weight"),)
    B, C, N, M, L, code, scale, dev = _checked(pred, target, path, length, kind, scale, also=also)
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
    empty = B == 0 or L == 0 or N == 0 or M == 0
    new = torch.zeros if empty else torch.empty
    dpred = new((B, C, N), dtype=torch.float32, device=dev) if want_p else None
    dtarget = new((B, C, M), dtype=torch.float32, device=dev) if want_t else None
    if empty:
        return dpred, dtarget
    _lib.require_gpu()
    lib = _lib.load()
    p, t, ij, ln = f32c(pred), f32c(target), _i32c(path, dev, (B, L, 2)), _i32c(length, dev, (B,))
    w = None if pair_weight is None else f32c(pair_weight)
    with torch.cuda.device(dev):
        # (0 bytes: a shape outside the domain; the call itself reports which limit, as an AlignerError of code EDOM)
        ws = _workspaces.get(dev, max(lib.aligner_path_cost_backward_workspace_bytes(code, B, N, M, L), 1))
        _lib.check(lib.aligner_path_cost_backward_f32(ptr(w), p.data_ptr(), t.data_ptr(), ij.data_ptr(), ln.data_ptr(), ptr(nn),
                                                      ptr(mm), code, scale, ptr(rs), ptr(dpred), ptr(dtarget), ws.data_ptr(),
                                                      ws.numel(), B, C, N, M, L, stream(dev)))
    return dpred, dtarget


class _DtwCostLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, pred, target, n, m, warp_penalty, bandwidth, scale, by_path):
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        # the cost table lives for these two lines: what is kept is the path
        cost, r, _ = _cost_and_path(kind, pred, target, n, m, warp_penalty, bandwidth, scale)
        del cost
        value = r.value
        if by_path:                      # the mean of the pair costs: the penalties steer the path and are not averaged
            _, total = path_cost(pred, target, r.path, r.length, n, m, kind, scale)
            value = total / r.length.clamp(min=1).to(torch.float32)
        if need:
            ctx.save_for_backward(pred, target, r.path, r.length)
        ctx.lengths = (n, m)
        ctx.kind, ctx.scale, ctx.by_path = kind, scale, by_path
        return value

    @staticmethod
    def backward(ctx, g_value):
        want = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if not (want[0] or want[1]) or g_value is None:
            return (None,) * 9
        pred, target, path, length = ctx.saved_tensors
        n, m = ctx.lengths
        g = g_value.detach().to(torch.float32)
        if ctx.by_path:
            g = g / length.clamp(min=1).to(torch.float32)
        # (an utterance without an alignment has no pairs and with them zero gradients, whatever its g)
        dpred, dtarget = path_cost_backward(None, pred, target, path, length, n, m, ctx.kind, ctx.scale, g, want)
        return (None, None if dpred is None else dpred.to(pred.dtype), None if dtarget is None else dtarget.to(target.dtype),
                None, None, None, None, None, None)


def _dtw_cost_loss(kind, pred, target, n, m, warp_penalty, bandwidth, scale, normalize, reduction, zero_infinity):
    if normalize not in ("none", "path"):
        raise ValueError("normalize must be 'none' or 'path'")
    check_reduction(reduction)
    value = _DtwCostLoss.apply(kind, pred, target, n, m, penalty(warp_penalty), bandwidth, scale, normalize == "path")
    return reduced(value, reduction, zero_infinity)


def dtw_l1_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                m: Optional[torch.Tensor] = None, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                scale: float = 1.0, normalize: str = "none", reduction: str = "mean",
                zero_infinity: bool = False) -> torch.Tensor:
    """Hard DTW on the L1 cost of pred [B,C,N] against target [B,C,M] as one autograd function: the gamma -> 0 limit of
    soft_dtw_l1_loss() / soft_dtw_l1_banded_loss().

    Forward: the cost table and the path exactly as dtw_path_l1() finds them -- l1_cost_banded() and dtw_path_banded()
    when 0 <= bandwidth <= 127 (any N), l1_cost() and dtw_path() otherwise (N <= 1024).  The table is dropped after the
    forward pass; what is saved is pred, target, the path and its length.  Backward: one path_cost_backward() call with
    the upstream gradient as row_scale; gradients come back in the inputs' dtypes, None for an input that does not
    require one.  The gradient is that of the value with the path held fixed: the derivative wherever the optimal path
    is unique, a subgradient at ties.

    normalize="none": the value is dtw_path_l1()'s value, bit for bit; the warp penalties are in it and have no
    gradient.  normalize="path": the value is the mean of the pair costs over the path's length[b] pairs (the MCD
    convention: the penalties steer the path and are not averaged).  An utterance without an alignment (a length below
    1, |n - m| > bandwidth) has value +inf and zero gradients; reduction and zero_infinity as in soft_dtw_loss()."""
    return _dtw_cost_loss(L1, pred, target, n, m, warp_penalty, bandwidth, scale, normalize, reduction, zero_infinity)


def dtw_l2_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                m: Optional[torch.Tensor] = None, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                scale: float = 1.0, normalize: str = "none", reduction: str = "mean", zero_infinity: bool = False,
                squared: bool = True) -> torch.Tensor:
    """dtw_l1_loss() on the Euclidean cost, squared (the default) or root: the path and the value of
    dtw_path_l2(..., squared=squared).  The root kind contributes no gradient from a pair at distance 0."""
    return _dtw_cost_loss(_kind(squared), pred, target, n, m, warp_penalty, bandwidth, scale, normalize, reduction, zero_infinity)


def mcd_dtw_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                 m: Optional[torch.Tensor] = None, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                 reduction: str = "mean", zero_infinity: bool = False) -> torch.Tensor:
    """Differentiable MCD-DTW in dB: dtw_l2_loss(squared=False, scale=10 sqrt(2) / ln 10, normalize="path"), the quantity
    mcd_dtw() reports, with a gradient.  The caller slices off c0 as there."""
    return dtw_l2_loss(pred, target, n, m, warp_penalty, bandwidth, MCD_SCALE, "path", reduction, zero_infinity, squared=False)
