"""Hard DTW (csrc/dtwpath.hip): the minimum-cost warping path between two frame sequences of different lengths and its
backtrack -- the hard counterpart of soft_dtw() / soft_dtw_banded() (their gamma -> 0 limit, which they cannot take),
as maximum_path() is the hard counterpart of forward_sum().  It is what an MCD-DTW or an L1-along-the-path evaluation
of a predicted spectrogram against a reference needs, with the cost, band and penalty the model was trained on.

For utterance b take n = n[b], m = m[b] (clamped as the soft calls clamp them), a warp penalty p (finite, >= 0) and an
optional band w.  Cell (i,j) exists iff i < n, j < m and |i - j| <= w.  All in float32, in exactly this order:

    a = R[i-1,j-1]                 (R[-1,-1] = 0; every other border cell +inf)
    b = R[i-1,j] + p
    c = R[i,j-1] + p
    best = a, k = 0;  if (b < best) { best = b; k = 1 }   if (c < best) { best = c; k = 2 }
    d = cost[i,j]
    R[i,j] = +inf            if the cell does not exist, or d is +inf or NaN, or best is +inf
           = best + d        otherwise
    value = R[n-1,m-1]

Ties: both comparisons are strict, so a tie prefers the diagonal, then the move that advances the row, then the move
that advances the column.  A -inf cost is legal and propagates; nothing computes inf - inf.  The path starts at
(n-1,m-1), follows k until (0,0) and is reported in ascending order; its length K satisfies max(n,m) <= K <= n+m-1.
An utterance without an alignment (a length below 1, |n - m| > w, a +inf value) has value +inf, length 0 and a path
of all -1.  Two additions and two comparisons per cell, no scaling: value, path and length are functions of the costs'
bits, the same in dense and in band storage (tests/dtwpath_oracle.py restates them in NumPy float32, bit for bit).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from ._operands import f32c, lengths, penalty, ptr, stream
from .banddtw import _bandwidth, l1_cost_banded
from .l1cost import l1_cost

_workspaces = _lib.StreamWorkspaces(zero=False)


class DtwPath(NamedTuple):
    value: torch.Tensor                 # [B] fp32
    path: Optional[torch.Tensor]        # [B,L,2] int32 (i,j) pairs, ascending, -1 past length; None without want_path
    length: Optional[torch.Tensor]      # [B] int32; None without want_path


def _empty(B: int, L: int, dev, want_path: bool) -> DtwPath:
    value = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
    if not want_path:
        return DtwPath(value, None, None)
    return DtwPath(value, torch.full((B, max(L, 0), 2), -1, dtype=torch.int32, device=dev),
                   torch.zeros((B,), dtype=torch.int32, device=dev))


def dtw_path(cost: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
             warp_penalty: float = 0.0, bandwidth: Optional[int] = None, want_path: bool = True) -> DtwPath:
    """DtwPath(value [B] fp32, path [B,N+M-1,2] int32, length [B] int32) of the module text.

    cost [B,N,M]: a GPU tensor (bf16 / fp16 are cast to fp32, a non-contiguous one is copied); n / m [B]: the
    utterances' lengths (None: N / M; larger values are clamped).  path[b,:length[b]] are the (i,j) pairs in ascending
    order, -1 beyond.  want_path=False: only the forward kernel runs, path and length are None, value has the same
    bits.  N <= 1024, B <= 65535, N*M < 2^29 (an AlignerError of code EDOM beyond).  One workgroup per utterance, no
    atomics: the same bits on every call.  Not attached to autograd.  Empty shapes return without a launch: value
    +inf, length 0.  Asynchronous on the current stream."""
    if not isinstance(cost, torch.Tensor) or cost.dim() != 3:
        raise ValueError("cost must be a [B,N,M] tensor")
    if not cost.is_floating_point():
        raise ValueError("cost must be a floating-point tensor")
    warp_penalty = penalty(warp_penalty)
    if bandwidth is not None and int(bandwidth) < 0:
        raise ValueError("bandwidth must be None (no band) or at least 0")
    if not cost.is_cuda:
        raise ValueError("cost must be a GPU tensor")
    band = -1 if bandwidth is None else min(int(bandwidth), 2 ** 30)
    B, N, M = cost.shape
    dev = cost.device
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0 or M == 0:
        return _empty(B, N + M - 1, dev, want_path)
    _lib.require_gpu()
    lib = _lib.load()
    c = f32c(cost)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    path = torch.empty((B, N + M - 1, 2), dtype=torch.int32, device=dev) if want_path else None
    length = torch.empty((B,), dtype=torch.int32, device=dev) if want_path else None
    with torch.cuda.device(dev):
        # (0 bytes: a shape outside the domain; the call itself reports which limit, as an AlignerError of code EDOM)
        ws = _workspaces.get(dev, max(lib.aligner_dtw_path_workspace_bytes(B, N, M), 1)) if want_path else None
        _lib.check(lib.aligner_dtw_path_f32(c.data_ptr(), ptr(nn), ptr(mm), warp_penalty, band, value.data_ptr(), ptr(path),
                                            ptr(length), ptr(ws), 0 if ws is None else ws.numel(), B, N, M, stream(dev)))
    return DtwPath(value, path, length)


def dtw_path_banded(cost_band: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                    warp_penalty: float = 0.0, want_path: bool = True) -> DtwPath:
    """dtw_path() on a cost in band storage (banddtw.py): cost_band [B,N,W], element [b,i,d] is cell (i, i + d - w),
    the bandwidth is w = (W - 1) / 2.  path is [B,2N+w-1,2].  n / m [B]: None means N for both (band storage does not
    know M); n is clamped to N, m to N + w.  value, path and length have the bits of dtw_path() on the dense image with
    bandwidth w.  An element whose cell does not exist is never read as a value.  bandwidth <= 127, B <= 65535,
    N*W < 2^29 (an AlignerError of code EDOM beyond) and no other limit on N."""
    if not isinstance(cost_band, torch.Tensor) or cost_band.dim() != 3:
        raise ValueError("cost_band must be a [B,N,W] tensor")
    if not cost_band.is_floating_point():
        raise ValueError("cost_band must be a floating-point tensor")
    if cost_band.shape[2] % 2 == 0:
        raise ValueError("cost_band must have an odd last dimension W = 2 bandwidth + 1")
    w = _bandwidth((cost_band.shape[2] - 1) // 2)
    warp_penalty = penalty(warp_penalty)
    if not cost_band.is_cuda:
        raise ValueError("cost_band must be a GPU tensor")
    B, N, _ = cost_band.shape
    dev = cost_band.device
    nn = lengths(n, B, dev, "n")
    mm = lengths(m, B, dev, "m")
    if B == 0 or N == 0:
        return _empty(B, 2 * N + w - 1, dev, want_path)
    _lib.require_gpu()
    lib = _lib.load()
    c = f32c(cost_band)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    path = torch.empty((B, 2 * N + w - 1, 2), dtype=torch.int32, device=dev) if want_path else None
    length = torch.empty((B,), dtype=torch.int32, device=dev) if want_path else None
    with torch.cuda.device(dev):
        ws = _workspaces.get(dev, max(lib.aligner_dtw_path_banded_workspace_bytes(B, N, w), 1)) if want_path else None
        _lib.check(lib.aligner_dtw_path_banded_f32(c.data_ptr(), ptr(nn), ptr(mm), warp_penalty, w, value.data_ptr(), ptr(path),
                                                   ptr(length), ptr(ws), 0 if ws is None else ws.numel(), B, N, stream(dev)))
    return DtwPath(value, path, length)


def dtw_path_l1(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                m: Optional[torch.Tensor] = None, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                scale: float = 1.0) -> DtwPath:
    """The DTW path of pred [B,C,N] against target [B,C,M] under the L1 cost of soft_dtw_l1_loss(): l1_cost_banded() and
    dtw_path_banded() when 0 <= bandwidth <= 127 (any N; path [B,2N+w-1,2]), l1_cost() and dtw_path() otherwise
    (N <= 1024; path [B,N+M-1,2]).  The cost tensor is dropped after the call.  Evaluation along the path:

        r = dtw_path_l1(pred, target, n, m, warp_penalty=p, bandwidth=w, scale=1 / C)
        for b in range(B):
            ij = r.path[b, :r.length[b]].long()                                     # [K,2]
            l1 = (pred[b][:, ij[:, 0]] - target[b][:, ij[:, 1]]).abs().mean()      # mean L1 distance along the path
        # on a cost tensor of one's own: cost[b, ij[:, 0], ij[:, 1]].sum() + p * (stalls) is value[b]

    or index any other pair of features with the same pairs and average.  For MCD-DTW, which aligns under the Euclidean
    distance of the mel cepstra themselves, mcd_dtw() (l2cost.py) is the call."""
    banded = bandwidth is not None and 0 <= int(bandwidth) <= 127
    if banded:
        cost = l1_cost_banded(pred, target, n, m, int(bandwidth), scale)
        if m is not None:                           # (the cost knows the target's M; the DP is told through m)
            m = torch.as_tensor(m).clamp(max=target.shape[2])
        else:
            m = torch.full((pred.shape[0],), target.shape[2], dtype=torch.int32, device=pred.device)
        return dtw_path_banded(cost, n, m, warp_penalty)
    return dtw_path(l1_cost(pred, target, n, m, bandwidth, scale), n, m, warp_penalty, bandwidth)


def path_to_dense(path: torch.Tensor, length: torch.Tensor, N: int, M: int) -> torch.Tensor:
    """[B,N,M] float32, 1 on the cells of each utterance's path and 0 elsewhere: the gamma -> 0 limit of soft_dtw()'s
    E.  Plain torch indexing, for inspection and tests; CPU tensors too."""
    if not isinstance(path, torch.Tensor) or path.dim() != 3 or path.shape[2] != 2:
        raise ValueError("path must be a [B,L,2] tensor")
    B, L, _ = path.shape
    if not isinstance(length, torch.Tensor) or length.numel() != B:
        raise ValueError("length must have one entry per utterance")
    out = torch.zeros((B, int(N), int(M)), dtype=torch.float32, device=path.device)
    on = torch.arange(L, device=path.device).view(1, L) < length.to(path.device).view(B, 1)
    b = torch.arange(B, device=path.device).view(B, 1).expand(B, L)[on]
    ij = path[on].long()
    out[b, ij[:, 0], ij[:, 1]] = 1.0
    return out
