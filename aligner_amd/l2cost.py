"""The Euclidean cost tables of Soft-DTW and hard DTW (csrc/l1cost.hip and csrc/banddtw.hip, instantiated on the kinds
of csrc/costkind.h), their gradient, the losses in one piece, and MCD-DTW.  Everything that is not the cell's own
arithmetic -- channel-major layout pred [B,C,N], target [B,C,M], lengths, band, fill values, band storage, domains --
is l1cost.py's and banddtw.py's, through the same helpers.

    squared:  cost[b,i,j] = scale      sum_c (pred[b,c,i] - target[b,c,j])^2        on existing cells
    root:     cost[b,i,j] = scale sqrt(sum_c (pred[b,c,i] - target[b,c,j])^2)
              +inf inside the lengths and outside the band (dense); 0 at or past n[b] or m[b]; band storage: 0 wherever
              no cell exists

    squared, backward, with G = grad_cost and g = row_scale:
    dpred[b,c,i]   =  2 g[b] scale sum_j G[b,i,j] (pred[b,c,i] - target[b,c,j])     over the existing cells of row i
    dtarget[b,c,j] = -2 g[b] scale sum_i G[b,i,j] (pred[b,c,i] - target[b,c,j])     over the existing cells of column j

The squared kind is the cost Soft-DTW was defined with; what it replaces is torch.cdist(p=2) ** 2 in front of
soft_dtw_loss(), which builds and keeps the whole [B,N,M] table whatever the band and does not exist in band storage.
The root kind is the distance MCD-DTW averages.  As a table it is forward only: its gradient needs the finished table
back and is singular at distance 0.  Along a warping path it has one (pathcost.py: mcd_dtw_loss()).

The cell is the direct form, d = target - pred and acc = fma(d, d, acc) over the channels in order, in fp32 on the
vector ALU: its error is relative to the distance itself.  (gaussian_logp with a zero log-std is also a scaled squared
distance, but through |x|^2 + |y|^2 - 2 x.y, whose error is relative to the norms: wrong for DTW, which walks exactly
the cells where pred is close to target.)
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._operands import penalty
from .banddtw import (_bandwidth, _cost_banded, _cost_banded_backward, _dp_columns, _soft_dtw_cost_banded_loss)
from .dtwpath import DtwPath, dtw_path, dtw_path_banded
from .l1cost import L2, L2_ROOT, _cost, _cost_backward, _soft_dtw_cost_loss

MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)          # dB per unit of Euclidean cepstral distance


def _kind(squared) -> str:
    return L2 if squared else L2_ROOT


def l2_cost(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
            bandwidth: Optional[int] = None, scale: float = 1.0, squared: bool = True) -> torch.Tensor:
    """cost [B,N,M] of the module text, fp32, squared or root; every cell is written.

    Operands, lengths, band and domain as in l1_cost(): GPU tensors (bf16 / fp16 are cast to fp32), B <= 65535,
    C <= 4096, N*M < 2^29.  Not attached to autograd (soft_dtw_l2_loss() is, for the squared kind).  Asynchronous on
    the current stream."""
    return _cost(_kind(squared), pred, target, n, m, bandwidth, scale)


def l2_cost_backward(grad_cost: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                     m: Optional[torch.Tensor] = None, bandwidth: Optional[int] = None, scale: float = 1.0,
                     row_scale: Optional[torch.Tensor] = None, want: Tuple[bool, bool] = (True, True)
                     ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(dpred [B,C,N] or None, dtarget [B,C,M] or None) of the squared cost, fp32, with G = grad_cost [B,N,M].

    Arguments as in l1_cost_backward().  G is masked by "the cell exists" before it is used, and rows and columns are
    taken from inside the lengths: a NaN in G where no cell exists, or in the padding of pred / target, reaches nothing.
    One owner per output element, no atomics: the same bits on every call, and each output has the bits it has beside
    the other.  The root cost has no gradient (module text)."""
    return _cost_backward(L2, grad_cost, pred, target, n, m, bandwidth, scale, row_scale, want)


def soft_dtw_l2_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                     m: Optional[torch.Tensor] = None, gamma: float = 1.0, warp_penalty: float = 0.0,
                     bandwidth: Optional[int] = None, scale: float = 1.0, reduction: str = "mean",
                     zero_infinity: bool = False) -> torch.Tensor:
    """Soft-DTW on the squared Euclidean cost of pred [B,C,N] against target [B,C,M] as one autograd function:
    soft_dtw_l1_loss() with l2_cost() / l2_cost_backward() in place of the L1 calls.  What is saved is pred, target, E
    and the lengths: no cost tensor and no cdist graph.  Arguments, reductions and domain (N <= 1024) as there; past
    1024 frames soft_dtw_l2_banded_loss() is the path."""
    return _soft_dtw_cost_loss(L2, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity)


def l2_cost_banded(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                   m: Optional[torch.Tensor] = None, bandwidth: int = 60, scale: float = 1.0,
                   squared: bool = True) -> torch.Tensor:
    """cost_band [B,N,W] in band storage (banddtw.py), fp32, squared or root: on the cells that exist the bits of
    dense_to_band(l2_cost(..., bandwidth=w)), exactly 0 elsewhere.  Operands, clamps (m to M and to N + w) and domain as
    in l1_cost_banded(): bandwidth <= 127, any N."""
    return _cost_banded(_kind(squared), pred, target, n, m, bandwidth, scale)


def l2_cost_banded_backward(grad_band: torch.Tensor, pred: torch.Tensor, target: torch.Tensor,
                            n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None, scale: float = 1.0,
                            row_scale: Optional[torch.Tensor] = None, want: Tuple[bool, bool] = (True, True)
                            ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """l2_cost_backward() with G = grad_band [B,N,W] in band storage (the bandwidth is (W - 1) / 2); arguments as in
    l1_cost_banded_backward()."""
    return _cost_banded_backward(L2, grad_band, pred, target, n, m, scale, row_scale, want)


def soft_dtw_l2_banded_loss(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                            m: Optional[torch.Tensor] = None, gamma: float = 1.0, warp_penalty: float = 0.0,
                            bandwidth: int = 60, scale: float = 1.0, reduction: str = "mean",
                            zero_infinity: bool = False) -> torch.Tensor:
    """soft_dtw_l2_loss() in band storage: soft_dtw_l1_banded_loss() on the squared Euclidean cost.  [B,N,2w+1] saved
    where the dense function keeps [B,N,M]; any N, bandwidth <= 127.  The forward value has the dense loss's bits."""
    return _soft_dtw_cost_banded_loss(L2, pred, target, n, m, gamma, warp_penalty, bandwidth, scale, reduction, zero_infinity)


def _banded(bandwidth) -> bool:
    return bandwidth is not None and 0 <= int(bandwidth) <= 127


def _cost_and_path(kind, pred, target, n, m, warp_penalty, bandwidth, scale):
    """(cost, DtwPath, in band storage?): band storage when 0 <= bandwidth <= 127, dense otherwise, as dtw_path_l1()."""
    warp_penalty = penalty(warp_penalty)
    if _banded(bandwidth):
        cost = _cost_banded(kind, pred, target, n, m, _bandwidth(bandwidth), scale)
        return cost, dtw_path_banded(cost, n, _dp_columns(m, pred, target), warp_penalty), True
    cost = _cost(kind, pred, target, n, m, bandwidth, scale)
    return cost, dtw_path(cost, n, m, warp_penalty, bandwidth), False


def dtw_path_l2(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None,
                m: Optional[torch.Tensor] = None, warp_penalty: float = 0.0, bandwidth: Optional[int] = None,
                scale: float = 1.0, squared: bool = False) -> DtwPath:
    """The DTW path of pred [B,C,N] against target [B,C,M] under the Euclidean cost (root by default, squared on
    request): l2_cost_banded() and dtw_path_banded() when 0 <= bandwidth <= 127 (any N; path [B,2N+w-1,2]), l2_cost()
    and dtw_path() otherwise (N <= 1024; path [B,N+M-1,2]), exactly as dtw_path_l1() dispatches.  The cost tensor is
    dropped after the call; mcd_dtw() keeps it for the mean along the path."""
    return _cost_and_path(_kind(squared), pred, target, n, m, warp_penalty, bandwidth, scale)[1]


def mcd_dtw(pred: torch.Tensor, target: torch.Tensor, n: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
            warp_penalty: float = 0.0, bandwidth: Optional[int] = None) -> Tuple[torch.Tensor, DtwPath]:
    """(mcd [B] fp32 in dB, DtwPath): mel-cepstral distortion along the DTW path, the objective metric of TTS evaluation.

    pred [B,C,N], target [B,C,M]: the mel cepstra of the synthesised and the reference utterances, channels first.  By
    the metric's convention the energy coefficient c0 is not part of it: the caller slices it off first
    (pred[:, 1:], target[:, 1:]).  The path is dtw_path_l2()'s under the root cost with scale = 10 sqrt(2) / ln 10, so
    that a cell's cost is that frame pair's distortion in dB, and mcd[b] is the mean of the cost over the path's
    length[b] cells -- gathered from the cost tensor for the whole batch at once, and independent of warp_penalty
    except through the path.  An utterance without an alignment (a length below 1, |n - m| > bandwidth) has mcd +inf.
    Storage form, domain and path layout as in dtw_path_l2(); not attached to autograd."""
    cost, r, banded = _cost_and_path(L2_ROOT, pred, target, n, m, warp_penalty, bandwidth, MCD_SCALE)
    B, L = r.path.shape[0], r.path.shape[1]
    on = torch.arange(L, device=cost.device).view(1, L) < r.length.view(B, 1)
    if cost.numel() == 0 or L == 0:
        return torch.full((B,), float("inf"), dtype=torch.float32, device=cost.device), r
    ij = r.path.long().clamp_(min=0)                            # (-1 past the length: gathered from cell (0,0), not added)
    i, j = ij[..., 0], ij[..., 1]
    col = j - i + int(bandwidth) if banded else j
    at = cost[torch.arange(B, device=cost.device).view(B, 1), i, col.clamp_(0, cost.shape[2] - 1)]
    total = torch.where(on, at, torch.zeros_like(at)).sum(1)
    mcd = torch.where(r.length > 0, total / r.length.clamp(min=1).to(torch.float32), torch.full_like(total, float("inf")))
    return mcd, r
