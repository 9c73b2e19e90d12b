"""Hard alignment search with optional pauses between tokens (aligner_pausepath, include/aligner_amd.h).

    align_with_pauses(value, t_x, t_y, pause=-1.0, gap_mask=None, ...) -> PauseAlignment

The Viterbi path over the CTC topology of the token sequence: the decoding counterpart of the blank that
forward_sum(..., blank_logprob=...) trains with.  align() / maximum_path() put every frame on a token; here a frame
may also fall into the pause of a gap between two tokens (or before the first / after the last), and gaps can be
restricted, e.g. to word boundaries.  Computed by the HIP kernel in csrc/pausepath.hip; PyTorch only supplies device
memory and streams, and there is no CPU implementation.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Union

import torch

from . import _lib
from ._operands import ptr, stream
from .maxpath import _SCORE_DTYPES, _TORCH_TO_DT

_workspaces = _lib.StreamWorkspaces(zero=False)      # decision words only: no status word, nothing to keep


class PauseAlignment(NamedTuple):
    tok: Optional[torch.Tensor]               # [B,Ty] int32: x on a token frame, -2-g on a pause frame of gap g, -1 past t_y
    durations: Optional[torch.Tensor]         # [B,Tx] int32 frames per token
    pauses: Optional[torch.Tensor]            # [B,Tx+1] int32 frames per gap (gap g is the place before token g)
    state_durations: Optional[torch.Tensor]   # [B,2*Tx+1] int32, the two interleaved: even entries gaps, odd entries tokens
    score: Optional[torch.Tensor]             # [B] fp32 score of the path (-inf for an utterance without one)


def release_workspaces(device=None, stream=None) -> None:
    """Free the scratch buffers align_with_pauses() keeps per (device, stream); see _lib.StreamWorkspaces."""
    _workspaces.release(device, stream)


def align_with_pauses(value: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor,
                      pause: Union[float, torch.Tensor] = -1.0, gap_mask: Optional[torch.Tensor] = None, *,
                      want_tok: bool = True, want_durations: bool = True, want_pauses: bool = True,
                      want_state_durations: bool = False, want_score: bool = True) -> PauseAlignment:
    """Best monotonic path through value [B,Tx,Ty] with an optional pause in every allowed gap.

    value: scores (log-probabilities) on the GPU; fp32, bf16 and fp16 are read as they are and computed in fp32, other
    dtypes are cast to fp32 first; a row pitch of its own (softattn.pitched_logp()) is read in place, as align() does.
    t_x, t_y: [B] lengths.  pause: the score of a pause frame, one float or a [B,Ty] tensor.  gap_mask: [B,Tx+1] bool /
    uint8 / integer, nonzero where gap g (before token g; gap t_x trails) may hold a pause; None allows every gap.
    An utterance with t_x < 1, t_y < 1 or t_x > t_y gets zero durations, tok -1 and score -inf.
    The outputs go straight into the existing consumers: binarization_loss(logp, res.tok, t_y) skips pause frames, and
    regulate(h_interleaved, res.state_durations, T_mel) expands text encodings interleaved with a pause embedding.
    Asynchronous on the current stream.
    """
    if value.dim() != 3:
        raise ValueError(f"value must be [b, t_x, t_y], got {tuple(value.shape)}")
    if not value.is_cuda:
        raise ValueError("align_with_pauses() takes GPU tensors")
    if not (want_tok or want_durations or want_pauses or want_state_durations or want_score):
        raise ValueError("no output requested")
    device = value.device
    B, Tx, Ty = value.shape
    if Tx > 1024:
        raise ValueError(f"Tx={Tx} too large (<= 1024)")
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(device):
        v = value.detach()
        if v.dtype not in _SCORE_DTYPES:
            v = v.float()
        ld = Ty
        ldc = int(v.stride(1)) if Tx > 1 else int(v.stride(0))
        if (not v.is_contiguous() and v.stride(2) == 1 and ldc >= Ty and (B == 1 or v.stride(0) == Tx * ldc)):
            ld = ldc
        elif not v.is_contiguous():
            v = v.contiguous()
        t_x = t_x.to(device=device, dtype=torch.int32).contiguous()
        t_y = t_y.to(device=device, dtype=torch.int32).contiguous()
        if t_x.numel() != B or t_y.numel() != B:
            raise ValueError("t_x/t_y must have one entry per utterance")
        pz = None
        pause_score = 0.0
        if isinstance(pause, torch.Tensor):
            if tuple(pause.shape) != (B, Ty):
                raise ValueError(f"pause must be a float or [B,Ty], got {tuple(pause.shape)}")
            pz = pause.detach().to(device=device, dtype=torch.float32).contiguous()
        else:
            pause_score = float(pause)
        gm = None
        if gap_mask is not None:
            if tuple(gap_mask.shape) != (B, Tx + 1):
                raise ValueError(f"gap_mask must be [B,Tx+1], got {tuple(gap_mask.shape)}")
            gm = gap_mask.detach().to(device)
            gm = (gm if gm.dtype == torch.uint8 else (gm != 0).to(torch.uint8)).contiguous()

        def out(shape, dtype, wanted):
            return torch.empty(shape, dtype=dtype, device=device) if wanted else None
        tok = out((B, Ty), torch.int32, want_tok)
        dur = out((B, Tx), torch.int32, want_durations)
        pauses = out((B, Tx + 1), torch.int32, want_pauses)
        sdur = out((B, 2 * Tx + 1), torch.int32, want_state_durations)
        score = out((B,), torch.float32, want_score)
        if B > 0 and Tx > 0 and Ty > 0:
            nbytes = lib.aligner_pausepath_workspace_bytes(B, Tx, Ty)
            ws = _workspaces.get(device, nbytes) if nbytes else None
            _lib.check(lib.aligner_pausepath(
                v.data_ptr(), _TORCH_TO_DT[v.dtype], ld, ptr(pz), pause_score, ptr(gm), t_x.data_ptr(), t_y.data_ptr(),
                ptr(tok), ptr(dur), ptr(pauses), ptr(sdur), ptr(score),
                ptr(ws), ws.numel() if ws is not None else 0, B, Tx, Ty, stream(device)))
        else:
            # no launch: an empty batch, or utterances without a path (Tx == 0 or Ty == 0) -- the outputs the kernel
            # gives an infeasible utterance
            for t in (dur, pauses, sdur):
                if t is not None:
                    t.zero_()
            if tok is not None:
                tok.fill_(-1)
            if score is not None:
                score.fill_(float("-inf"))
    return PauseAlignment(tok, dur, pauses, sdur, score)
