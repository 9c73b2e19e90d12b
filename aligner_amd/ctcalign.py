"""CTC forced alignment from emissions (aligner_ctc_align, include/aligner_amd.h).

    ctc_forced_align(log_probs, targets, input_lengths=None, target_lengths=None, blank=0, ...) -> CtcAlignment
    ctc_token_spans(res, input_lengths=None) -> (start, end, score, logp)

The Viterbi path of a transcript through the frame posteriors of a pretrained CTC acoustic model (wav2vec2, MMS, a
phoneme recogniser): the way duration-based TTS systems get their durations before training.  It computes what
torchaudio.functional.forced_align computes, for a whole batch per call, with repeated labels, ragged lengths and
16-bit or strided emissions read in place.  align_with_pauses() runs the same search over distinct states; here the
states come from a label sequence, and between two equal labels the blank is mandatory.  Computed by the HIP kernel in
csrc/ctcalign.hip; PyTorch only supplies device memory and streams, and there is no CPU implementation.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._operands import ptr, stream
from .maxpath import _SCORE_DTYPES, _TORCH_TO_DT

_workspaces = _lib.StreamWorkspaces(zero=False)      # decision words only: no status word, nothing to keep

_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


class CtcAlignment(NamedTuple):
    tok: Optional[torch.Tensor]               # [B,T] int32: x on a frame of token x, -2-g on a blank frame of gap g, -1 past t_y
    labels: Optional[torch.Tensor]            # [B,T] int32: the frame's vocabulary entry (targets[b,x] or blank), -1 past t_y
    frame_scores: Optional[torch.Tensor]      # [B,T] fp32: log_probs[b, y, labels[b,y]], 0 past t_y
    durations: Optional[torch.Tensor]         # [B,L] int32 frames per token
    pauses: Optional[torch.Tensor]            # [B,L+1] int32 blank frames per gap (gap g is the place before token g)
    state_durations: Optional[torch.Tensor]   # [B,2*L+1] int32, the two interleaved: even entries gaps, odd entries tokens
    score: Optional[torch.Tensor]             # [B] fp32 score of the path (-inf for an utterance without one)


def release_workspaces(device=None, stream=None) -> None:
    """Free the scratch buffers ctc_forced_align() keeps per (device, stream); see _lib.StreamWorkspaces."""
    _workspaces.release(device, stream)


def _lengths(t, n: int, B: int, device, name: str) -> torch.Tensor:
    if t is None:
        return torch.full((B,), n, dtype=torch.int32, device=device)
    t = torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()
    if t.numel() != B:
        raise ValueError(f"{name} must have one entry per utterance")
    return t


def ctc_forced_align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: Optional[torch.Tensor] = None,
                     target_lengths: Optional[torch.Tensor] = None, blank: int = 0, *,
                     want_tok: bool = True, want_labels: bool = True, want_frame_scores: bool = True,
                     want_durations: bool = True, want_pauses: bool = True, want_state_durations: bool = True,
                     want_score: bool = True) -> CtcAlignment:
    """Best CTC path of targets [B,L] through log_probs [B,T,V], a whole batch in one launch.

    log_probs: emissions on the GPU, any scores (they need not be normalised); fp32, bf16 and fp16 are read as they are
    and computed in fp32, other dtypes are cast to fp32 first.  The tensor is read in place whenever its last stride is
    1 and its frame stride is at least V -- a [T,B,V].transpose(0,1) view costs no copy; anything else is made
    contiguous.  targets: integer labels; input_lengths / target_lengths: [B], None meaning T / L.
    Between two equal labels the path must pass through the blank, so an utterance needs
    target_length + (number of repeats) <= input_length.  An utterance without a path -- that, a length below 1 or
    beyond the tensor, a label outside [0,V) -- gets zero durations and pauses, tok and labels -1, frame_scores 0 and
    score -inf; the rest of the batch is unaffected.  A label equal to `blank` is an ordinary label that happens to
    score the blank column: its frames are token frames (tok >= 0) of that token.
    Ties keep the earlier of stay / advance / skip and a NaN never wins, as in align_with_pauses(); the result is a
    legal path for any scores.  tok and state_durations follow PauseAlignment's conventions, so
    binarization_loss(value, res.tok, t_y) and regulate(h_interleaved, res.state_durations, T) take them unchanged.
    L <= 1024.  Asynchronous on the current stream; no autograd.
    """
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError(f"log_probs must be [B, T, V], got {tuple(getattr(log_probs, 'shape', ()))}")
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2:
        raise ValueError(f"targets must be [B, L], got {tuple(getattr(targets, 'shape', ()))}")
    if targets.dtype not in _INT_DTYPES:
        raise ValueError(f"targets must be an integer tensor, got {targets.dtype}")
    B, T, V = log_probs.shape
    if targets.shape[0] != B:
        raise ValueError(f"targets must be [B={B}, L], got {tuple(targets.shape)}")
    L = targets.shape[1]
    blank = int(blank)
    if not 0 <= blank < max(V, 1):
        raise ValueError(f"blank={blank} outside [0, V={V})")
    if not log_probs.is_cuda or not targets.is_cuda:
        raise ValueError("ctc_forced_align() takes GPU tensors")
    if not (want_tok or want_labels or want_frame_scores or want_durations or want_pauses or want_state_durations
            or want_score):
        raise ValueError("no output requested")
    if L > 1024:
        raise ValueError(f"L={L} too large (<= 1024)")
    device = log_probs.device
    with torch.no_grad(), torch.cuda.device(device):
        lp = log_probs.detach()
        if lp.dtype not in _SCORE_DTYPES:
            lp = lp.float()
        if not (V >= 1 and lp.stride(2) == 1 and (T <= 1 or lp.stride(1) >= V)):
            lp = lp.contiguous()
        stride_b = int(lp.stride(0)) if B > 1 else 0
        stride_t = max(int(lp.stride(1)), V) if T > 1 else V
        tg = targets.detach().to(device=device, dtype=torch.int32).contiguous()
        t_y = _lengths(input_lengths, T, B, device, "input_lengths")
        t_x = _lengths(target_lengths, L, B, device, "target_lengths")

        def out(shape, dtype, wanted):
            return torch.empty(shape, dtype=dtype, device=device) if wanted else None
        tok = out((B, T), torch.int32, want_tok)
        labels = out((B, T), torch.int32, want_labels)
        fscore = out((B, T), torch.float32, want_frame_scores)
        dur = out((B, L), torch.int32, want_durations)
        pauses = out((B, L + 1), torch.int32, want_pauses)
        sdur = out((B, 2 * L + 1), torch.int32, want_state_durations)
        score = out((B,), torch.float32, want_score)
        if B > 0 and L > 0 and T > 0 and V > 0:
            lib = _lib.load()
            nbytes = lib.aligner_ctc_align_workspace_bytes(B, L, T)
            ws = _workspaces.get(device, nbytes) if nbytes else None
            _lib.check(lib.aligner_ctc_align(
                lp.data_ptr(), _TORCH_TO_DT[lp.dtype], stride_b, stride_t, V, blank, tg.data_ptr(), t_x.data_ptr(),
                t_y.data_ptr(), ptr(tok), ptr(labels), ptr(fscore), ptr(dur), ptr(pauses), ptr(sdur), ptr(score),
                ptr(ws), ws.numel() if ws is not None else 0, B, L, T, stream(device)))
        else:
            # no launch: an empty batch, or utterances without a path (no label, no frame) -- the outputs the kernel
            # gives an infeasible utterance
            for t in (dur, pauses, sdur, fscore):
                if t is not None:
                    t.zero_()
            for t in (tok, labels):
                if t is not None:
                    t.fill_(-1)
            if score is not None:
                score.fill_(float("-inf"))
    return CtcAlignment(tok, labels, fscore, dur, pauses, sdur, score)


def ctc_token_spans(res: CtcAlignment, input_lengths: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(start [B,L] int32, end [B,L] int32, score [B,L] fp32, logp [B,L] fp32) of the tokens of an alignment.

    Token x owns the frames [start, end): the exclusive prefix sum of res.state_durations and that plus the token's own
    duration.  score is the mean over those frames of exp(frame_scores) -- merge_tokens() of the torchaudio forced
    alignment tutorial -- and logp their summed frame_scores; both come from segment_reduce() over the state durations
    (blank runs are segments of their own; the odd entries are the tokens').  A token without frames (an utterance
    without a path, a position past target_length) gets start == end, score 0 and logp 0.  res needs frame_scores and
    state_durations.  input_lengths is taken so that the call reads like ctc_forced_align()'s and is checked to hold one
    entry per utterance; the spans do not need it, res.state_durations already sum to it.
    """
    from .objective import segment_reduce
    if res.frame_scores is None or res.state_durations is None:
        raise ValueError("ctc_token_spans() needs frame_scores and state_durations")
    fs, sd = res.frame_scores, res.state_durations
    B, T = fs.shape
    L = (sd.shape[1] - 1) // 2
    if input_lengths is not None and torch.as_tensor(input_lengths).numel() != B:
        raise ValueError("input_lengths must have one entry per utterance")
    ends = torch.cumsum(sd, 1, dtype=torch.int32)
    end = ends[:, 1::2].contiguous()
    dur = sd[:, 1::2]
    start = (end - dur).contiguous()
    if B == 0 or L == 0 or T == 0:
        z = torch.zeros((B, L), dtype=torch.float32, device=fs.device)
        return start, end, z, z.clone()
    frames = torch.stack([fs.exp(), fs], 1)                           # [B,2,T]
    sums = segment_reduce(frames, sd)[:, :, 1::2]                     # [B,2,L]: the token segments
    score = sums[:, 0] / dur.clamp_min(1).to(torch.float32)
    return start, end, score.contiguous(), sums[:, 1].contiguous()
