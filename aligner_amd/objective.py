"""The steps either side of the alignment path, on the HIP path (build-defined
specs -- the reference snapshot only links the OTA paper, README.md:21-25,50):

    forward_sum(logp, t_x, t_y)          -log-likelihood of all monotonic alignments (+ gradient)
    beta_binomial_prior(t_x, t_y, ...)   the alignment prior soft_attention() can add
    regulate(h, durations, T_mel)        length regulator: expand text encodings to frames (differentiable in h)
    average_by_duration(frames, dur)     the other direction: per-token mean of frame-level features
    binarization_loss(logp, hard, ...)   -log soft-probability on the hard path (+ its sparse gradient)
    alignment_loss(logp, t_x, t_y, hard) forward-sum + binarization with one gradient tensor

All arithmetic runs in libaligner_amd.so; torch only owns the buffers.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib
from .maxpath import Alignment
from ._operands import lengths, ptr, stream
from .softattn import _chk

_fs_workspaces = _lib.StreamWorkspaces(zero=False, slack=1.0)


def _fs_workspace(device, nbytes: int) -> torch.Tensor:
    return _fs_workspaces.get(device, nbytes)          # one per (device, stream)


def _lengths(t, B: int, dev, name: str) -> torch.Tensor:
    """lengths(), for the entry points that require t_x / t_y and take them as [B] only."""
    if torch.as_tensor(t).shape != (B,):
        raise ValueError(f"{name} must have shape [{B}]")
    return lengths(t, B, dev, name)


def forward_sum(logp: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor, want_grad: bool = True,
                blank_logprob: Optional[float] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """loss[B] = -log sum over monotonic alignments of prod_y exp(logp[b, x(y), y]) and, if
    `want_grad`, d loss / d logp [B,T_text,T_mel] (= minus the posterior occupancy of each cell).

    blank_logprob (e.g. -1.0): the CTC form the OTA paper's code trains with instead -- a blank column at that
    log-prob before the text, every frame renormalised over blank + text, loss = CTC loss of the tokens 1..t_x;
    equal to torch.nn.functional.ctc_loss on log_softmax(pad(logp)), reduction "none" (tests/test_objective.py)."""
    _lib.require_gpu()
    lp = _chk(logp, "logp")
    if lp.dim() != 3:
        raise ValueError("logp must be [B, T_text, T_mel]")
    B, Tx, Ty = lp.shape
    dev = lp.device
    tx = _lengths(t_x, B, dev, "t_x")
    ty = _lengths(t_y, B, dev, "t_y")
    lib = _lib.load()
    ctc = blank_logprob is not None
    nws = (lib.aligner_forward_sum_ctc_workspace_bytes if ctc else lib.aligner_forward_sum_workspace_bytes)(B, Tx, Ty)
    if nws == 0 and B > 0:
        raise ValueError(f"unsupported shape B={B} T_text={Tx} T_mel={Ty} (T_text <= {1023 if ctc else 1024})")
    ws = _fs_workspace(dev, nws)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_grad else None
    if ctc:
        with torch.cuda.device(dev):
            _lib.check(lib.aligner_forward_sum_ctc_f32(lp.data_ptr(), tx.data_ptr(), ty.data_ptr(), float(blank_logprob),
                                                       loss.data_ptr(), ptr(grad), ws.data_ptr(), ws.numel(), B, Tx, Ty,
                                                       stream(dev)))
        return loss, grad
    with torch.cuda.device(dev):
        _lib.check(lib.aligner_forward_sum_f32(lp.data_ptr(), tx.data_ptr(), ty.data_ptr(), loss.data_ptr(),
                                               ptr(grad), ws.data_ptr(), ws.numel(), B, Tx, Ty, stream(dev)))
    return loss, grad


class _ForwardSumLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, t_x, t_y, blank_logprob):
        need = ctx.needs_input_grad[0]
        loss, grad = forward_sum(logp.detach(), t_x, t_y, want_grad=need, blank_logprob=blank_logprob)
        ctx.save_for_backward(grad if need else None)
        ctx.in_dtype = logp.dtype                   # (the kernels compute in fp32; a bf16 / fp16 logp gets its gradient back in its dtype)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (grad,) = ctx.saved_tensors
        if grad is None or g_loss is None:
            return None, None, None, None
        return (grad * g_loss.to(grad.dtype).view(-1, 1, 1)).to(ctx.in_dtype), None, None, None


def forward_sum_loss(logp: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor, blank_logprob: Optional[float] = -1.0,
                     reduction: str = "mean", zero_infinity: bool = False, length_normalize: bool = False) -> torch.Tensor:
    """The OTA aligner's ForwardSumLoss as an autograd function on the GPU kernels: forward_sum() with its gradient
    attached, so that `forward_sum_loss(logp, t_x, t_y).backward()` reaches whatever differentiable torch code produced
    `logp` -- alignment_encoder() / soft_attention() included: their backward is HIP as well (soft_attention_backward(),
    conv1d_backward()), so the gradient reaches the encoder weights.  One launch pair computes loss AND gradient in the forward pass (both sweeps side by side); backward()
    only scales.  blank_logprob = -1.0: the published CTC form (None: the plain monotonic form).  reduction: "mean" (a plain
    mean over the batch), "sum" or "none".  The two switches of torch.nn.CTCLoss that published aligner code is usually
    written with (neither the reference snapshot nor SNIPPETS.md holds that code: parity unpinned) are here as options, off
    by default: zero_infinity -- an infeasible utterance (t_x > t_y: loss +inf) contributes 0 and no gradient instead of
    making the batch loss +inf; length_normalize -- each utterance's loss is divided by its t_x (CTCLoss's own "mean")."""
    loss = _ForwardSumLoss.apply(logp, t_x, t_y, blank_logprob)
    if zero_infinity:
        loss = torch.where(torch.isinf(loss), torch.zeros_like(loss), loss)
    if length_normalize:
        loss = loss / torch.as_tensor(t_x).to(device=loss.device, dtype=loss.dtype).clamp_min(1)
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "none":
        return loss
    raise ValueError("reduction must be 'mean', 'sum' or 'none'")


def beta_binomial_prior(t_x: torch.Tensor, t_y: torch.Tensor, T_text: int, T_mel: int, scaling: float = 1.0
                        ) -> torch.Tensor:
    """prior[B,T_text,T_mel]: BetaBinomial(n=t_x, a=s*(y+1), b=s*(t_y-y)).pmf(x); 0 in the padding."""
    _lib.require_gpu()
    t_x = torch.as_tensor(t_x)
    if not t_x.is_cuda:
        raise ValueError("t_x must be a GPU tensor")
    dev = t_x.device
    B = t_x.shape[0]
    tx = _lengths(t_x, B, dev, "t_x")
    ty = _lengths(t_y, B, dev, "t_y")
    out = torch.empty((B, T_text, T_mel), dtype=torch.float32, device=dev)
    if B == 0:
        return out                                       # (an empty tensor has a null pointer, which the C ABI rejects)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aligner_beta_binomial_prior_f32(tx.data_ptr(), ty.data_ptr(), out.data_ptr(), B, T_text,
                                                               T_mel, float(scaling), stream(dev)))
    return out


def _durations(durations: torch.Tensor, B: int, Tx: int, dev) -> torch.Tensor:
    dur = torch.as_tensor(durations).detach().to(device=dev, dtype=torch.int32).contiguous()
    if dur.shape != (B, Tx):
        raise ValueError("durations must be [B, T_text]")
    return dur


def _regulate(hh: torch.Tensor, dur: torch.Tensor, T_mel: int, want_tok: bool = True):
    B, C, Tx = hh.shape
    dev = hh.device
    out = torch.empty((B, C, T_mel), dtype=torch.float32, device=dev)
    tok = torch.empty((B, T_mel), dtype=torch.int32, device=dev) if want_tok else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aligner_regulate_f32(hh.data_ptr(), dur.data_ptr(), out.data_ptr(),
                                                    ptr(tok), B, C, Tx, T_mel, stream(dev)))
    return out, tok


def segment_reduce(frames: torch.Tensor, durations: torch.Tensor, mean: bool = False) -> torch.Tensor:
    """tokens[B,C,T_text]: the sum (mean: the average) of frames[B,C,T_mel] over the frames each token owns under
    `durations` -- the segments of regulate(); a token without a frame gets 0 (aligner_segment_reduce_f32).  No
    autograd: regulate() and average_by_duration() are the differentiable faces."""
    _lib.require_gpu()
    ff = _chk(frames, "frames")
    if ff.dim() != 3:
        raise ValueError("frames must be [B, C, T_mel]")
    B, C, Ty = ff.shape
    dev = ff.device
    dur = torch.as_tensor(durations)
    if dur.dim() != 2:
        raise ValueError("durations must be [B, T_text]")
    Tx = dur.shape[1]
    dur = _durations(dur, B, Tx, dev)
    out = torch.empty((B, C, Tx), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aligner_segment_reduce_f32(ff.data_ptr(), dur.data_ptr(), out.data_ptr(), B, C, Tx, Ty,
                                                          1 if mean else 0, stream(dev)))
    return out


class _Regulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, dur, T_mel):
        out, tok = _regulate(_chk(h, "h"), dur, T_mel)
        ctx.save_for_backward(dur)
        ctx.in_dtype = h.dtype
        ctx.mark_non_differentiable(tok)
        return out, tok

    @staticmethod
    def backward(ctx, g_out, _g_tok):
        (dur,) = ctx.saved_tensors
        if g_out is None:
            return None, None, None
        return segment_reduce(g_out, dur, mean=False).to(ctx.in_dtype), None, None


def regulate(h: torch.Tensor, durations: torch.Tensor, T_mel: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out[B,C,T_mel], tok[B,T_mel]): out[b,:,y] = h[b,:,tok[b,y]]; frames past sum(durations[b]) are 0 / -1.
    Differentiable in `h` (a text encoder trains through it): the backward pass is the segment sum of the output's
    gradient over the same durations, in h's dtype."""
    _lib.require_gpu()
    if not h.is_cuda:
        raise ValueError("h must be a GPU tensor")
    if h.dim() != 3:
        raise ValueError("h must be [B, C, T_text]")
    B, C, Tx = h.shape
    dur = _durations(durations, B, Tx, h.device)
    if h.requires_grad and torch.is_grad_enabled():
        return _Regulate.apply(h, dur, T_mel)
    return _regulate(_chk(h, "h"), dur, T_mel)


class _AverageByDuration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames, dur):
        ctx.save_for_backward(dur)
        ctx.in_dtype = frames.dtype
        ctx.T_mel = frames.shape[2]
        return segment_reduce(frames, dur, mean=True)

    @staticmethod
    def backward(ctx, g):
        (dur,) = ctx.saved_tensors
        T_mel = ctx.T_mel
        # frames a token actually owns: its interval clipped to T_mel (a [B,T_text] computation)
        d = dur.clamp_min(0).to(torch.int64)
        end = d.cumsum(1)
        n = (end.clamp_max(T_mel) - (end - d).clamp_max(T_mel)).clamp_min(1).to(torch.float32)
        out, _ = _regulate((g.float() / n.unsqueeze(1)).contiguous(), dur, T_mel, want_tok=False)
        return out.to(ctx.in_dtype), None


def average_by_duration(frames: torch.Tensor, durations: torch.Tensor) -> torch.Tensor:
    """[B,C,T_text]: the mean of frames[B,C,T_mel] over the frames of each token (0 for a token without one) -- the
    per-token pitch / energy averaging of duration-based models, over the segments of regulate().  Differentiable
    in `frames`: the backward pass is the regulator applied to g / max(n_frames, 1)."""
    _lib.require_gpu()
    if not frames.is_cuda:
        raise ValueError("frames must be a GPU tensor")
    if frames.dim() != 3:
        raise ValueError("frames must be [B, C, T_mel]")
    dur = torch.as_tensor(durations)
    if dur.dim() != 2:
        raise ValueError("durations must be [B, T_text]")
    dur = _durations(dur, frames.shape[0], dur.shape[1], frames.device)
    if frames.requires_grad and torch.is_grad_enabled():
        return _AverageByDuration.apply(frames, dur)
    return segment_reduce(frames, dur, mean=True)


MIN_LOGP = math.log(1e-12)                 # the published log(clamp(soft, 1e-12))
_LOGP_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}


def _logp_in_place(logp: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(tensor the kernels can read, row pitch in elements): fp32 / bf16 / fp16 with the mel axis contiguous and
    uniformly pitched rows (contiguous, or pitched_logp()) is read where it is; anything else is copied."""
    if not logp.is_cuda:
        raise ValueError("logp must be a GPU tensor")
    if logp.dim() != 3:
        raise ValueError("logp must be [B, T_text, T_mel]")
    lp = logp.detach()
    if lp.dtype not in _LOGP_DTYPES:
        lp = lp.float()
    B, Tx, Ty = lp.shape
    ld = lp.stride(1)
    if not (lp.stride(2) == 1 and ld >= Ty and (B == 1 or lp.stride(0) == Tx * ld)) or Tx == 1:
        lp = lp.contiguous()
        ld = Ty
    return lp, ld


def _hard_tok(hard, B: int, Tx: int, Ty: int, dev) -> torch.Tensor:
    tok = hard.tok if isinstance(hard, Alignment) else hard
    if tok is None:
        raise ValueError("the Alignment has no tok: call align(..., want_tok=True)")
    tok = torch.as_tensor(tok).detach().to(dev)
    if tok.dim() == 3:                                  # a dense 0/1 path as maximum_path() returns it
        if tok.shape != (B, Tx, Ty):
            raise ValueError(f"a dense path must be [{B}, {Tx}, {Ty}]")
        on = tok != 0
        tok = torch.where(on.any(1), on.to(torch.uint8).argmax(1), -1)
    if tok.shape != (B, Ty) or tok.is_floating_point():
        raise ValueError(f"hard must be an Alignment, an integer [{B}, {Ty}] token-per-frame tensor or a dense path")
    return tok.to(torch.int32).contiguous()


def _bin_loss(lp: torch.Tensor, ld: int, tok: torch.Tensor, ty: Optional[torch.Tensor], min_logp: float
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """aligner_bin_loss on prepared operands: lp / ld from _logp_in_place(), tok int32 [B,T_mel], ty int32 [B] or None."""
    B, Tx, Ty = lp.shape
    dev = lp.device
    nll = torch.empty((B,), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aligner_bin_loss(lp.data_ptr(), _LOGP_DTYPES[lp.dtype], ld, tok.data_ptr(),
                                                ptr(ty), float(min_logp), nll.data_ptr(), count.data_ptr(), B, Tx, Ty,
                                                stream(dev)))
    return nll, count


def bin_loss(logp: torch.Tensor, tok: torch.Tensor, t_y: Optional[torch.Tensor] = None, min_logp: float = MIN_LOGP
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(nll[B] fp32, count[B] int32) of aligner_bin_loss: minus the summed max(logp, min_logp) at the cells
    (tok[b,y], y) of the frames that count, and how many count.  No autograd (binarization_loss() has it)."""
    _lib.require_gpu()
    lp, ld = _logp_in_place(logp)
    B, Tx, Ty = lp.shape
    tok = _hard_tok(tok, B, Tx, Ty, lp.device)
    ty = None if t_y is None else _lengths(t_y, B, lp.device, "t_y")
    return _bin_loss(lp, ld, tok, ty, min_logp)


def _bin_loss_grad(lp, ld, tok, ty, min_logp, scale, grad, accumulate):
    B, Tx, Ty = lp.shape
    dev = lp.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aligner_bin_loss_grad_f32(lp.data_ptr(), _LOGP_DTYPES[lp.dtype], ld, tok.data_ptr(),
                                                         ptr(ty), float(min_logp),
                                                         scale.data_ptr(), grad.data_ptr(), 1 if accumulate else 0,
                                                         B, Tx, Ty, stream(dev)))


class _BinLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, tok, ty, min_logp):
        lp, ld = _logp_in_place(logp)                        # (once: a copy, where one is needed, is also the saved tensor)
        nll, count = _bin_loss(lp, ld, tok, ty, min_logp)
        ctx.save_for_backward(lp, tok, ty)
        ctx.ld, ctx.min_logp, ctx.in_dtype = ld, min_logp, logp.dtype
        ctx.mark_non_differentiable(count)
        return nll, count

    @staticmethod
    def backward(ctx, g_nll, _g_count):
        lp, tok, ty = ctx.saved_tensors
        if g_nll is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        grad = torch.empty(lp.shape, dtype=torch.float32, device=lp.device)
        _bin_loss_grad(lp, ctx.ld, tok, ty, ctx.min_logp, g_nll.float().contiguous(), grad, accumulate=False)
        return grad.to(ctx.in_dtype), None, None, None


def binarization_loss(logp: torch.Tensor, hard, t_y: Optional[torch.Tensor] = None, min_logp: float = MIN_LOGP,
                      reduction: str = "mean") -> torch.Tensor:
    """The OTA aligner's binarization loss on the GPU kernels, with autograd: minus the log soft-probability
    max(logp, min_logp) at the cells of the hard path.  `hard`: an Alignment (its .tok: align(..., want_tok=True)), an
    integer [B,T_mel] token-per-frame tensor (-1 or >= T_text: the frame does not count), or a dense 0/1
    [B,T_text,T_mel] path as maximum_path() returns it.  t_y: frames at and past t_y[b] do not count.  reduction:
    "mean" -- sum(nll) / max(number of counting frames of the batch, 1), the published form -- "sum" or "none"
    (nll[B]).  min_logp = log(1e-12) is the published log(clamp(soft, 1e-12)) (parity unpinned); a cell below it
    contributes min_logp and no gradient.  The gradient is sparse -- one cell per frame -- and written as fp32 by one
    streaming pass (a 16-bit logp gets it converted to its dtype by a second, torch pass); logp (fp32 / bf16 / fp16,
    pitched_logp() included) is read in place."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    _lib.require_gpu()
    if not logp.is_cuda:
        raise ValueError("logp must be a GPU tensor")
    if logp.dim() != 3:
        raise ValueError("logp must be [B, T_text, T_mel]")
    B, Tx, Ty = logp.shape
    tok = _hard_tok(hard, B, Tx, Ty, logp.device)
    ty = None if t_y is None else _lengths(t_y, B, logp.device, "t_y")
    nll, count = _BinLoss.apply(logp, tok, ty, float(min_logp))
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return nll.sum() / count.sum().clamp_min(1).to(torch.float32)


class _AlignmentLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, t_x, t_y, tok, bin_weight, blank_logprob, min_logp):
        need = ctx.needs_input_grad[0]
        lp = _chk(logp, "logp")
        B = lp.shape[0]
        loss, grad = forward_sum(lp, t_x, t_y, want_grad=need, blank_logprob=blank_logprob)
        ty = _lengths(t_y, B, lp.device, "t_y")
        nll, count = _bin_loss(lp, lp.shape[2], tok, ty, min_logp)
        n = count.sum().clamp_min(1)
        fs_part = loss.mean()
        bin_part = nll.sum() / n.to(torch.float32)
        total = fs_part + bin_weight * bin_part
        if need:
            # backward() multiplies the whole tensor by g / B once (the forward-sum mean): the binarization term goes in
            # as -bin_weight * B / N, so that the one pass leaves g * (G_fs / B - bin_weight / N) on the path's cells
            scale = (float(bin_weight) * B / n.to(torch.float64)).to(torch.float32).expand(B).contiguous()
            _bin_loss_grad(lp, lp.shape[2], tok, ty, min_logp, scale, grad, accumulate=True)
        ctx.save_for_backward(grad if need else None)
        ctx.in_dtype, ctx.B = logp.dtype, B
        ctx.mark_non_differentiable(fs_part, bin_part)
        return total, fs_part, bin_part

    @staticmethod
    def backward(ctx, g_total, _g_fs, _g_bin):
        (grad,) = ctx.saved_tensors
        if grad is None or g_total is None:
            return (None,) * 7
        g_loss = (g_total.to(grad.dtype) / ctx.B).expand(ctx.B)           # what mean() hands each utterance
        return ((grad * g_loss.view(-1, 1, 1)).to(ctx.in_dtype),) + (None,) * 6


def alignment_loss(logp: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor, hard, bin_weight: float = 1.0,
                   blank_logprob: Optional[float] = -1.0, min_logp: float = MIN_LOGP
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(total, forward_sum_part, bin_part) of the OTA alignment objective: total = forward_sum_loss(logp, t_x, t_y,
    blank_logprob, reduction="mean") + bin_weight * binarization_loss(logp, hard, t_y, reduction="mean"), with ONE
    gradient tensor: the forward-sum kernels write theirs as in forward_sum_loss(), the binarization term is scattered
    into its path cells (aligner_bin_loss_grad_f32, accumulate) -- no zero-fill, no dense add, and backward() is the
    one scaling pass.  Only `total` carries the graph; the two parts are for logging."""
    _lib.require_gpu()
    if not logp.is_cuda:
        raise ValueError("logp must be a GPU tensor")
    if logp.dim() != 3:
        raise ValueError("logp must be [B, T_text, T_mel]")
    B, Tx, Ty = logp.shape
    tok = _hard_tok(hard, B, Tx, Ty, logp.device)
    return _AlignmentLoss.apply(logp, t_x, t_y, tok, float(bin_weight), blank_logprob, float(min_logp))
