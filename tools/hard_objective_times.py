#!/usr/bin/env python3
"""Timings of the hard half of the objective on one MI355X (called at the end of tools/config_times.py; runs alone too):
segment reduction at [64,512,200,1000] on the aligner's durations and on a skewed set (one token owns 90 % of the
frames), against the length regulator's forward at the same shape (the same bytes, the other way) and against the torch
formulation (index_add_ over tok); binarization loss and its gradient at [64,200,1000] against advanced indexing + autograd;
alignment_loss() against the unfused forward_sum_loss() + binarization_loss().  Device events around interleaved rounds of
every variant in one process; median and minimum over the rounds; bytes the algorithm needs over the median time."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

PEAK = 8.0e12          # HBM3E, bytes/s (spec)


def rounds(variants, n_rounds=7, it=20, warm=3):
    """variants: {name: fn}.  Interleaved rounds; returns {name: (median us, min us)}."""
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for _ in range(n_rounds):
        for name, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(it):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / it * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def report(title, res, nbytes):
    print(title)
    for name, (med, lo) in res.items():
        b = nbytes.get(name)
        rate = "" if b is None else "  %6.2f TB/s = %4.1f %% of the 8 TB/s peak (%.1f MB)" % (b / med / 1e6, 100 * b / (med * 1e-6) / PEAK, b / 1e6)
        print("    %-62s median %8.1f us  min %8.1f us%s" % (name, med, lo, rate))


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, C, Tx, Ty = 64, 512, 200, 1000
    lp = torch.log_softmax(torch.randn(B, Tx, Ty, generator=g) * 3.0, dim=1).to(dev)
    tx = torch.full((B,), Tx, dtype=torch.int32, device=dev)
    ty = torch.full((B,), Ty, dtype=torch.int32, device=dev)
    al = aligner_amd.align(lp, tx, ty, want_path=False, want_tok=True)
    dur, tok = al.durations, al.tok
    skew = torch.ones((B, Tx), dtype=torch.int32)
    skew[:, 0] = 0
    skew[:, 100:] = 0
    skew[:, 37] = Ty - 98                                        # 902 of the 1000 frames on one token
    skew = skew.to(dev)
    assert int(skew.sum(1).min()) == Ty and int(dur.sum(1).min()) == Ty
    frames = torch.randn(B, C, Ty, generator=g).to(dev)
    h = torch.randn(B, C, Tx, generator=g).to(dev)
    tok_skew = aligner_amd.regulate(h, skew, Ty)[1]
    idx, idx_skew = tok.long(), tok_skew.long()

    def torch_segment_sum(index):                                # torch yardstick 1: the batched scatter_add_ (atomics); the
        out = torch.zeros(B, C, Tx, device=dev)                  # zero-fill of the output is inside the timed region
        return out.scatter_add_(2, index[:, None, :].expand(B, C, Ty), frames)

    flat = (idx + torch.arange(B, device=dev)[:, None] * Tx).reshape(-1)

    flat_skew = (idx_skew + torch.arange(B, device=dev)[:, None] * Tx).reshape(-1)

    def torch_index_add(fl):                                     # torch yardstick 2: index_add_ wants one flat index, hence a
        out = torch.zeros(C, B * Tx, device=dev)                 # transposed copy of the frames: timed, as a user pays for it
        return out.index_add_(1, fl, frames.transpose(0, 1).reshape(C, B * Ty))

    moved = 4 * (B * C * Ty + B * C * Tx)
    res = rounds({
        "segment_reduce sum, aligner durations": lambda: aligner_amd.segment_reduce(frames, dur),
        "segment_reduce sum, skewed durations": lambda: aligner_amd.segment_reduce(frames, skew),
        "segment_reduce mean, aligner durations": lambda: aligner_amd.segment_reduce(frames, dur, mean=True),
        "regulate forward (the same bytes, the other way)": lambda: aligner_amd.regulate(h, dur, Ty),
        "torch scatter_add_ over tok, aligner durations": lambda: torch_segment_sum(idx),
        "torch scatter_add_ over tok, skewed durations": lambda: torch_segment_sum(idx_skew),
        "torch index_add_ (incl. transposed copy), aligner durations": lambda: torch_index_add(flat),
        "torch index_add_ (incl. transposed copy), skewed durations": lambda: torch_index_add(flat_skew),
    })
    report("segment reduction [%d,%d,%d,%d] fp32" % (B, C, Tx, Ty), res,
           {k: moved for k in res if not k.startswith("torch")})

    # the losses at [64,200,1000]
    from aligner_amd import objective
    x = lp.clone().requires_grad_(True)
    ar = torch.arange(Ty, device=dev)
    bi = torch.arange(B, device=dev)[:, None]

    def torch_bin(x):
        return -(x[bi, idx, ar[None, :]].clamp_min(objective.MIN_LOGP)).sum() / (B * Ty)

    def grad_of(fn):
        def run():
            (gx,) = torch.autograd.grad(fn(), x)
            return gx
        return run

    scale = torch.full((B,), 1.0 / (B * Ty), device=dev)
    gbuf = torch.empty(B, Tx, Ty, device=dev)
    lpd, ld = objective._logp_in_place(lp)
    res = rounds({
        "aligner_bin_loss (nll, count)": lambda: objective.bin_loss(lp, tok, ty),
        "aligner_bin_loss_grad_f32, whole tensor": lambda: objective._bin_loss_grad(lpd, ld, tok, ty, objective.MIN_LOGP, scale, gbuf, False),
        "aligner_bin_loss_grad_f32, accumulate": lambda: objective._bin_loss_grad(lpd, ld, tok, ty, objective.MIN_LOGP, scale, gbuf, True),
        "binarization_loss forward + backward": grad_of(lambda: aligner_amd.binarization_loss(x, tok, ty)),
        "torch indexing forward": lambda: torch_bin(lp),
        "torch indexing forward + backward": grad_of(lambda: torch_bin(x)),
    })
    report("binarization loss [%d,%d,%d] fp32" % (B, Tx, Ty), res,
           {"aligner_bin_loss_grad_f32, whole tensor": 4 * B * Tx * Ty})
    res = rounds({
        "alignment_loss forward + backward (one gradient tensor)": grad_of(lambda: aligner_amd.alignment_loss(x, tx, ty, tok)[0]),
        "forward_sum_loss + binarization_loss forward + backward": grad_of(
            lambda: aligner_amd.forward_sum_loss(x, tx, ty) + aligner_amd.binarization_loss(x, tok, ty)),
        "forward_sum_loss alone forward + backward": grad_of(lambda: aligner_amd.forward_sum_loss(x, tx, ty)),
    }, it=10)
    report("alignment objective [%d,%d,%d] fp32" % (B, Tx, Ty), res, {})


if __name__ == "__main__":
    main()
