#!/usr/bin/env python3
"""Time of ctc_forced_align() on one MI355X against the way the same alignment is computed without it, in one process:

    ctc_forced_align(log_probs, targets)                               the new kernel, emissions read in place
    log_probs.transpose(1,2).gather(...) into [B,L,T]  +  align_with_pauses(..., pause=log_probs[:,:,blank])   the yardstick

(the gather writes [B,L,T] in one pass; the form that gathers into [B,T,L] and transposes in a second pass is timed
beside it, and the ratio is taken against the faster of the two: which one that is depends on V)

at [64, L=200, T=1000] with V = 32 and V = 512, fp32 and bf16 (or B L T from the command line).  The transcripts have no
two equal neighbours, where the two searches are the same search: the tool checks that tok, durations, pauses and score
agree bit for bit before it times anything.  Device events around interleaved rounds, the median, minimum and maximum of
the per-call GPU time over the rounds; every call takes the next of a ring of input copies that is larger than the
on-package cache, so no call finds its emissions there.  The spread between the rounds of the yardstick is printed with
the ratio: a difference inside it is no difference."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

CACHE_BYTES = 256 << 20          # MI355X: 256 MiB of on-package cache in front of HBM


class Ring:
    """Copies of a tensor, handed out in turn; together at least twice the cache."""

    def __init__(self, t):
        n = max(2, min(128, -(-2 * CACHE_BYTES // max(t.numel() * t.element_size(), 1))))
        self.items = [t.clone() for _ in range(n)]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def rounds(variants, n_rounds=9, it=10, warm=3):
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
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def one(B, L, T, V, dtype, dev):
    g = torch.Generator().manual_seed(V)
    blank = 0
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * 3.0, dim=2).to(dtype).to(dev)
    # labels 1 .. V-1, no two neighbours equal: a random step of 1 .. V-2 from the label before
    step = torch.randint(1, V - 1, (B, L), generator=g)
    tg = ((torch.cumsum(step, 1) % (V - 1)) + 1).to(dev)
    assert not (tg[:, 1:] == tg[:, :-1]).any() and int(tg.min()) >= 1 and int(tg.max()) < V
    tx = torch.full((B,), L, dtype=torch.int32, device=dev)
    ty = torch.full((B,), T, dtype=torch.int32, device=dev)
    idx = tg[:, None, :].expand(B, T, L)
    idx_t = tg[:, :, None].expand(B, L, T)

    def yardstick(x):                                  # one pass: [B,L,T] written as it is gathered
        value = x.transpose(1, 2).gather(1, idx_t)
        return aligner_amd.align_with_pauses(value, tx, ty, pause=x[:, :, blank])

    def yardstick_two_pass(x):                         # gather into [B,T,L], then a transposing copy
        value = x.gather(2, idx).transpose(1, 2).contiguous()
        return aligner_amd.align_with_pauses(value, tx, ty, pause=x[:, :, blank])

    some = dict(want_labels=False, want_frame_scores=False, want_state_durations=False)
    new = aligner_amd.ctc_forced_align(lp, tg, ty, tx, blank)
    for ref in (yardstick(lp), yardstick_two_pass(lp)):
        for name in ("tok", "durations", "pauses"):
            assert torch.equal(getattr(new, name), getattr(ref, name)), name
        assert torch.equal(new.score.view(torch.int32), ref.score.view(torch.int32))
    ring = Ring(lp)
    pre = lp.transpose(1, 2).gather(1, idx_t)
    pre_ring = Ring(pre)
    pz = lp[:, :, blank].float().contiguous()
    variants = {
        "ctc_forced_align, all seven outputs": lambda: aligner_amd.ctc_forced_align(ring.next(), tg, ty, tx, blank),
        "ctc_forced_align, the yardstick's four outputs": lambda: aligner_amd.ctc_forced_align(ring.next(), tg, ty, tx, blank, **some),
        "yardstick: one-pass gather + align_with_pauses": lambda: yardstick(ring.next()),
        "(gather to [B,T,L] + transpose + align_with_pauses)": lambda: yardstick_two_pass(ring.next()),
        "(align_with_pauses alone, scores gathered before)": lambda: aligner_amd.align_with_pauses(pre_ring.next(), tx, ty, pause=pz),
    }
    res = rounds(variants)
    names = list(variants)
    print(f"[{B}, L={L}, T={T}], V={V}, {str(dtype).replace('torch.', '')}: GPU time per call, "
          f"{len(ring.items)} input copies in turn ({len(ring.items) * lp.numel() * lp.element_size() >> 20} MiB)")
    for name, (med, lo, hi) in res.items():
        print("    %-52s median %8.1f us  min %8.1f  max %8.1f" % (name, med, lo, hi))
    y = min(res[names[2]], res[names[3]])              # the faster of the yardstick's two forms at this shape
    print("    new / faster yardstick: %.2fx (all outputs), %.2fx (the same four); that yardstick's spread between rounds: %.1f %% of its median"
          % (res[names[0]][0] / y[0], res[names[1]][0] / y[0], 100.0 * (y[2] - y[1]) / y[0]))
    print("    blank frames: %.1f %%" % (100.0 * float((new.tok <= -2).sum()) / (B * T)))
    sys.stdout.flush()


def main():
    B, L, T = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (64, 200, 1000)
    dev = torch.device("cuda:0")
    for V in (32, 512):
        for dtype in (torch.float32, torch.bfloat16):
            one(B, L, T, V, dtype, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
