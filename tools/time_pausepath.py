#!/usr/bin/env python3
"""Time of align_with_pauses() on one MI355X against the two forms of the pause-free search, in one process:

    align_with_pauses(pause=-1.0, every gap allowed)
    align(force_generic=True, want_path=False, want_tok=True)      the kernel it shares its structure with
    align(want_path=False, want_tok=True)                          the pipelined search

at [64,200,1000] fp32 (or B Tx Ty from the command line).  Device events around interleaved rounds, median and minimum of
the per-call GPU time; then the forward / backtrack split of the new kernel and of the generic search from the
in-kernel stamps (aligner_debug_set_stamps: shader-clock cycles of wave 0, median over the utterances)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402


def rounds(variants, n_rounds=9, it=20, warm=5):
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


def stamps(fn, B):
    """Shader-clock stamps of wave 0 of every utterance's workgroup during one call: [B,16]."""
    lib = _lib.load()
    st = torch.zeros((2 * B, 16, 16), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    lib.aligner_debug_set_stamps(st.data_ptr())
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.aligner_debug_set_stamps(None)
    return st.cpu().numpy().astype(np.float64)[:B, 0]


def main():
    B, Tx, Ty = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (64, 200, 1000)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(B, Tx, Ty, generator=g) * 3.0, dim=1).to(dev)
    lp16 = lp.to(torch.bfloat16)
    pz = torch.full((B, Ty), -1.0, device=dev)
    tx = torch.full((B,), Tx, dtype=torch.int32, device=dev)
    ty = torch.full((B,), Ty, dtype=torch.int32, device=dev)
    variants = {
        "align_with_pauses(pause=-1.0)": lambda: aligner_amd.align_with_pauses(lp, tx, ty, pause=-1.0),
        "align(force_generic=True, want_tok=True)": lambda: aligner_amd.align(lp, tx, ty, force_generic=True, want_path=False, want_tok=True),
        "align(want_tok=True)": lambda: aligner_amd.align(lp, tx, ty, want_path=False, want_tok=True),
        "align_with_pauses(bf16, pause=-1.0)": lambda: aligner_amd.align_with_pauses(lp16, tx, ty, pause=-1.0),
        "align_with_pauses(pause=[B,Ty] tensor)": lambda: aligner_amd.align_with_pauses(lp, tx, ty, pause=pz),
        "align(bf16, force_generic=True, want_tok=True)": lambda: aligner_amd.align(lp16, tx, ty, force_generic=True, want_path=False, want_tok=True),
    }
    res = rounds(variants)
    print(f"[{B},{Tx},{Ty}], GPU time per call (fp32 unless named)")
    for name, (med, lo) in res.items():
        print("    %-48s median %8.1f us  min %8.1f us" % (name, med, lo))
    names = list(variants)
    print("    pause-aware / generic: %.2fx (bf16: %.2fx)   pause-aware / pipelined: %.2fx" %
          (res[names[0]][0] / res[names[1]][0], res[names[3]][0] / res[names[5]][0], res[names[0]][0] / res[names[2]][0]))
    r = aligner_amd.align_with_pauses(lp, tx, ty, pause=-1.0)
    print("    pause frames: %.1f %%" % (100.0 * float((r.tok <= -2).sum()) / (B * Ty)))
    # the forward / backtrack split: stamp 1 = sweep done, 3 = walk done (shader clock); 6 / 7 = the 100 MHz clock at the
    # workgroup's entry / exit (the pause kernel only), which turns its cycles into microseconds
    for name in (names[0], names[3], names[1]):
        s = stamps(variants[name], B)
        walk = np.median(s[:, 3] - s[:, 1])
        line = "    %-48s backtrack %8.0f cycles" % (name, walk)
        if (s[:, 7] > s[:, 6]).all():
            total_us = (s[:, 7] - s[:, 6]) / 100.0
            line += "; workgroup entry to exit %7.1f us (median over utterances)" % np.median(total_us)
        print(line)
    # forward cycles of the pause kernel: a stamp pair inside one clock domain needs the entry stamp too -- slot 0
    s = stamps(variants[names[0]], B)
    if (s[:, 0] > 0).all():
        print("    %-48s forward %9.0f cycles, backtrack %8.0f cycles, outputs %6.0f cycles (wave 0, median)" %
              (names[0], np.median(s[:, 1] - s[:, 0]), np.median(s[:, 3] - s[:, 1]), np.median(s[:, 5] - s[:, 3])))


if __name__ == "__main__":
    main()
