#!/usr/bin/env python3
"""Time of hard DTW (aligner_amd.dtw_path / dtw_path_banded) against the soft call of the same storage form, on one
MI355X, in one process, on the same L1 cost tables:

    hard forward             aligner_dtw_path_f32 / aligner_dtw_path_banded_f32 without a path (the forward kernel alone)
    hard forward + path      the same with path and length (forward kernel writing its decisions, then the backtrack)
    soft forward + E A / B   aligner_soft_dtw_f32 / aligner_soft_dtw_banded_f32 with the expected alignment -- the only
                             other way this library yields an alignment -- measured twice: the difference of the two
                             medians is the spread the gate allows

at [B,C,N,M] = [16,80,1000,1000] and [64,80,200,1000] dense (no band) and [16,80,1000,1000] and [16,80,4000,4000] in
band storage with w = 60; gamma 1, penalty 0.1, full lengths.  All through the C ABI on buffers allocated once, every call
on the next of enough copies of the cost table to exceed the 256 MiB on-package cache.  Device events around `it` calls,
seven interleaved rounds after a warm-up, the median (and minimum) of the per-call GPU time.

Gate: hard forward + path <= soft forward + E + spread.  The backtrack runs one wave per utterance side by side, so its
time is that of the longest path: ns per step = (forward + path - forward) / max K.  Prints a table and, last, one JSON
line: python tools/dtwpath_time.py | tee profiles/dtwpath_times.txt.  Fails without a GPU."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402

CACHE_BYTES = 256 * 2 ** 20
GAMMA, PENALTY, SCALE = 1.0, 0.1, 1.0 / 80


def rounds(variants, n_rounds=7, warm=2):
    times = {k: [] for k in variants}
    for fn, _ in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for _ in range(n_rounds):
        for name, (fn, it) in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(it):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / it * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def copies(t):
    """Enough copies of t that one turn through them exceeds the cache."""
    n = int(CACHE_BYTES * 2.25 / (t.numel() * t.element_size())) + 1
    return [t.clone() for _ in range(n)]


def one_shape(B, C, N, M, w, dev):
    """w: None for the dense calls without a band, else band storage of that bandwidth."""
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.uniform(0, 1, (B, C, N)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(0, 1, (B, C, M)).astype(np.float32)).to(dev)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    banded = w is not None
    if banded:
        tables = copies(aligner_amd.l1_cost_banded(pred, target, None, None, w, SCALE))
        L = 2 * N + w - 1
        ws_hard = lib.aligner_dtw_path_banded_workspace_bytes(B, N, w)
        ws_soft = lib.aligner_soft_dtw_banded_workspace_bytes(B, N, w, 1)
    else:
        tables = copies(aligner_amd.l1_cost(pred, target, None, None, None, SCALE))
        L = N + M - 1
        ws_hard = lib.aligner_dtw_path_workspace_bytes(B, N, M)
        ws_soft = lib.aligner_soft_dtw_workspace_bytes(B, N, M, 1)
    grads = [torch.empty_like(t) for t in tables]
    ms = torch.full((B,), M, dtype=torch.int32, device=dev)
    value = torch.empty(B, device=dev)
    path = torch.empty((B, L, 2), dtype=torch.int32, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    hws = torch.empty(max(ws_hard, 1), dtype=torch.uint8, device=dev)
    sws = torch.empty(max(ws_soft, 1), dtype=torch.uint8, device=dev)
    turn = [0]

    def hard(want_path):
        k = turn[0] = (turn[0] + 1) % len(tables)
        out = (value.data_ptr(), path.data_ptr() if want_path else None, length.data_ptr() if want_path else None,
               hws.data_ptr() if want_path else None, hws.numel() if want_path else 0)
        if banded:
            _lib.check(lib.aligner_dtw_path_banded_f32(tables[k].data_ptr(), None, ms.data_ptr(), PENALTY, w, *out, B, N, stream))
        else:
            _lib.check(lib.aligner_dtw_path_f32(tables[k].data_ptr(), None, None, PENALTY, -1, *out, B, N, M, stream))

    def soft():
        k = turn[0] = (turn[0] + 1) % len(tables)
        if banded:
            _lib.check(lib.aligner_soft_dtw_banded_f32(tables[k].data_ptr(), None, ms.data_ptr(), GAMMA, PENALTY, w, value.data_ptr(),
                                                       grads[k].data_ptr(), sws.data_ptr(), sws.numel(), B, N, stream))
        else:
            _lib.check(lib.aligner_soft_dtw_f32(tables[k].data_ptr(), None, None, GAMMA, PENALTY, -1, value.data_ptr(),
                                                grads[k].data_ptr(), sws.data_ptr(), sws.numel(), B, N, M, stream))

    variants = {"soft forward + E A": (soft, 10), "hard forward": (lambda: hard(False), 10),
                "hard forward + path": (lambda: hard(True), 10), "soft forward + E B": (soft, 10)}
    res = rounds(variants)
    hard(True)
    torch.cuda.synchronize()
    K = length.cpu().numpy()
    assert (K > 0).all()
    form = f"band storage, bandwidth {w}" if banded else "dense, no band"
    print(f"[{B},{C},{N},{M}] {form}: path lengths {int(K.min())} .. {int(K.max())}, decisions {ws_hard / 1e6:.1f} MB")
    for name, (med, lo) in res.items():
        print("    %-24s median %10.1f us  min %10.1f us" % (name, med, lo))
    a, b = res["soft forward + E A"][0], res["soft forward + E B"][0]
    f, fp = res["hard forward"][0], res["hard forward + path"][0]
    spread = abs(a - b)
    met = bool(fp <= min(a, b) + spread)
    share, per_step = (fp - f) / fp, (fp - f) * 1e3 / int(K.max())
    print(f"    gate: hard forward + path {fp:.1f} us against soft forward + E {min(a, b):.1f} us + spread {spread:.1f} us: "
          f"{'met' if met else 'MISSED'}")
    print(f"    decisions + backtrack: {fp - f:.1f} us, {100 * share:.1f}% of the call, {per_step:.1f} ns a step of the longest path")
    return {"shape": [B, C, N, M], "bandwidth": w, "us": {k: {"median": round(med, 1), "min": round(lo, 1)} for k, (med, lo) in res.items()},
            "path_length": {"min": int(K.min()), "max": int(K.max())},
            "gate": {"soft_us": round(min(a, b), 1), "spread_us": round(spread, 1), "hard_us": round(fp, 1), "met": met},
            "backtrack_share": round(share, 3), "ns_per_step": round(per_step, 1)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dtwpath_time.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [(16, 80, 1000, 1000, None), (64, 80, 200, 1000, None), (16, 80, 1000, 1000, 60), (16, 80, 4000, 4000, 60)]
    if len(sys.argv) > 4:
        B, C, N, M = (int(a) for a in sys.argv[1:5])
        shapes = [(B, C, N, M, int(sys.argv[5]) if len(sys.argv) > 5 else None)]
    out = []
    for B, C, N, M, w in shapes:
        out.append(one_shape(B, C, N, M, w, dev))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "dtwpath_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
