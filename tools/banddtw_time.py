#!/usr/bin/env python3
"""Time and memory of the band-storage Soft-DTW against the dense functions of the same tree, on one MI355X, in one
process, on the same inputs, bandwidth 60:

    forward / forward + E, C ABI     aligner_soft_dtw_f32 (bandwidth 60) on the dense table against
                                     aligner_soft_dtw_banded_f32 on band storage, buffers allocated once, every call on
                                     the next of enough copies of the table to exceed the 256 MiB on-package cache
    loss step                        soft_dtw_l1_loss(...).backward() against soft_dtw_l1_banded_loss(...).backward()
                                     (inputs rotated past the cache; the tables are the caching allocator's)
    the three cost kernels           aligner_l1_cost_banded_f32, and aligner_l1_cost_banded_backward_f32 for dpred alone
                                     and dtarget alone, inputs, G and outputs allocated once and rotated in the same way
    peak memory of one loss step     torch.cuda.max_memory_allocated above what was allocated when the step began, the
                                     gradients of earlier steps freed first: the cost table and R / E, the two input
                                     gradients and the small per-utterance tensors

at [B,C,N,M] = [16,80,1000,1000] (the gate), [64,80,1000,1000] and [16,80,4000,4000] (band only: the dense DP stops at
1024 rows), gamma 1, penalty 0.1, full lengths.  Device events around `it` calls, seven interleaved rounds after a
warm-up, the median (and minimum) of the per-call GPU time.  Every dense variant runs twice ("A" and "B"): the
difference of the two medians is the spread the gate allows.  Prints a table and, last, one JSON line:
python tools/banddtw_time.py | tee profiles/banddtw_times.txt.  Fails without a GPU."""
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


def copies(t, together=1):
    """Enough copies of t that one turn through them (with `together` tensors of that size a call) exceeds the cache."""
    n = int(CACHE_BYTES * 2.25 / (t.numel() * t.element_size() * together)) + 1
    return [t.clone() for _ in range(n)]


def peak_of(step, inputs):
    for t in inputs:                                   # (the gradients of earlier steps are not this step's memory)
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def one_shape(B, C, N, M, w, dev, dense):
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.uniform(0, 1, (B, C, N)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(0, 1, (B, C, M)).astype(np.float32)).to(dev)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    W = 2 * w + 1
    value = torch.empty(B, device=dev)
    variants = {}

    bands = copies(aligner_amd.l1_cost_banded(pred, target, None, None, w, SCALE))
    bgrads = [torch.empty_like(t) for t in bands]
    ms = torch.full((B,), M, dtype=torch.int32, device=dev)
    bws = torch.empty(max(lib.aligner_soft_dtw_banded_workspace_bytes(B, N, w, 1), 1), dtype=torch.uint8, device=dev)
    turn = [0, 0, 0]

    def band_raw(grad):
        k = turn[0] = (turn[0] + 1) % len(bands)
        _lib.check(lib.aligner_soft_dtw_banded_f32(bands[k].data_ptr(), None, ms.data_ptr(), GAMMA, PENALTY, w, value.data_ptr(),
                                                   bgrads[k].data_ptr() if grad else None, bws.data_ptr(), bws.numel(), B, N, stream))

    preds, targets = copies(pred, 2), copies(target, 2)

    def loss_step(fn):
        k = turn[1] = (turn[1] + 1) % len(preds)
        p, t = preds[k].requires_grad_(), targets[k].requires_grad_()
        p.grad = t.grad = None
        fn(p, t, None, None, GAMMA, PENALTY, w, SCALE, reduction="sum").backward()

    if dense:
        costs = copies(aligner_amd.l1_cost(pred, target, None, None, w, SCALE))
        grads = [torch.empty_like(t) for t in costs]
        ws = torch.empty(max(lib.aligner_soft_dtw_workspace_bytes(B, N, M, 1), 1), dtype=torch.uint8, device=dev)

        def dense_raw(grad):
            k = turn[2] = (turn[2] + 1) % len(costs)
            _lib.check(lib.aligner_soft_dtw_f32(costs[k].data_ptr(), None, None, GAMMA, PENALTY, w, value.data_ptr(),
                                                grads[k].data_ptr() if grad else None, ws.data_ptr(), ws.numel(), B, N, M, stream))

        for ab in "AB":
            variants[f"dense forward {ab}"] = (lambda: dense_raw(False), 10)
            variants[f"dense forward + E {ab}"] = (lambda: dense_raw(True), 10)
            variants[f"dense loss step {ab}"] = (lambda: loss_step(aligner_amd.soft_dtw_l1_loss), 5)
    variants["band forward"] = (lambda: band_raw(False), 10)
    variants["band forward + E"] = (lambda: band_raw(True), 10)
    variants["band loss step"] = (lambda: loss_step(aligner_amd.soft_dtw_l1_banded_loss), 5)
    # the cost kernels through the C ABI on buffers allocated once: inputs, G and outputs all rotated
    cpreds = copies(pred, 4)
    ctargets, couts, cdp, cdt = ([torch.empty_like(t) for _ in cpreds] for t in (target, bands[0], pred, target))
    for t in ctargets:
        t.copy_(target)
    cG = [torch.rand(B, N, W, device=dev) for _ in cpreds]
    cturn = [0]

    def cost_raw(which):
        k = cturn[0] = (cturn[0] + 1) % len(cpreds)
        if which == "cost":
            _lib.check(lib.aligner_l1_cost_banded_f32(cpreds[k].data_ptr(), ctargets[k].data_ptr(), None, None, w, SCALE,
                                                      couts[k].data_ptr(), B, C, N, M, stream))
        else:
            _lib.check(lib.aligner_l1_cost_banded_backward_f32(cG[k].data_ptr(), cpreds[k].data_ptr(), ctargets[k].data_ptr(), None, None,
                                                               w, SCALE, None, cdp[k].data_ptr() if which == "dpred" else None,
                                                               cdt[k].data_ptr() if which == "dtarget" else None, B, C, N, M, stream))

    variants["band cost"] = (lambda: cost_raw("cost"), 10)
    variants["band dpred"] = (lambda: cost_raw("dpred"), 10)
    variants["band dtarget"] = (lambda: cost_raw("dtarget"), 10)
    res = rounds(variants)

    rec = {"shape": [B, C, N, M], "bandwidth": w, "us": {k: {"median": round(med, 1), "min": round(lo, 1)} for k, (med, lo) in res.items()},
           "band_bytes_two_tensors": 8 * B * N * W, "dense_bytes_two_tensors": 8 * B * N * M,
           "steps_band": N + M - 1}
    rec["peak_bytes_band_loss_step"] = peak_of(lambda: loss_step(aligner_amd.soft_dtw_l1_banded_loss), preds + targets)
    print(f"[{B},{C},{N},{M}] bandwidth {w}: cost + gradient tensors {8 * B * N * W / 1e6:.1f} MB in band storage, "
          f"{8 * B * N * M / 1e6:.1f} MB dense")
    for name, (med, lo) in res.items():
        print("    %-24s median %10.1f us  min %10.1f us" % (name, med, lo))
    if dense:
        rec["peak_bytes_dense_loss_step"] = peak_of(lambda: loss_step(aligner_amd.soft_dtw_l1_loss), preds + targets)
        gate = {}
        for what in ("forward + E", "loss step"):
            a, b = res[f"dense {what} A"][0], res[f"dense {what} B"][0]
            spread, band = abs(a - b), res[f"band {what}"][0]
            gate[what] = {"dense_us": round(min(a, b), 1), "spread_us": round(spread, 1), "band_us": round(band, 1),
                          "met": bool(band <= min(a, b) + spread)}
            print(f"    gate, {what}: band {band:.1f} us against dense {min(a, b):.1f} us + spread {spread:.1f} us: "
                  f"{'met' if gate[what]['met'] else 'MISSED'}")
        rec["gate"] = gate
        print(f"    peak memory of a loss step: dense {rec['peak_bytes_dense_loss_step'] / 1e6:.1f} MB, "
              f"band {rec['peak_bytes_band_loss_step'] / 1e6:.1f} MB")
    else:
        print(f"    peak memory of a loss step: band {rec['peak_bytes_band_loss_step'] / 1e6:.1f} MB (the dense DP refuses N = {N})")
    fe, f = res["band forward + E"][0], res["band forward"][0]
    rec["ns_per_step_band"] = {"forward": round(f * 1e3 / (N + M - 1), 1), "backward": round((fe - f) * 1e3 / (N + M - 1), 1)}
    print(f"    band: {N + M - 1} steps, {rec['ns_per_step_band']['forward']} ns a step forward, "
          f"{rec['ns_per_step_band']['backward']} ns backward")
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("banddtw_time.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [(16, 80, 1000, 1000, 60, True), (64, 80, 1000, 1000, 60, True), (16, 80, 4000, 4000, 60, False)]
    if len(sys.argv) > 4:
        B, C, N, M = (int(a) for a in sys.argv[1:5])
        shapes = [(B, C, N, M, int(sys.argv[5]) if len(sys.argv) > 5 else 60, N <= 1024)]
    out = []
    for B, C, N, M, w, dense in shapes:
        out.append(one_shape(B, C, N, M, w, dev, dense))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "banddtw_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
