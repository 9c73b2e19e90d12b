#!/usr/bin/env python3
"""Time of the Euclidean cost calls on one MI355X beside their L1 counterparts, on the method of tools/l1cost_time.py:
device events around `it` calls, seven interleaved rounds after a warm-up, every C-ABI call on the next of enough cost /
grad_cost tables to exceed the 256 MiB on-package cache; the median, the minimum and the spread of the per-call time.

    (a) C ABI, dense          l1_cost, l2_cost squared, l2_cost root; l1_cost_backward, l2_cost_backward (both outputs)
    (p) the same L1 calls of another build of the library (--other-lib PATH, e.g. the parent commit's), interleaved
        with (a) in the same rounds: the guard for the re-templated L1 kernels (--other-first: before (a) in a round)
    (s) C ABI, band storage   (bandwidth <= 127) l1 / l2 cost_banded and their backward calls
    (b) torch.cdist(p=2)      forward; forward + backward of cdist ** 2, on [B,T,C] views of the same data
    (c) whole steps           soft_dtw_l2_loss; soft_dtw_loss(cdist ** 2 * scale); soft_dtw_l2_banded_loss

at [B,C,N,M] = [64,80,200,1000], [16,80,1000,1000] and the latter with bandwidth 60, scale 1/C, gamma 1, no penalty,
full lengths; then the peak memory of one soft_dtw_l2_banded_loss step at [16,80,4000,4000], bandwidth 60, which no
dense path can run.  Expectations (from instruction counts): squared forward within 15 % of l1_cost, squared backward
no slower than l1_cost_backward, (a) L1 within 15 % of (p).

    python tools/l2cost_time.py [--other-lib PATH [--other-first]] | tee profiles/l2cost_times.txt        Fails without a GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402
from l1cost_time import CACHE_BYTES, rounds  # noqa: E402


def other_library(path):
    """Another build of the library with the signatures of its L1 cost calls."""
    lib = ctypes.CDLL(path)
    for name in ("aligner_l1_cost_f32", "aligner_l1_cost_backward_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def one_shape(B, C, N, M, band, dev, other, other_first=False):
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.uniform(-1, 1, (B, C, N)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(-1, 1, (B, C, M)).astype(np.float32)).to(dev)
    scale, gamma = 1.0 / C, 1.0
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ncopies = int(CACHE_BYTES * 2.25 / (4.0 * B * N * M)) + 1
    costs = [torch.empty((B, N, M), device=dev) for _ in range(ncopies)]
    i, j = torch.arange(N, device=dev)[:, None], torch.arange(M, device=dev)[None, :]
    ok = torch.ones((N, M), dtype=torch.bool, device=dev) if band is None else (i - j).abs() <= band
    cells = int(ok.sum().item()) * B
    Gs = [torch.where(ok[None], torch.randn((B, N, M), device=dev), torch.full((), float("nan"), device=dev)) for _ in range(ncopies)]
    Gz = torch.nan_to_num(Gs[0], nan=0.0)
    dpred, dtarget = torch.empty_like(pred), torch.empty_like(target)
    cband = -1 if band is None else band
    turn = [0]
    P, T, none = pred.data_ptr(), target.data_ptr(), None

    def nxt(n):
        turn[0] = (turn[0] + 1) % n
        return turn[0]

    def l1_fwd(lb=lib):
        _lib.check(lb.aligner_l1_cost_f32(P, T, none, none, cband, scale, costs[nxt(ncopies)].data_ptr(), B, C, N, M, stream))

    def l2_fwd(squared):
        _lib.check(lib.aligner_l2_cost_f32(P, T, none, none, cband, scale, squared, costs[nxt(ncopies)].data_ptr(), B, C, N, M, stream))

    def bwd(fn):
        _lib.check(fn(Gs[nxt(ncopies)].data_ptr(), P, T, none, none, cband, scale, none, dpred.data_ptr(), dtarget.data_ptr(),
                      B, C, N, M, stream))

    variants = {
        "(a) l1_cost": (l1_fwd, 10),
        "(a) l2_cost squared": (lambda: l2_fwd(1), 10),
        "(a) l2_cost root": (lambda: l2_fwd(0), 10),
        "(a) l1_cost_backward": (lambda: bwd(lib.aligner_l1_cost_backward_f32), 10),
        "(a) l2_cost_backward": (lambda: bwd(lib.aligner_l2_cost_backward_f32), 10),
    }
    if other is not None:
        theirs = {"(p) l1_cost, other build": (lambda: l1_fwd(other), 10),
                  "(p) l1_cost_backward, other build": (lambda: bwd(other.aligner_l1_cost_backward_f32), 10)}
        variants = {**theirs, **variants} if other_first else {**variants, **theirs}      # (the order within a round)
    banded = band is not None and band <= 127
    if banded:
        W = 2 * band + 1
        nb = int(CACHE_BYTES * 2.25 / (4.0 * B * N * W)) + 1
        bcosts = [torch.empty((B, N, W), device=dev) for _ in range(nb)]
        bG = [aligner_amd.dense_to_band(Gs[0], band, fill=float("nan")) + 0 * k for k in range(nb)]

        def band_fwd(l2):
            out = bcosts[nxt(nb)].data_ptr()
            if l2:
                _lib.check(lib.aligner_l2_cost_banded_f32(P, T, none, none, band, scale, 1, out, B, C, N, M, stream))
            else:
                _lib.check(lib.aligner_l1_cost_banded_f32(P, T, none, none, band, scale, out, B, C, N, M, stream))

        def band_bwd(fn):
            _lib.check(fn(bG[nxt(nb)].data_ptr(), P, T, none, none, band, scale, none, dpred.data_ptr(), dtarget.data_ptr(),
                          B, C, N, M, stream))

        variants.update({
            "(s) l1_cost_banded": (lambda: band_fwd(False), 10),
            "(s) l2_cost_banded squared": (lambda: band_fwd(True), 10),
            "(s) l1_cost_banded_backward": (lambda: band_bwd(lib.aligner_l1_cost_banded_backward_f32), 10),
            "(s) l2_cost_banded_backward": (lambda: band_bwd(lib.aligner_l2_cost_banded_backward_f32), 10),
        })

    x = pred.transpose(1, 2).detach().requires_grad_()                 # [B,T,C] views of the same data
    y = target.transpose(1, 2).detach().requires_grad_()

    def cdist_fwd():
        with torch.no_grad():
            return torch.cdist(x, y, p=2)

    def cdist_both():
        x.grad = y.grad = None
        (torch.cdist(x, y, p=2) ** 2).backward(Gz)

    pg, tg = pred.clone().requires_grad_(), target.clone().requires_grad_()

    def step_fused():
        pg.grad = tg.grad = None
        aligner_amd.soft_dtw_l2_loss(pg, tg, None, None, gamma, 0.0, band, scale, reduction="sum").backward()

    def step_band():
        pg.grad = tg.grad = None
        aligner_amd.soft_dtw_l2_banded_loss(pg, tg, None, None, gamma, 0.0, band, scale, reduction="sum").backward()

    def step_cdist():
        x.grad = y.grad = None
        aligner_amd.soft_dtw_loss(torch.cdist(x, y, p=2) ** 2 * scale, None, None, gamma, 0.0, band, reduction="sum").backward()

    variants.update({"(b) cdist(p=2) forward": (cdist_fwd, 4), "(b) cdist(p=2) ** 2 forward + backward": (cdist_both, 4),
                     "(c) step, soft_dtw_l2_loss": (step_fused, 4), "(c) step, soft_dtw_loss(cdist ** 2)": (step_cdist, 4)})
    if banded:
        variants["(c) step, soft_dtw_l2_banded_loss"] = (step_band, 4)
    res = rounds(variants)
    # the two paths agree (fp32 against fp32) on the cells that exist
    cost = aligner_amd.l2_cost(pred, target, None, None, band, scale)
    ref = cdist_fwd() ** 2 * scale
    dc = ((cost - ref).abs()[:, ok].max() / ref.abs().max()).item()
    rec = {"shape": [B, C, N, M], "bandwidth": band, "existing_cells": cells, "max_rel_cost_difference_to_cdist": dc, "us": {}}
    print(f"[{B},{C},{N},{M}] bandwidth {band}: {cells} of {B * N * M} cells exist; l2_cost against cdist(p=2) ** 2: {dc:.2e} "
          "relative to the largest")
    for name, (med, lo, spread) in res.items():
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2), "spread": round(spread, 2)}
        print("    %-40s median %10.1f us  min %10.1f us  spread %8.1f us" % (name, med, lo, spread))
    m = lambda k: res[k][0]                                            # noqa: E731
    rec["l2_over_l1_forward"] = round(m("(a) l2_cost squared") / m("(a) l1_cost"), 3)
    rec["l2_over_l1_backward"] = round(m("(a) l2_cost_backward") / m("(a) l1_cost_backward"), 3)
    line = "    squared / L1: forward %.3f, backward %.3f" % (rec["l2_over_l1_forward"], rec["l2_over_l1_backward"])
    if other is not None:
        rec["l1_over_other_build_forward"] = round(m("(a) l1_cost") / m("(p) l1_cost, other build"), 3)
        rec["l1_over_other_build_backward"] = round(m("(a) l1_cost_backward") / m("(p) l1_cost_backward, other build"), 3)
        line += "; L1 of this build / other build: forward %.3f, backward %.3f" % (rec["l1_over_other_build_forward"],
                                                                                  rec["l1_over_other_build_backward"])
    print(line)
    return rec


def long_step_memory(dev, B=16, C=80, N=4000, M=4000, band=60):
    """Peak memory of one soft_dtw_l2_banded_loss step past the dense DP's 1024 rows."""
    rng = np.random.default_rng(1)
    pred = torch.from_numpy(rng.uniform(-1, 1, (B, C, N)).astype(np.float32)).to(dev).requires_grad_()
    target = torch.from_numpy(rng.uniform(-1, 1, (B, C, M)).astype(np.float32)).to(dev).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss = aligner_amd.soft_dtw_l2_banded_loss(pred, target, None, None, 1.0, 0.0, band, 1.0 / C, reduction="sum")
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    dense = 4.0 * B * N * M
    print(f"[{B},{C},{N},{M}] bandwidth {band}, one soft_dtw_l2_banded_loss step: loss {loss.item():.4f}, peak memory above the "
          f"inputs {peak / 2 ** 20:.1f} MiB (one dense [B,N,M] table would be {dense / 2 ** 20:.1f} MiB)")
    return {"shape": [B, C, N, M], "bandwidth": band, "peak_step_bytes": int(peak), "one_dense_table_bytes": int(dense)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("l2cost_time.py needs a GPU")
    dev = torch.device("cuda:0")
    args = sys.argv[1:]
    other = None
    if "--other-lib" in args:
        k = args.index("--other-lib")
        other = other_library(args[k + 1])
        del args[k:k + 2]
    other_first = "--other-first" in args
    out = []
    for shape in [(64, 80, 200, 1000, None), (16, 80, 1000, 1000, None), (16, 80, 1000, 1000, 60)]:
        out.append(one_shape(*shape, dev, other, other_first))
        torch.cuda.empty_cache()
    mem = long_step_memory(dev)
    print(json.dumps({"tool": "l2cost_time", "device": torch.cuda.get_device_name(0), "results": out, "long_step": mem}))


if __name__ == "__main__":
    main()
