#!/usr/bin/env python3
"""Time of l1_cost() / l1_cost_backward() / soft_dtw_l1_loss() on one MI355X against torch.cdist(p=1), in one process, on
the same device and data:

    (a) l1_cost, C ABI                 aligner_l1_cost_f32 on buffers allocated once, every call on the next of enough
        l1_cost_backward, C ABI        cost / grad_cost tables to exceed the 256 MiB on-package cache; both outputs, and
                                       each alone (one kernel each)
    (b) cdist forward                  torch.cdist(p=1) on [B,T,C] views of the same pred / target, without a graph
        cdist forward + backward       ... with both inputs requiring a gradient, .backward(G); also on contiguous
                                       [B,T,C] copies, the layout a frame-major caller holds
    (c) step, soft_dtw_l1_loss         soft_dtw_l1_loss(pred, target, ...).backward()
        step, soft_dtw_loss(cdist)     soft_dtw_loss(torch.cdist(...) * scale, ...).backward()

at [B,C,N,M] = [64,80,200,1000], [16,80,1000,1000] and [16,80,1000,1000] with bandwidth 60 (or B C N M [bandwidth] from
the command line), scale 1/C, gamma 1, no penalty, full lengths.  Device events around `it` calls, seven interleaved
rounds after a warm-up; the median, the minimum and the spread (max - min) of the per-call GPU time.

Each kernel's floor on its own work: bytes at the 6.29 TB/s a copy reaches (forward: the whole table written, since every
cell is; backward: grad_cost read on the existing cells; the [B,C,T] operands on top), and vector instructions at one
per lane and clock on 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 / s (the 157.3 TFLOPS fp32 vector peak counts a
fused multiply-add as two; nothing here is one): forward 2 per existing cell and channel (a subtraction, an add of the
magnitude), backward 5 per existing cell, channel and output (two compares, two selects, an add).

Prints a table and, last, one JSON line: python tools/l1cost_time.py | tee profiles/l1cost_times.txt.  Fails without a GPU."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
CACHE_BYTES = 256 * 2 ** 20


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
    return {k: (sorted(v)[len(v) // 2], min(v), max(v) - min(v)) for k, v in times.items()}


def one_shape(B, C, N, M, band, dev):
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
    # grad_cost: random on the cells, NaN elsewhere (nothing may read it there)
    Gs = [torch.where(ok[None], torch.randn((B, N, M), device=dev), torch.full((), float("nan"), device=dev)) for _ in range(ncopies)]
    Gz = torch.nan_to_num(Gs[0], nan=0.0)                              # what the torch path gets: it multiplies
    dpred, dtarget = torch.empty_like(pred), torch.empty_like(target)
    cband = -1 if band is None else band
    turn = [0]

    def fwd():
        k = turn[0] = (turn[0] + 1) % ncopies
        _lib.check(lib.aligner_l1_cost_f32(pred.data_ptr(), target.data_ptr(), None, None, cband, scale, costs[k].data_ptr(),
                                           B, C, N, M, stream))

    def bwd(want_pred=True, want_target=True):
        k = turn[0] = (turn[0] + 1) % ncopies
        _lib.check(lib.aligner_l1_cost_backward_f32(Gs[k].data_ptr(), pred.data_ptr(), target.data_ptr(), None, None, cband, scale,
                                                    None, dpred.data_ptr() if want_pred else None,
                                                    dtarget.data_ptr() if want_target else None, B, C, N, M, stream))

    def both():
        fwd()
        bwd()

    x = pred.transpose(1, 2).detach().requires_grad_()                 # [B,T,C] views of the same data
    y = target.transpose(1, 2).detach().requires_grad_()

    def cdist_fwd():
        with torch.no_grad():
            return torch.cdist(x, y, p=1)

    def cdist_both():
        x.grad = y.grad = None
        torch.cdist(x, y, p=1).backward(Gz)

    xc = pred.transpose(1, 2).contiguous().requires_grad_()           # [B,T,C] copies: what a frame-major caller holds
    yc = target.transpose(1, 2).contiguous().requires_grad_()

    def cdist_both_contiguous():
        xc.grad = yc.grad = None
        torch.cdist(xc, yc, p=1).backward(Gz)

    pg, tg = pred.clone().requires_grad_(), target.clone().requires_grad_()

    def step_fused():
        pg.grad = tg.grad = None
        aligner_amd.soft_dtw_l1_loss(pg, tg, None, None, gamma, 0.0, band, scale, reduction="sum").backward()

    def step_cdist():
        x.grad = y.grad = None
        aligner_amd.soft_dtw_loss(torch.cdist(x, y, p=1) * scale, None, None, gamma, 0.0, band, reduction="sum").backward()

    variants = {
        "(a) l1_cost, C ABI": (fwd, 10),
        "(a) l1_cost_backward, C ABI": (bwd, 10),
        "(a)   ... dpred only": (lambda: bwd(True, False), 10),
        "(a)   ... dtarget only": (lambda: bwd(False, True), 10),
        "(a) forward + backward": (both, 10),
        "(b) cdist forward": (cdist_fwd, 4),
        "(b) cdist forward + backward": (cdist_both, 4),
        "(b)   ... on contiguous [B,T,C]": (cdist_both_contiguous, 4),
        "(c) step, soft_dtw_l1_loss": (step_fused, 4),
        "(c) step, soft_dtw_loss(cdist)": (step_cdist, 4),
    }
    res = rounds(variants)
    # the two paths agree (fp32 against fp32) on the cells that exist
    cost = aligner_amd.l1_cost(pred, target, None, None, band, scale)
    ref = cdist_fwd() * scale
    dc = ((cost - ref).abs()[:, ok].max() / ref.abs().max()).item()
    dp, dt = aligner_amd.l1_cost_backward(Gs[0], pred, target, None, None, band, scale)
    x.grad = y.grad = None
    (torch.cdist(x, y, p=1) * scale).backward(Gz)
    dg = max((dp - x.grad.transpose(1, 2)).abs().max().item(), (dt - y.grad.transpose(1, 2)).abs().max().item()) / x.grad.abs().max().item()
    operand_bytes = 4.0 * B * C * (N + M)
    floors = {
        "(a) l1_cost, C ABI": ((4.0 * B * N * M + operand_bytes) / COPY_BYTES_PER_S * 1e6, 2.0 * cells * C / VALU_LANE_OPS_PER_S * 1e6),
        "(a) l1_cost_backward, C ABI": ((4.0 * cells + 2 * operand_bytes) / COPY_BYTES_PER_S * 1e6,
                                        10.0 * cells * C / VALU_LANE_OPS_PER_S * 1e6),
    }
    rec = {"shape": [B, C, N, M], "bandwidth": band, "existing_cells": cells, "max_rel_cost_difference": dc,
           "max_rel_gradient_difference": dg, "us": {}}
    print(f"[{B},{C},{N},{M}] bandwidth {band}: {cells} of {B * N * M} cells exist; fused against cdist: cost {dc:.2e}, "
          f"gradients {dg:.2e} relative to the largest")
    for name, (med, lo, spread) in res.items():
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2), "spread": round(spread, 2)}
        line = "    %-34s median %10.1f us  min %10.1f us  spread %8.1f us" % (name, med, lo, spread)
        if name in floors:
            fb, fv = floors[name]
            rec["us"][name].update(bytes_floor_us=round(fb, 2), valu_floor_us=round(fv, 2))
            line += "   bytes floor %7.1f us (%4.1f %%), vector-instruction floor %7.1f us (%4.1f %%)" % (fb, 100 * fb / med, fv, 100 * fv / med)
        print(line)
    a = res["(a) forward + backward"]
    b_ = min(res["(b) cdist forward + backward"], res["(b)   ... on contiguous [B,T,C]"])      # the faster yardstick
    rec["cdist_over_fused_forward"] = round(res["(b) cdist forward"][0] / res["(a) l1_cost, C ABI"][0], 2)
    rec["cdist_over_fused_forward_backward"] = round(b_[0] / a[0], 2)
    rec["step_cdist_over_fused"] = round(res["(c) step, soft_dtw_loss(cdist)"][0] / res["(c) step, soft_dtw_l1_loss"][0], 2)
    rec["forward_backward_gap_us"] = round(b_[0] - a[0], 2)
    rec["forward_backward_spread_us"] = round(max(a[2], b_[2]), 2)
    print("    cdist / fused: forward %.2fx, forward + backward %.2fx (gap %.1f us, larger spread %.1f us), whole step %.2fx"
          % (rec["cdist_over_fused_forward"], rec["cdist_over_fused_forward_backward"], rec["forward_backward_gap_us"],
             rec["forward_backward_spread_us"], rec["step_cdist_over_fused"]))
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("l1cost_time.py needs a GPU")
    dev = torch.device("cuda:0")
    if len(sys.argv) > 4:
        shapes = [(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else None)]
    else:
        shapes = [(64, 80, 200, 1000, None), (16, 80, 1000, 1000, None), (16, 80, 1000, 1000, 60)]
    out = []
    for shape in shapes:
        out.append(one_shape(*shape, dev))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "l1cost_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
