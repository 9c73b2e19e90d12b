#!/usr/bin/env python3
"""Time of the cost kinds along a path on one MI355X, on the method of tools/l1cost_time.py: device events around `it`
calls, seven interleaved rounds after a warm-up; the median, the minimum and the spread of the per-call time.  The
operands are small (pred, target, a path of K <= N + M - 1 pairs): they live in the caches, as they do in a training
step, where the DP that made the path has just read them.

    (a) path_cost                     per kind, pair costs and total
    (b) path_cost_backward            per kind, both outputs, unit weights
    (c) the composed path             path_to_dense + l1_cost_backward / l2_cost_backward: what the parent commit offers
                                      for the same gradient; dense shapes only, no root kind, no band storage
    (d) whole steps                   dtw_l1_loss forward + backward; soft_dtw_l1_loss (dense) or soft_dtw_l1_banded_loss
                                      (band storage) at the same shape

at [B,C,N,M] = [64,80,200,1000] (no band, dense), [16,80,1000,1000] with bandwidth 60 in band storage and, dense, with
bandwidth 128 (the losses dispatch a band of at most 127 to band storage, so 128 is the narrowest band the dense step
has), and [16,80,4000,4000] with bandwidth 60 in band storage; scale 1/C, warp penalty 0.05, full lengths.  Then the
peak memory of one dtw_l1_loss step against the composed path's.

    python tools/pathcost_time.py | tee profiles/pathcost_times.txt        Fails without a GPU."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from l1cost_time import rounds  # noqa: E402

PENALTY = 0.05


def _peak(dev, fn, *leaves):
    """Peak memory of fn() above what is allocated before it, the leaves' old gradients freed first (fn frees them
    itself: counted in `before`, they would be subtracted from the peak)."""
    for leaf in leaves:
        leaf.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - before)


def one_shape(B, C, N, M, band, storage, dev):
    """storage: "dense" (dtw_path on a [B,N,M] table, whatever the band) or "band" (band storage, bandwidth <= 127)."""
    rng = np.random.default_rng(0)
    # a slowly varying signal and a warped copy of it plus noise: a path with runs, as real features give
    base = np.cumsum(rng.uniform(-1, 1, (B, C, max(N, M) + 64)), axis=2) * 0.1
    pred = torch.from_numpy(base[:, :, :N].astype(np.float32)).to(dev)
    t = np.linspace(0.0, 1.0, M)
    warp = np.clip(np.round(t * (N - 1) + min(0.03 * N, 40.0) * np.sin(2 * np.pi * t)), 0, N - 1).astype(int)      # (inside any band >= 40)
    target = torch.from_numpy((base[:, :, warp] + rng.normal(0, 0.05, (B, C, M))).astype(np.float32)).to(dev)
    scale = 1.0 / C
    dense = storage == "dense"
    # (dense storage is dispatched for a band of None or past 127: the dense DP's band here is the same cells or more)
    w = band if not dense else (None if band is None else max(band, 128))
    r = aligner_amd.dtw_path_l1(pred, target, None, None, PENALTY, w, scale)
    K = r.length.cpu().numpy()
    assert (K > 0).all(), "an utterance has no alignment"
    runs = aligner_amd.path_runs(r.path, r.length, N, M)
    variants = {}
    for kind in ("l1", "l2", "l2root"):
        variants[f"(a) path_cost {kind}"] = (lambda kind=kind: aligner_amd.path_cost(pred, target, r.path, r.length, None, None, kind, scale), 10)
    for kind in ("l1", "l2", "l2root"):
        variants[f"(b) path_cost_backward {kind}"] = (
            lambda kind=kind: aligner_amd.path_cost_backward(None, pred, target, r.path, r.length, None, None, kind, scale), 10)
    if dense:
        E = aligner_amd.path_to_dense(r.path, r.length, N, M)
        variants["(c) path_to_dense"] = (lambda: aligner_amd.path_to_dense(r.path, r.length, N, M), 4)
        variants["(c) l1_cost_backward on the dense path"] = (lambda: aligner_amd.l1_cost_backward(E, pred, target, None, None, None, scale), 4)
        variants["(c) l2_cost_backward on the dense path"] = (lambda: aligner_amd.l2_cost_backward(E, pred, target, None, None, None, scale), 4)
    pg, tg = pred.clone().requires_grad_(), target.clone().requires_grad_()

    def step_hard():
        pg.grad = tg.grad = None
        aligner_amd.dtw_l1_loss(pg, tg, None, None, PENALTY, w, scale, reduction="sum").backward()

    def step_soft():
        pg.grad = tg.grad = None
        if dense:
            aligner_amd.soft_dtw_l1_loss(pg, tg, None, None, 1.0, PENALTY, w, scale, reduction="sum").backward()
        else:
            aligner_amd.soft_dtw_l1_banded_loss(pg, tg, None, None, 1.0, PENALTY, w, scale, reduction="sum").backward()

    def step_composed():
        pg.grad = tg.grad = None
        rr = aligner_amd.dtw_path_l1(pg, tg, None, None, PENALTY, w, scale)
        aligner_amd.l1_cost_backward(aligner_amd.path_to_dense(rr.path, rr.length, N, M), pg, tg, None, None, None, scale)

    variants["(d) step, dtw_l1_loss"] = (step_hard, 4)
    if dense and N <= 1024:
        variants["(d) step, soft_dtw_l1_loss"] = (step_soft, 4)
        variants["(d) step, dtw_path_l1 + path_to_dense + l1_cost_backward"] = (step_composed, 4)
    elif not dense:
        variants["(d) step, soft_dtw_l1_banded_loss"] = (step_soft, 4)
    res = rounds(variants)
    rec = {"shape": [B, C, N, M], "bandwidth": band, "storage": storage, "path_length": [int(K.min()), int(K.max())],
           "longest_run": [int(runs.row_count.max()), int(runs.col_count.max())], "us": {}}
    print(f"[{B},{C},{N},{M}] bandwidth {band}, {storage} storage: path lengths {K.min()} .. {K.max()}, longest row / column run "
          f"{rec['longest_run'][0]} / {rec['longest_run'][1]}")
    for name, (med, lo, spread) in res.items():
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2), "spread": round(spread, 2)}
        print("    %-60s median %10.1f us  min %10.1f us  spread %8.1f us" % (name, med, lo, spread))
    rec["peak_step_bytes"] = {"dtw_l1_loss": _peak(dev, step_hard, pg, tg), "soft loss": _peak(dev, step_soft, pg, tg)}
    if dense and N <= 1024:
        rec["peak_step_bytes"]["composed"] = _peak(dev, step_composed, pg, tg)
    print("    peak memory of one step above the inputs: " + ", ".join(f"{k} {v / 2 ** 20:.1f} MiB" for k, v in rec["peak_step_bytes"].items())
          + f" (one dense [B,N,M] table: {4.0 * B * N * M / 2 ** 20:.1f} MiB)")
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("pathcost_time.py needs a GPU")
    dev = torch.device("cuda:0")
    out = []
    for shape in [(64, 80, 200, 1000, None, "dense"), (16, 80, 1000, 1000, 60, "dense"), (16, 80, 1000, 1000, 60, "band"),
                  (16, 80, 4000, 4000, 60, "band")]:
        out.append(one_shape(*shape, dev))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "pathcost_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
