#!/usr/bin/env python3
"""Time of soft_dtw() on one MI355X, in one process, on the same device and inputs:

    forward, C ABI                aligner_soft_dtw_f32 without a gradient buffer, on buffers allocated once, every call on
                                  the next of enough copies of the cost to exceed the 256 MiB on-package cache
    forward + E, C ABI            ... with the gradient buffer (the forward kernel leaves R in it, the backward one E)
    forward + E, autograd         soft_dtw_loss(cost, ...).backward()
    composed forward / + backward Soft-DTW as a caller composes it in torch: the cost skewed once so that an anti-diagonal
                                  is a column, then N + M - 1 steps of a stacked logsumexp over the three shifted
                                  predecessors; .backward() through it
    forward_sum with gradient     aligner_amd.forward_sum at [64,200,1000] only: the nearest log-domain DP over the same bytes

at [B,N,M] = [64,200,1000], [16,1000,1000] and [16,1000,1000] with bandwidth 60 (or B N M [bandwidth] from the command
line), costs mean|x - y| over 8 channels, gamma 1, no penalty, full lengths.  Device events around `it` calls, seven
interleaved rounds after a warm-up, the median (and minimum) of the per-call GPU time; the composed path runs 2 calls a
round.  The copy ceiling is one read and one write of the tensor at the 6.29 TB/s a copy reaches.  Prints a table and,
last, one JSON line: python tools/softdtw_time.py | tee profiles/softdtw_times.txt.  Fails without a GPU."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
CACHE_BYTES = 256 * 2 ** 20
BIG = 1e30


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


def composed(cost, gamma, band):
    """value [B] by the anti-diagonal loop; differentiable in cost."""
    B, N, M = cost.shape
    dev = cost.device
    i = torch.arange(N, device=dev)[:, None]
    s = torch.arange(N + M - 1, device=dev)[None, :]
    j = s - i
    ok = (j >= 0) & (j < M)
    if band is not None:
        ok &= (i - j).abs() <= band
    sk = torch.where(ok[None], cost.gather(2, j.clamp(0, M - 1)[None].expand(B, N, N + M - 1)), cost.new_tensor(BIG))
    big = cost.new_full((B, 1), BIG)
    p2 = cost.new_full((B, N), BIG)                     # diagonal s - 2, diagonal s - 1
    p1 = cost.new_full((B, N), BIG)
    first = torch.cat([cost.new_zeros((B, 1)), cost.new_full((B, N - 1), BIG)], 1)
    for step in range(N + M - 1):
        diag = torch.cat([big, p2[:, :-1]], 1) if step else first
        up = torch.cat([big, p1[:, :-1]], 1)
        sm = -gamma * torch.logsumexp(torch.stack([diag, up, p1]) * (-1.0 / gamma), dim=0)
        p2, p1 = p1, (sk[:, :, step] + sm).clamp_max(BIG)
    return p1[:, N - 1]


def one_shape(B, N, M, band, dev):
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, (B, N, 1, 8)).astype(np.float32)
    y = rng.uniform(0, 1, (B, 1, M, 8)).astype(np.float32)
    cost = torch.from_numpy(np.abs(x - y).mean(3)).to(dev)
    gamma = 1.0
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ncopies = int(CACHE_BYTES * 2.25 / (4.0 * B * N * M)) + 1
    costs = [cost.clone() for _ in range(ncopies)]
    grads = [torch.empty_like(cost) for _ in range(ncopies)]
    value = torch.empty(B, device=dev)
    ws = torch.empty(max(lib.aligner_soft_dtw_workspace_bytes(B, N, M, 1), 1), dtype=torch.uint8, device=dev)
    turn = [0]

    def raw(grad):
        k = turn[0] = (turn[0] + 1) % ncopies
        _lib.check(lib.aligner_soft_dtw_f32(costs[k].data_ptr(), None, None, gamma, 0.0, -1 if band is None else band,
                                            value.data_ptr(), grads[k].data_ptr() if grad else None, ws.data_ptr(), ws.numel(),
                                            B, N, M, stream))

    cg = cost.clone().requires_grad_()

    def fused():
        cg.grad = None
        aligner_amd.soft_dtw_loss(cg, None, None, gamma, 0.0, band, reduction="sum").backward()

    def torch_path(grad):
        if not grad:
            with torch.no_grad():
                return composed(cost, gamma, band)
        cg.grad = None
        composed(cg, gamma, band).sum().backward()

    variants = {
        "forward, C ABI": (lambda: raw(False), 20),
        "forward + E, C ABI": (lambda: raw(True), 20),
        "forward + E, autograd": (fused, 20),
        "composed forward": (lambda: torch_path(False), 2),
        "composed forward + backward": (lambda: torch_path(True), 2),
    }
    if (B, N, M) == (64, 200, 1000) and band is None:
        logp = torch.log_softmax(torch.randn(B, N, M, device=dev), dim=1)
        tx = torch.full((B,), N, dtype=torch.int32, device=dev)
        ty = torch.full((B,), M, dtype=torch.int32, device=dev)
        variants["forward_sum with gradient"] = (lambda: aligner_amd.forward_sum(logp, tx, ty, want_grad=True), 20)
    res = rounds(variants)
    # the two paths agree (fp32 against fp32)
    v_f, E_f = aligner_amd.soft_dtw(cost, None, None, gamma, 0.0, band)
    torch_path(True)
    v_c = composed(cost, gamma, band)
    dv = ((v_f - v_c).abs().max() / v_c.abs().max()).item()
    dE = (E_f - cg.grad).abs().max().item()
    ceiling = 8.0 * B * N * M / COPY_BYTES_PER_S * 1e6
    rec = {"shape": [B, N, M], "bandwidth": band, "max_rel_value_difference": dv, "max_abs_E_difference": dE,
           "copy_ceiling_us": round(ceiling, 2), "us": {}}
    print(f"[{B},{N},{M}] bandwidth {band}: fused against composed: value {dv:.2e} relative, E {dE:.2e} absolute; "
          f"one read + one write of the tensor at 6.29 TB/s: {ceiling:.1f} us")
    for name, (med, lo) in res.items():
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2)}
        print("    %-30s median %10.1f us  min %10.1f us" % (name, med, lo))
    rec["composed_over_fused_forward"] = round(res["composed forward"][0] / res["forward, C ABI"][0], 2)
    rec["composed_over_fused_forward_backward"] = round(res["composed forward + backward"][0] / res["forward + E, autograd"][0], 2)
    print("    composed / fused: forward %.1fx, forward + gradient %.1fx"
          % (rec["composed_over_fused_forward"], rec["composed_over_fused_forward_backward"]))
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("softdtw_time.py needs a GPU")
    dev = torch.device("cuda:0")
    if len(sys.argv) > 3:
        shapes = [(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else None)]
    else:
        shapes = [(64, 200, 1000, None), (16, 1000, 1000, None), (16, 1000, 1000, 60)]
    out = [one_shape(*shape, dev) for shape in shapes]
    print(json.dumps({"tool": "softdtw_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
