#!/usr/bin/env python3
"""Time of gaussian_nll() / gaussian_nll_loss() on one MI355X against the path a caller composes from regulate() and
torch elementwise ops, in one process, on the same device and inputs:

    loss only                     gaussian_nll(z, m, s, dur, t_y)
    loss + gradient               gaussian_nll(..., want_grad=True)
    the same two, C ABI           aligner_gauss_nll_f32 on buffers allocated once (the kernels; the wrappers above are bound
                                  by the host at these sizes), every call on the next of enough copies of z and dz to
                                  exceed the 256 MiB on-package cache -- these are the rows the share of HBM peak is for --
                                  and, beside them, on one and the same buffers (served from that cache)
    rows per wave = 1, 2, 4       loss + gradient, C ABI, rotating buffers, the launch pinned ("gaussnll_rows")
    autograd forward + backward   gaussian_nll_loss(...).backward()          (z, mean, logstd require grad)
    composed forward + backward   regulate(mean), regulate(logstd), the elementwise chain, sum, .backward()

at [B,C,T_text,T_mel] = [64,80,200,1000] (Glow-TTS) and [64,192,200,1000] (VITS), or B C Tx Ty from the command line, with
the durations gaussian_align() finds on planted inputs.  Device events around 200 calls (5 ms and more a window), nine interleaved rounds after a warm-up,
the median (and minimum) of the per-call GPU time.  The algorithmic bytes are 4 B C T_mel per read of z and per write of
dz -- one read for the loss, a read and a write for loss + gradient, two reads and a write for forward + backward -- and
are stated over the time as a share of 8 TB/s.  Prints a table and, last, one JSON line:
python tools/gaussnll_time.py | tee profiles/gaussnll_times.txt.  Fails without a GPU."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

HBM_BYTES_PER_S = 8e12
CACHE_BYTES = 256 * 2 ** 20
HALF_LN_2PI = 0.5 * math.log(2 * math.pi)


def rounds(variants, n_rounds=9, it=200, warm=10):
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


def planted(B, C, Tx, Ty, seed=0):
    """Planted alignments with ragged lengths (durations >= 1 summing to t_y, z drawn from the owners' Gaussians)."""
    rng = np.random.default_rng(seed)
    t_x = rng.integers((3 * Tx) // 4, Tx + 1, B)
    t_y = rng.integers((3 * Ty) // 4, Ty + 1, B)
    t_x[0], t_y[0] = Tx, Ty
    m = 1.5 * rng.standard_normal((B, C, Tx))
    sig = rng.uniform(0.5, 1.5, (B, C, Tx))
    z = rng.standard_normal((B, C, Ty))
    for b in range(B):
        tx, ty = int(t_x[b]), int(t_y[b])
        dur = 1 + np.bincount(rng.integers(0, tx, ty - tx), minlength=tx)
        tok = np.repeat(np.arange(tx), dur)
        z[b, :, :ty] = m[b][:, tok] + sig[b][:, tok] * rng.standard_normal((C, ty))
    f = lambda a: torch.from_numpy(a.astype(np.float32))      # noqa: E731
    return f(z), f(m), f(np.log(sig)), torch.from_numpy(t_x.astype(np.int32)), torch.from_numpy(t_y.astype(np.int32))


def composed_loss(z, m, s, dur, t_y):
    Ty = z.shape[2]
    m_y, tok = aligner_amd.regulate(m, dur, Ty)
    s_y, _ = aligner_amd.regulate(s, dur, Ty)
    counts = ((tok >= 0) & (torch.arange(Ty, device=z.device)[None, :] < t_y[:, None])).unsqueeze(1)
    term = HALF_LN_2PI + s_y + 0.5 * (z - m_y) ** 2 * torch.exp(-2 * s_y)
    return (term * counts).sum() / (z.shape[1] * counts.sum()).clamp_min(1)


def one_shape(B, C, Tx, Ty, dev):
    z, m, s, t_x, t_y = (a.to(dev) for a in planted(B, C, Tx, Ty))
    dur = aligner_amd.gaussian_align(z, m, s, t_x, t_y, want_path=False).durations
    assert torch.equal(dur.sum(1).to(torch.int32), t_y)
    zg, mg, sg = (a.clone().requires_grad_() for a in (z, m, s))

    def fused_fb():
        zg.grad = mg.grad = sg.grad = None
        aligner_amd.gaussian_nll_loss(zg, mg, sg, dur, t_y).backward()

    def composed_fb():
        zg.grad = mg.grad = sg.grad = None
        composed_loss(zg, mg, sg, dur, t_y).backward()

    # the C ABI on buffers allocated once: the two launches without torch's allocations and the wrapper's checks, so that
    # the host enqueues faster than the GPU runs and the events see the kernels
    from aligner_amd import _lib
    lib = _lib.load()
    nll, count = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    dm, ds = torch.empty_like(m), torch.empty_like(s)
    ws = torch.empty(lib.aligner_gauss_nll_workspace_bytes(B, C, Tx), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ncopies = int(CACHE_BYTES * 2.25 / (4.0 * B * C * Ty)) + 1          # z copies alone exceed the cache twice over
    zs = [z.clone() for _ in range(ncopies)]
    dzs = [torch.empty_like(z) for _ in range(ncopies)]
    turn = [0]

    def raw(grad, rotate=True, rows=0):
        i = 0
        if rotate:
            i = turn[0] = (turn[0] + 1) % ncopies
        if rows:
            lib.aligner_debug_set_option(b"gaussnll_rows", rows)
        g = (dzs[i].data_ptr(), dm.data_ptr(), ds.data_ptr()) if grad else (None, None, None)
        _lib.check(lib.aligner_gauss_nll_f32(zs[i].data_ptr(), m.data_ptr(), s.data_ptr(), dur.data_ptr(), t_y.data_ptr(), None,
                                             nll.data_ptr(), count.data_ptr(), *g, ws.data_ptr(), ws.numel(), B, C, Tx, Ty, stream))
        if rows:
            lib.aligner_debug_set_option(b"gaussnll_rows", 0)          # (read at the launch: the host's side of the call)

    variants = {
        "loss only": lambda: aligner_amd.gaussian_nll(z, m, s, dur, t_y),
        "loss + gradient": lambda: aligner_amd.gaussian_nll(z, m, s, dur, t_y, want_grad=True),
        "loss only, C ABI": lambda: raw(False),
        "loss + gradient, C ABI": lambda: raw(True),
        "loss only, C ABI, same buffers": lambda: raw(False, rotate=False),
        "loss + gradient, C ABI, same buffers": lambda: raw(True, rotate=False),
        "loss + gradient, C ABI, rows per wave = 1": lambda: raw(True, rows=1),
        "loss + gradient, C ABI, rows per wave = 2": lambda: raw(True, rows=2),
        "loss + gradient, C ABI, rows per wave = 4": lambda: raw(True, rows=4),
        "autograd forward + backward": fused_fb,
        "composed forward + backward": composed_fb,
    }
    res = rounds(variants)
    # the two paths agree (fp32 against fp32: reordered sums)
    fused_fb()
    gz, gm, gs, lf = zg.grad.clone(), mg.grad.clone(), sg.grad.clone(), aligner_amd.gaussian_nll_loss(z, m, s, dur, t_y).item()
    composed_fb()
    diff = max(((a - b).abs().max() / b.abs().max()).item() for a, b in ((gz, zg.grad), (gm, mg.grad), (gs, sg.grad)))
    lc = composed_loss(z, m, s, dur, t_y).item()
    zbytes = 4.0 * B * C * Ty
    passes = {name: (1 if name.startswith("loss only") else 2) for name in variants if name.startswith("loss")}
    passes["autograd forward + backward"] = 3
    rec = {"shape": [B, C, Tx, Ty], "loss_fused": lf, "loss_composed": lc, "max_rel_grad_difference": diff, "us": {}, "hbm_share": {}}
    print(f"[{B},{C},{Tx},{Ty}]: loss fused {lf:.6f}, composed {lc:.6f}; largest gradient difference / largest gradient {diff:.2e}")
    base = res["composed forward + backward"][0]
    for name, (med, lo) in res.items():
        line = "    %-42s median %8.1f us  min %8.1f us" % (name, med, lo)
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2)}
        if name in passes:
            share = passes[name] * zbytes / (med * 1e-6) / HBM_BYTES_PER_S
            rec["hbm_share"][name] = round(share, 4)
            line += "  %6.1f MB of z / dz: %4.1f %% of 8 TB/s" % (passes[name] * zbytes / 1e6, 100.0 * share)
        print(line)
    rec["composed_over_fused"] = round(base / res["autograd forward + backward"][0], 3)
    print("    composed / fused (forward + backward): %.2fx" % rec["composed_over_fused"])
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("gaussnll_time.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(a) for a in sys.argv[1:5])] if len(sys.argv) > 4 else [(64, 80, 200, 1000), (64, 192, 200, 1000)]
    out = [one_shape(*shape, dev) for shape in shapes]
    print(json.dumps({"tool": "gaussnll_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
