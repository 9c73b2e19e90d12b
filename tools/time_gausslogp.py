#!/usr/bin/env python3
"""Time of gaussian_logp() on one MI355X against the four-term torch formulation a Glow-TTS / VITS step runs, in one
process, on the same device and inputs:

    gaussian_logp(fp32, contiguous)      gaussian_logp(fp32, pitched)      gaussian_logp(bf16)
    torch: exp, two matmuls, two reductions, three broadcast adds (fp32)

at [B,C,T_text,T_mel] = [64,80,200,1000] and [64,192,200,1000] (or B C Tx Ty from the command line).  Device events around
20 calls, interleaved rounds, the median (and minimum) of the per-call GPU time; then the algorithmic bytes over the time
as a share of 8 TB/s and the split-product flops over the time as a share of 2.5 PF.  Raw output: profiles/gausslogp_times.txt
(python tools/time_gausslogp.py | tee profiles/gausslogp_times.txt).  Fails without a GPU."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

HBM_BYTES_PER_S = 8e12
BF16_FLOPS = 2.5e15


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


def torch_four_terms(z, m, s):
    """Glow-TTS's formulation (its training step, under no_grad), fp32."""
    w = torch.exp(-2 * s)
    logp1 = torch.sum(-0.5 * math.log(2 * math.pi) - s, [1]).unsqueeze(-1)
    logp2 = torch.matmul(w.transpose(1, 2), -0.5 * (z ** 2))
    logp3 = torch.matmul((m * w).transpose(1, 2), z)
    logp4 = torch.sum(-0.5 * (m ** 2) * w, [1]).unsqueeze(-1)
    return logp1 + logp2 + logp3 + logp4


def one_shape(B, C, Tx, Ty, dev):
    g = torch.Generator().manual_seed(0)
    m = (1.5 * torch.randn(B, C, Tx, generator=g)).to(dev)
    s = torch.log(torch.rand(B, C, Tx, generator=g) + 0.5).to(dev)
    z = torch.randn(B, C, Ty, generator=g).to(dev)
    out32 = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev)
    out16 = torch.empty((B, Tx, Ty), dtype=torch.bfloat16, device=dev)
    outp = aligner_amd.softattn.pitched_logp(B, Tx, Ty, dev, torch.float32)
    variants = {
        "gaussian_logp(fp32, contiguous)": lambda: aligner_amd.gaussian_logp(z, m, s, out=out32),
        "gaussian_logp(fp32, pitched)": lambda: aligner_amd.gaussian_logp(z, m, s, out=outp),
        "gaussian_logp(bf16)": lambda: aligner_amd.gaussian_logp(z, m, s, out=out16),
        "torch four-term formulation (fp32)": lambda: torch_four_terms(z, m, s),
    }
    with torch.no_grad():
        res = rounds(variants)
        ref = torch_four_terms(z.double(), m.double(), s.double())
        err = (aligner_amd.gaussian_logp(z, m, s).double() - ref).abs().max().item()
        err_t = (torch_four_terms(z, m, s).double() - ref).abs().max().item()
    print(f"[{B},{C},{Tx},{Ty}], GPU time per call; max |fused - float64| {err:.2e}, max |torch fp32 - float64| {err_t:.2e}")
    base = res["torch four-term formulation (fp32)"][0]
    flops = 3.0 * 2.0 * B * Tx * Ty * 2 * C
    for name, (med, lo) in res.items():
        line = "    %-38s median %8.1f us  min %8.1f us" % (name, med, lo)
        if name.startswith("gaussian_logp"):
            esz = 2 if "bf16" in name else 4
            nbytes = 4.0 * B * C * (2 * Tx + Ty) + esz * B * Tx * Ty
            line += "  %5.1f MB: %4.1f %% of 8 TB/s;  %5.1f GF split products: %4.1f %% of 2.5 PF;  %.2fx the torch chain" % (
                nbytes / 1e6, 100.0 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S, flops / 1e9,
                100.0 * flops / (med * 1e-6) / BF16_FLOPS, base / med)
        print(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_gausslogp.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(a) for a in sys.argv[1:5])] if len(sys.argv) > 4 else [(64, 80, 200, 1000), (64, 192, 200, 1000)]
    for shape in shapes:
        one_shape(*shape, dev)


if __name__ == "__main__":
    main()
