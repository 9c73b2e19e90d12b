#!/usr/bin/env python3
"""Time of the gradient of gaussian_logp() on one MI355X against the same step composed in torch, in one process, on the
same device and inputs:

    gaussian_logp_backward(G, z, m, s)                        the raw vector-Jacobian product (three outputs)
    gaussian_logp_backward, dz only / dm and ds only           its two halves
    gaussian_logp(differentiable=True) + backward             forward + backward through autograd, cotangent G
    torch: the four-term formulation (fp32) + backward         the same step composed in torch, cotangent G

at [B,C,T_text,T_mel] = [64,80,200,1000] and [64,192,200,1000] (or B C Tx Ty from the command line).  Device events around
10 calls a round, 9 interleaved rounds (90 timed calls a variant) after 5 warm-up calls each, the median (and minimum) of
the per-call GPU time; then the raw call's algorithmic bytes (G read once per contraction direction, operands and
outputs) over its time as a share of 8 TB/s and its split-product flops as a share of 2.5 PF.  Raw output:
profiles/gausslogp_backward_times.txt (python tools/time_gausslogp_backward.py | tee profiles/gausslogp_backward_times.txt).
Fails without a GPU."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

HBM_BYTES_PER_S = 8e12
BF16_FLOPS = 2.5e15


def rounds(variants, n_rounds=9, it=10, warm=5):
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
    """Glow-TTS's formulation of the value tensor."""
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
    G = torch.randn(B, Tx, Ty, generator=g).to(dev)
    zr, mr, sr = (t.clone().requires_grad_() for t in (z, m, s))

    def step(value_of):
        for t in (zr, mr, sr):
            t.grad = None
        value_of(zr, mr, sr).backward(G)
        return zr.grad, mr.grad, sr.grad

    variants = {
        "gaussian_logp_backward (dz, dm, ds)": lambda: aligner_amd.gaussian_logp_backward(G, z, m, s),
        "gaussian_logp_backward (dz only)": lambda: aligner_amd.gaussian_logp_backward(G, z, m, s, need_mean=False, need_logstd=False),
        "gaussian_logp_backward (dm, ds only)": lambda: aligner_amd.gaussian_logp_backward(G, z, m, s, need_z=False),
        "autograd: gaussian_logp fwd + bwd": lambda: step(lambda a, b, c: aligner_amd.gaussian_logp(a, b, c, differentiable=True)),
        "torch four-term fwd + bwd (fp32)": lambda: step(torch_four_terms),
    }
    res = rounds(variants)
    # both steps against float64 autograd, relative to each gradient's largest element
    ref = [t.clone().double().requires_grad_() for t in (z, m, s)]
    torch_four_terms(*ref).backward(G.double())
    errs = {}
    for name, fn in (("HIP", variants["autograd: gaussian_logp fwd + bwd"]), ("torch fp32", variants["torch four-term fwd + bwd (fp32)"])):
        errs[name] = max(((a.double() - r.grad).abs().max() / r.grad.abs().max()).item() for a, r in zip(fn(), ref))
    print(f"[{B},{C},{Tx},{Ty}], GPU time per call; max |grad - float64| / max |grad|: HIP {errs['HIP']:.2e}, torch fp32 {errs['torch fp32']:.2e}")
    base = res["torch four-term fwd + bwd (fp32)"][0]
    flops = 3.0 * 4 * 2.0 * B * C * Tx * Ty
    nbytes = 4.0 * (2 * B * Tx * Ty + 2 * B * C * (2 * Tx + Ty))
    for name, (med, lo) in res.items():
        line = "    %-38s median %8.1f us  min %8.1f us" % (name, med, lo)
        if name.startswith("gaussian_logp_backward (dz, dm"):
            line += "  %5.1f MB: %4.1f %% of 8 TB/s;  %5.1f GF split products: %4.1f %% of 2.5 PF" % (
                nbytes / 1e6, 100.0 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S, flops / 1e9, 100.0 * flops / (med * 1e-6) / BF16_FLOPS)
        if name.startswith("autograd"):
            line += "  %.2fx the torch step" % (base / med)
        print(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_gausslogp_backward.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(a) for a in sys.argv[1:5])] if len(sys.argv) > 4 else [(64, 80, 200, 1000), (64, 192, 200, 1000)]
    for shape in shapes:
        one_shape(*shape, dev)


if __name__ == "__main__":
    main()
