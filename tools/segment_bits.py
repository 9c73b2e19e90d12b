#!/usr/bin/env python3
"""The bits of the kernels that work on the duration segments, for comparing two builds of the library: one sha256 per
output of segment_reduce (sum, mean), regulate (out, tok) and gaussian_nll (loss only; with gradient: nll, count, dz, dm,
ds) at five shapes [B,C,T_text,T_mel], from fixed seeds, on the aligner's own durations and on a set with zeros,
negatives and a sum that misses T_mel.  The kernels have one summation order, so two builds that perform the same
operations print the same listing:

    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/segment_bits.py > a.txt
    python tools/segment_bits.py > b.txt && cmp a.txt b.txt

Fails without a GPU."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402

SHAPES = [(64, 512, 200, 1000), (64, 80, 200, 1000), (64, 192, 200, 1000), (2, 9, 600, 1201), (2100, 33, 5, 19)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def durations(kind, B, Tx, Ty, rng, dev):
    """(durations [B,Tx] int32, t_y [B] int32) on the device."""
    t_y = rng.integers(max(Ty // 2, min(Tx, Ty)), Ty + 1, size=B)
    t_y[0] = Ty
    if kind == "align":
        t_x = np.array([rng.integers(max(1, min(Tx, t) // 2), min(Tx, t) + 1) for t in t_y])
        t_x[0] = min(Tx, Ty)
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        val = torch.randn((B, Tx, Ty), generator=g).to(dev)
        dur = aligner_amd.align(val, torch.from_numpy(t_x.astype(np.int32)).to(dev),
                                torch.from_numpy(t_y.astype(np.int32)).to(dev), want_path=False).durations.to(torch.int32)
    else:
        d = rng.integers(-3, max(2, 2 * Ty // Tx + 2), size=(B, Tx))
        d[rng.random((B, Tx)) < 0.3] = 0
        dur = torch.from_numpy(d.astype(np.int32)).to(dev)
    return dur, torch.from_numpy(t_y.astype(np.int32)).to(dev)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("segment_bits.py needs a GPU")
    dev = torch.device("cuda:0")
    for i, (B, C, Tx, Ty) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(100 + i)
        frames = (torch.randn(B, C, Ty, generator=g) * 3.0 + 0.5).to(dev)
        mean = torch.randn(B, C, Tx, generator=g).to(dev)
        logstd = (torch.rand(B, C, Tx, generator=g) - 0.5).to(dev)
        scale = (torch.rand(B, generator=g) + 0.25).to(dev)
        for kind in ("align", "zeros_neg"):
            dur, t_y = durations(kind, B, Tx, Ty, np.random.default_rng(1000 * i + len(kind)), dev)
            out = {"durations": dur,
                   "segment_reduce sum": aligner_amd.segment_reduce(frames, dur),
                   "segment_reduce mean": aligner_amd.segment_reduce(frames, dur, mean=True)}
            out["regulate out"], out["regulate tok"] = aligner_amd.regulate(mean, dur, Ty)
            out["gaussian_nll loss only nll"], out["gaussian_nll loss only count"] = aligner_amd.gaussian_nll(frames, mean, logstd, dur, t_y)
            grads = aligner_amd.gaussian_nll(frames, mean, logstd, dur, t_y, want_grad=True, scale=scale)
            out.update(zip(("gaussian_nll nll", "gaussian_nll count", "gaussian_nll dz", "gaussian_nll dm", "gaussian_nll ds"), grads))
            torch.cuda.synchronize()
            for name, t in out.items():
                print("[%d,%d,%d,%d] %-9s %-28s %s" % (B, C, Tx, Ty, kind, name, sha(t)))


if __name__ == "__main__":
    main()
