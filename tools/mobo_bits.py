#!/usr/bin/env python3
"""The bits of the boundary search and of its gradient, for comparing two builds of the library: one sha256 per output
-- boundaries, durations, map_score (the MAP sequence alone; the same through the full kernel, `mobo_full_chain`),
log_alpha, gamma (the sum-product chain alone, want_map=False), all five (both chains) and grad_energies (cotangents on
log_alpha and gamma) -- from fixed seeds, on ragged lengths, with fp32 and bf16 energies.  The shapes [B,Tx,Ty,D] take
every chain kernel of the launch plan on 256 CUs: the split form with H = 4, 2, 1 lanes per position, each with and
without a helper wave, and the several-positions kernel.  The kernels have one summation order, so two builds that
perform the same operations print the same listing:

    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/mobo_bits.py > a.txt
    python tools/mobo_bits.py > b.txt && cmp a.txt b.txt

Fails without a GPU."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib, mobo  # noqa: E402

SHAPES = [(4, 12, 40, 8),        # H = 4, no helper
          (3, 40, 300, 16),      # H = 4, helper
          (1, 4, 100, 60),       # H = 2, no helper
          (5, 33, 700, 40),      # H = 2, helper
          (2, 30, 1100, 64),     # H = 2, helper, 128 positions a segment
          (1, 4, 300, 200),      # H = 1, no helper
          (3, 12, 600, 100),     # H = 1, helper
          (2, 8, 1500, 800),     # several positions per thread, one segment
          (1, 6, 2600, 1300),
          (300, 4, 20, 6),       # more utterances than CUs
          (8, 500, 4000, 32)]    # bench.py --config c5


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("mobo_bits.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for n, (B, Tx, Ty, D) in enumerate(SHAPES):
        rng = np.random.default_rng(500 + n)
        tx = np.array([Tx] + [int(rng.integers(max(1, -(-Ty // (2 * D))), Tx + 1)) for _ in range(B - 1)], np.int32)
        ty = np.array([Ty] + [int(rng.integers(tx[b], min(Ty, tx[b] * D) + 1)) for b in range(1, B)], np.int32)
        if Ty > Tx * D:
            ty[0] = Tx * D
        txd, tyd = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
        g = torch.Generator().manual_seed(700 + n)
        e32 = torch.randn(B, Tx, Ty, generator=g) * 2
        w_la, w_ga = torch.randn(B, Tx, Ty, generator=g).to(dev), torch.randn(B, Tx, Ty, generator=g).to(dev)
        for dt in (torch.float32, torch.bfloat16):
            e = e32.to(dt).to(dev)
            out = {}
            r = aligner_amd.boundary_search(e, txd, tyd, D)
            out.update({"map only " + k: getattr(r, k) for k in ("boundaries", "durations", "map_score")})
            assert lib.aligner_debug_set_option(b"mobo_full_chain", 1) == 0
            try:
                r = aligner_amd.boundary_search(e, txd, tyd, D)
                torch.cuda.synchronize()
            finally:
                lib.aligner_debug_set_option(b"mobo_full_chain", 0)
            out.update({"map only, full kernel " + k: getattr(r, k) for k in ("boundaries", "durations", "map_score")})
            r = aligner_amd.boundary_search(e, txd, tyd, D, want_gamma=True, want_map=False)
            out.update({"sum only " + k: getattr(r, k) for k in ("log_alpha", "gamma")})
            r = aligner_amd.boundary_search(e, txd, tyd, D, want_gamma=True)
            out.update({"both " + k: getattr(r, k) for k in ("boundaries", "durations", "map_score", "log_alpha", "gamma")})
            out["backward grad_energies"] = aligner_amd.boundary_search_backward(e, txd, tyd, D, r.log_alpha, w_la, w_ga)
            torch.cuda.synchronize()
            status = mobo.read_status(dev)
            for name, t in out.items():
                print("[%d,%d,%d,%d] %-8s %-36s %s" % (B, Tx, Ty, D, str(dt).split(".")[1], name, sha(t)))
            print("[%d,%d,%d,%d] %-8s status %d" % (B, Tx, Ty, D, str(dt).split(".")[1], status))


if __name__ == "__main__":
    main()
