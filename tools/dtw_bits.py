#!/usr/bin/env python3
"""The bits of the warping kernels, for comparing two builds of the library: one sha256 per output of every case the GPU
tests of the three files iterate (tests/softdtw_oracle.py CASE_NAMES, tests/banddtw_oracle.py CASE_NAMES,
tests/dtwpath_oracle.py DENSE_NAMES + BAND_NAMES; the cases' inputs only, no oracle is run) -- `value` and `E` of
`soft_dtw` and `soft_dtw_banded`, `value`, `path` and `length` of `dtw_path` and `dtw_path_banded`, and the `value` of the
same call without its table (want_grad / want_path False: the forward kernels' other path).  The kernels use no atomics
and have one order of operations, so two builds that perform the same operations print the same listing:

    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/dtw_bits.py > a.txt
    python tools/dtw_bits.py > b.txt && cmp a.txt b.txt

Fails without a GPU."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import aligner_amd  # noqa: E402
import banddtw_oracle as bo  # noqa: E402
import dtwpath_oracle as dpo  # noqa: E402
import softdtw_oracle as orc  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def show(tag, names, full, bare):
    torch.cuda.synchronize()
    for name, t in zip(names, full):
        print("%-34s %-6s %s" % (tag, name, sha(t)))
    assert all(t is None for t in bare[1:])
    print("%-34s %-6s %s" % (tag, "value*", sha(bare[0])))                   # without the table


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dtw_bits.py needs a GPU")
    dev = torch.device("cuda:0")

    def i32(t):
        return None if t is None else torch.tensor(t, dtype=torch.int32, device=dev)

    for c in orc.CASES:
        args = (torch.tensor(orc.case_cost(c)).to(dev), i32(c.n), i32(c.m), c.gamma, c.p, c.band)
        show("soft_dtw " + c.name, ("value", "E"), aligner_amd.soft_dtw(*args), aligner_amd.soft_dtw(*args, want_grad=False))
    for c in bo.CASES:
        args = (torch.tensor(bo.to_band(bo.raw_cost(c), c.w)).to(dev), i32(c.n), i32(bo.m_of(c)), c.gamma, c.p)
        show("soft_dtw_banded " + c.name, ("value", "E"), aligner_amd.soft_dtw_banded(*args),
             aligner_amd.soft_dtw_banded(*args, want_grad=False))
    for name in dpo.DENSE_NAMES + dpo.BAND_NAMES:
        c = dpo.CASES[name]
        cost = dpo.case_cost(c)
        if name in dpo.BAND_NAMES:
            call, args = aligner_amd.dtw_path_banded, (torch.tensor(bo.to_band(cost, c.w)).to(dev), i32(c.n), i32(c.m), c.p)
        else:
            call, args = aligner_amd.dtw_path, (torch.tensor(cost).to(dev), i32(c.n), i32(c.m), c.p, c.w)
        show(call.__name__ + " " + name, ("value", "path", "length"), call(*args), call(*args, want_path=False))


if __name__ == "__main__":
    main()
