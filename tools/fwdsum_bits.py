#!/usr/bin/env python3
"""The bits of the forward-sum objective, for comparing two builds of the library: one sha256 each of `loss` and `grad`
from fixed seeds, for the plain form and the CTC form (blank_logprob = -1.0), with want_grad False and True, under the
default setting and the debug options `fwdsum_serial`, `fwdsum_one_wave`, `fwdsum_serial` + `fwdsum_no_grad_stager`, and
with `logp` at a 16-byte aligned address and as a contiguous view that starts 4 bytes into a larger buffer (which sends
every call through the compiler-scheduled stagers).  Lengths are ragged: utterance 0 at full extent, one with t_x > t_y
("no alignment"), and at least one aligned utterance whose t_y is no multiple of any tile width (both asserted).  The
shapes [B,Tx,Ty] take every sweep kernel of the launch plan; where Tx > Ty an aligned utterance has at most Ty rows, so
only [2,100,140] and [64,200,1000] have real rows past a first wave's 63.  The kernels use no atomics and have one summation order, so two builds that perform the same operations
print the same listing:

    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/fwdsum_bits.py > a.txt
    python tools/fwdsum_bits.py > b.txt && cmp a.txt b.txt

Fails without a GPU."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402

ALL = ("default", "serial", "one_wave", "serial+no_grad_stager")
SHAPES = [((3, 70, 48), ALL),            # four waves, two of them own rows; three tiles; T_mel % 4 == 0
          ((3, 70, 50), ALL),            # ... four tiles, T_mel % 4 == 2
          ((3, 260, 40), ALL),           # eight waves, TW = 8
          ((3, 260, 42), ALL),
          ((2, 253, 24), ALL),           # the CTC form needs 254 rows: eight waves; the plain form's first eight-wave size
          ((2, 520, 72), ALL),           # one wave, R = 16
          ((1, 1023, 40), ALL),
          ((2, 300, 70), ("one_wave",)),   # R = 8
          ((2, 100, 140), ("one_wave",)),  # R = 4; more than two tiles of 32
          ((130, 20, 64), ALL),          # past half the CU count: serial whatever is asked
          ((64, 200, 1000), ALL)]        # bench.py's shape
OPTIONS = {"default": (), "serial": ("fwdsum_serial",), "one_wave": ("fwdsum_one_wave",),
           "serial+no_grad_stager": ("fwdsum_serial", "fwdsum_no_grad_stager")}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def lengths(rng, B, Tx, Ty):
    """Ragged.  Utterance 0 at full extent: the t_x > t_y utterance ("no alignment") when Tx > Ty.  Otherwise utterance 1
    is the t_x > t_y one, unless it is the only other one and utterance 0's t_y is a multiple of a tile width.  Then, or
    with more than two utterances, the last one is aligned, with at least half as many rows as frames and a t_y that is no
    multiple of a tile width.  One utterance only ([1,1023,40]): that last rule alone."""
    ty = rng.integers(max(Ty // 2, 2), Ty + 1, size=B)
    tx = np.minimum(rng.integers(1, Tx + 1, size=B), ty)
    tx[0], ty[0] = Tx, Ty
    k = B - 1
    if B >= 2 and Tx <= Ty and (B > 2 or Ty % 8 != 0):
        ty[1] = max(1, Tx // 2)
        tx[1] = min(Tx, ty[1] + 3)                            # t_x > t_y
        k = B - 1 if B > 2 else 0
    if k != 0 or B == 1:
        if B == 1 or ty[k] % 8 == 0:
            ty[k] = Ty - 3 if Ty % 8 != 3 else Ty - 1
        tx[k] = min(Tx, int(rng.integers((ty[k] + 1) // 2, ty[k] + 1)))
    ok = (1 <= tx) & (tx <= ty)
    assert (ok & (ty % 8 != 0)).any(), "no aligned utterance with a partial last tile"
    assert B == 1 or (tx > ty).any(), "no utterance without an alignment"
    return tx.astype(np.int32), ty.astype(np.int32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("fwdsum_bits.py needs a GPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for n, ((B, Tx, Ty), settings) in enumerate(SHAPES):
        rng = np.random.default_rng(900 + n)
        tx, ty = lengths(rng, B, Tx, Ty)
        tx, ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
        g = torch.Generator().manual_seed(1100 + n)
        lp = torch.log_softmax(torch.randn(B, Tx, Ty, generator=g) * 3, dim=1).to(dev)
        buf = torch.empty(B * Tx * Ty + 1, dtype=torch.float32, device=dev)
        off = buf[1:].view(B, Tx, Ty)
        off.copy_(lp)
        assert lp.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous()
        for setting in settings:
            try:
                for opt in OPTIONS[setting]:
                    assert lib.aligner_debug_set_option(opt.encode(), 1) == 0
                for where, x in (("aligned", lp), ("offset 4", off)):
                    for form, blank in (("plain", None), ("ctc", -1.0)):
                        for want_grad in (False, True):
                            loss, grad = aligner_amd.forward_sum(x, tx, ty, want_grad=want_grad, blank_logprob=blank)
                            torch.cuda.synchronize()
                            tag = "[%d,%d,%d] %-21s %-8s %-5s want_grad=%d" % (B, Tx, Ty, setting, where, form, want_grad)
                            print("%s loss %s" % (tag, sha(loss)))
                            if want_grad:
                                print("%s grad %s" % (tag, sha(grad)))
            finally:
                for opt in OPTIONS[setting]:
                    lib.aligner_debug_set_option(opt.encode(), 0)


if __name__ == "__main__":
    main()
