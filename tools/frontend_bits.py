#!/usr/bin/env python3
"""The bits of the front-end kernels (csrc/softattn.hip, softattn_bwd.hip, gausslogp.hip, gausslogp_bwd.hip), for
comparing two builds of the library: one sha256 per output, from fixed seeds, of

    soft_attention            in its row-tile (fp32 and bf16), strip (`softattn_strips`) and exact (`softattn_exact`) forms
    soft_attention_backward   (dk, dq), with and without a cotangent of the soft output
    gaussian_logp             fp32, bf16 and pitched
    gaussian_logp_backward    (dz, dm, ds)

at the smallest shapes [B,C,T_text,T_mel] that reach both block maps (B a multiple of 8 or not) and more than one
workgroup per utterance, each once without lengths and once with a full utterance, a t_x = 0, a t_y = 0 and lengths
below 0 and above the extent.  The further shapes change only C: 16, 40, 128 and 256 channels instantiate the other
channel counts of the same kernels.  Every sum in these kernels has a fixed order, so two builds that perform the same
operations print the same listing:

    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/frontend_bits.py > a.txt
    python tools/frontend_bits.py > b.txt && cmp a.txt b.txt

Fails without a GPU."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligner_amd  # noqa: E402
from aligner_amd import _lib  # noqa: E402

# 256- and 128-frame workgroups of the three similarity forms; the multi-row-group form; then other channel counts
SIM_SHAPES = [(8, 80, 70, 520), (3, 80, 70, 520), (8, 80, 300, 260),
              (3, 128, 70, 520), (8, 256, 150, 136), (3, 256, 40, 136), (3, 16, 70, 520), (3, 40, 70, 520)]
# 64-frame workgroups, 32-frame strips, 32-token tiles; then other channel counts
GAUSS_SHAPES = [(8, 33, 70, 200), (5, 33, 70, 200), (5, 80, 70, 200), (8, 16, 70, 200)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def lengths(B, Tx, Ty, dev):
    """Utterance 0 is full (t_x above the extent), 1 has t_x = 0, 2 a negative t_x and t_y above the extent, 3 t_y = 0,
    4 a negative t_y; the rest are ordinary."""
    t_x = [Tx + 9, 0, -3, Tx, 17, 33, Tx - 1, 32][:B]
    t_y = [Ty, 40, Ty + 5, 0, -1, 63, 64, Ty - 1][:B]
    return torch.tensor(t_x, dtype=torch.int32, device=dev), torch.tensor(t_y, dtype=torch.int32, device=dev)


def set_option(name, value):
    _lib.check(_lib.load().aligner_debug_set_option(name.encode(), value))


def show(shape, lens, outputs):
    torch.cuda.synchronize()
    for name, t in outputs.items():
        print("[%d,%d,%d,%d] %-7s %-36s %s" % (*shape, lens, name, sha(t)))


def similarity(shape, seed, dev):
    B, C, Tx, Ty = shape
    g = torch.Generator().manual_seed(seed)
    k, q = torch.randn(B, C, Tx, generator=g).to(dev), torch.randn(B, C, Ty, generator=g).to(dev)
    gl, gs = torch.randn(B, Tx, Ty, generator=g).to(dev), torch.randn(B, Tx, Ty, generator=g).to(dev)
    for lens, t_x in (("none", None), ("lengths", lengths(B, Tx, Ty, dev)[0])):
        out = {"soft_attention": aligner_amd.soft_attention(k, q, t_x=t_x)[0],
               "soft_attention bf16": aligner_amd.soft_attention(k, q, t_x=t_x, logp_dtype=torch.bfloat16)[0]}
        for form in ("softattn_strips", "softattn_exact"):
            set_option(form, 1)
            try:
                out["soft_attention " + form] = aligner_amd.soft_attention(k, q, t_x=t_x)[0]
            finally:
                set_option(form, 0)
        out["soft_attention_backward dk"], out["soft_attention_backward dq"] = aligner_amd.soft_attention_backward(k, q, gl, t_x=t_x)
        out["soft_attention_backward soft dk"], out["soft_attention_backward soft dq"] = aligner_amd.soft_attention_backward(
            k, q, gl, t_x=t_x, grad_soft=gs)
        show(shape, lens, out)


def gaussian(shape, seed, dev):
    B, C, Tx, Ty = shape
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, C, Ty, generator=g) * 1.5 + 0.25).to(dev)
    mean = torch.randn(B, C, Tx, generator=g).to(dev)
    logstd = (torch.rand(B, C, Tx, generator=g) - 0.5).to(dev)
    gv = torch.randn(B, Tx, Ty, generator=g).to(dev)
    for lens, (t_x, t_y) in (("none", (None, None)), ("lengths", lengths(B, Tx, Ty, dev))):
        out = {"gaussian_logp": aligner_amd.gaussian_logp(z, mean, logstd, t_x, t_y),
               "gaussian_logp bf16": aligner_amd.gaussian_logp(z, mean, logstd, t_x, t_y, out_dtype=torch.bfloat16),
               "gaussian_logp pitched": aligner_amd.gaussian_logp(z, mean, logstd, t_x, t_y, pitched=True)}
        grads = aligner_amd.gaussian_logp_backward(gv, z, mean, logstd, t_x, t_y)
        out.update(zip(("gaussian_logp_backward dz", "gaussian_logp_backward dm", "gaussian_logp_backward ds"), grads))
        show(shape, lens, out)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("frontend_bits.py needs a GPU")
    dev = torch.device("cuda:0")
    for i, shape in enumerate(SIM_SHAPES):
        similarity(shape, 200 + i, dev)
    for i, shape in enumerate(GAUSS_SHAPES):
        gaussian(shape, 300 + i, dev)


if __name__ == "__main__":
    main()
