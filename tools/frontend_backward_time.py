"""hipEvent times of the front end's backward entry points: aligner_softattn_backward_f32 at the bench shape
[64,80,200,1000] (and a few others), and the conv backward (aligner_conv1d_backward_weight_f32, the transposed-weight dX
convolution) at the five encoder layers of tests/test_frontend_backward_splits.py FULL_CASES beside the forward convolution
of the same layer, and the two prepare launches of the layer's weight images (what a call pays when its image is not
cached: a weight in training, a captured graph).  Prints achieved bytes/s against the compulsory traffic of each call.

    python tools/frontend_backward_time.py [--iters N] [--conv-only]

ALIGNER_AMD_LIB=<path to another build's libaligner_amd.so> times that build with the same script.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from aligner_amd import _lib  # noqa: E402


def ev(fn, it, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--conv-only", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(0)
    print("soft-attention backward (grad_logp only, no prior; dK and dQ)")
    for (B, C, Tx, Ty, sim) in [] if a.conv_only else [(64, 80, 200, 1000, "l2"), (64, 80, 200, 1000, "dot"),
                                                       (16, 128, 224, 1000, "l2"), (8, 80, 500, 2000, "l2")]:
        k = (torch.randn(B, C, Tx, generator=g) * 2).to(dev)
        q = (torch.randn(B, C, Ty, generator=g) * 2).to(dev)
        gl = torch.randn(B, Tx, Ty, generator=g).to(dev)
        gk, gq = torch.empty_like(k), torch.empty_like(q)
        nws = lib.aligner_softattn_backward_workspace_bytes(B, C, Tx, Ty)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        simc = _lib.SIM_L2 if sim == "l2" else _lib.SIM_DOT

        def run(need_k=True, need_q=True):
            _lib.check(lib.aligner_softattn_backward_f32(k.data_ptr(), q.data_ptr(), None, None, gl.data_ptr(), None,
                                                         gk.data_ptr() if need_k else None, gq.data_ptr() if need_q else None,
                                                         ws.data_ptr(), nws, B, C, Tx, Ty, 0.0005, simc, st))
        t = ev(run, a.iters)
        tq = ev(lambda: run(need_k=False), a.iters)
        nbytes = 4.0 * (B * Tx * Ty + 2 * B * C * (Tx + Ty))
        print(f"  [{B},{C},{Tx},{Ty}] {sim}: {t:.1f} us ({nbytes / t / 1e6:.2f} TB/s on {nbytes / 1e6:.1f} MB); "
              f"dQ only (column kernel) {tq:.1f} us, dK kernel {t - tq:.1f} us")
    print("conv backward (relu; dW + db + dYpre, then dX through the transposed-weight forward convolution)")
    for (B, Ci, Co, T, K, relu) in [(64, 512, 1024, 200, 3, 1), (64, 1024, 80, 200, 1, 0), (64, 1024, 80, 200, 1, 1),
                                    (64, 80, 160, 900, 3, 1), (64, 160, 80, 900, 1, 1), (64, 80, 80, 900, 1, 1)]:
        x = torch.randn(B, Ci, T, generator=g).to(dev)
        w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).to(dev)
        bias = torch.randn(Co, generator=g).to(dev)
        y = torch.randn(B, Co, T, generator=g).to(dev).relu_()        # (the timed forward overwrites it with its own output)
        gy = torch.randn(B, Co, T, generator=g).to(dev)
        gyp, gx = torch.empty_like(gy), torch.empty_like(x)
        gw, gb = torch.empty_like(w), torch.empty_like(bias)
        n = lib.aligner_conv1d_prepared_bytes(Co, Ci, K)
        prep = torch.empty(n, dtype=torch.uint8, device=dev)
        nt = lib.aligner_conv1d_prepared_bytes(Ci, Co, K)
        prept = torch.empty(nt, dtype=torch.uint8, device=dev)
        _lib.check(lib.aligner_conv1d_prepare_f32(w.data_ptr(), prep.data_ptr(), n, Co, Ci, K, st))
        _lib.check(lib.aligner_conv1d_prepare_transposed_f32(w.data_ptr(), prept.data_ptr(), nt, Co, Ci, K, st))
        nf = lib.aligner_conv1d_workspace_bytes(B, Ci, Co, T, K)
        wsf = torch.empty(max(nf, 1), dtype=torch.uint8, device=dev)
        nb = lib.aligner_conv1d_workspace_bytes(B, Co, Ci, T, K)
        wsb = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        nw = lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, K)
        wsw = torch.empty(nw, dtype=torch.uint8, device=dev)
        fwd = lambda: _lib.check(lib.aligner_conv1d_prepared_ws_f32(x.data_ptr(), prep.data_ptr(), bias.data_ptr(), y.data_ptr(),  # noqa: E731
                                                                    wsf.data_ptr(), nf, B, Ci, Co, T, K, relu, st))
        bw = lambda: _lib.check(lib.aligner_conv1d_backward_weight_f32(x.data_ptr(), y.data_ptr(), gy.data_ptr(), gyp.data_ptr(),  # noqa: E731
                                                                       gw.data_ptr(), gb.data_ptr(), wsw.data_ptr(), nw,
                                                                       B, Ci, Co, T, K, relu, st))
        bx = lambda: _lib.check(lib.aligner_conv1d_prepared_ws_f32(gyp.data_ptr(), prept.data_ptr(), None, gx.data_ptr(),  # noqa: E731
                                                                   wsb.data_ptr(), nb, B, Co, Ci, T, K, 0, st))
        tp = ev(lambda: _lib.check(lib.aligner_conv1d_prepare_f32(w.data_ptr(), prep.data_ptr(), n, Co, Ci, K, st)), a.iters)
        tpt = ev(lambda: _lib.check(lib.aligner_conv1d_prepare_transposed_f32(w.data_ptr(), prept.data_ptr(), nt, Co, Ci, K, st)),
                 a.iters)
        tf = ev(fwd, a.iters)
        tw = ev(bw, a.iters)
        tx = ev(bx, a.iters)
        fl = 2.0 * B * T * Co * Ci * K
        bytes_w = 4.0 * (B * Ci * T + 3 * B * Co * T + Co * Ci * K)
        print(f"  [{B},{Ci}->{Co},T={T},k={K},relu={relu}] forward {tf:.1f} us ({fl / tf / 1e6:.1f} TFLOP/s); "
              f"dW+db {tw:.1f} us ({fl / tw / 1e6:.1f} TFLOP/s, {bytes_w / tw / 1e6:.2f} TB/s); dX {tx:.1f} us; "
              f"backward total {tw + tx:.1f} us = {(tw + tx) / tf:.2f}x forward; prepare {tp:.1f} us, transposed {tpt:.1f} us")


if __name__ == "__main__":
    main()
