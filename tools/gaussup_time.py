#!/usr/bin/env python3
"""Time of gaussian_upsample() on one MI355X against the path a caller composes in torch -- energy [B,T_mel,T_text], masked
fill, softmax, bmm, and .backward() -- in one process, on the same device and inputs:

    forward, C ABI                    aligner_gauss_upsample_f32 on buffers allocated once (the kernels; the wrappers are
                                      bound by the host at these sizes), every call on the next of enough copies of out to
                                      exceed the 256 MiB on-package cache
    forward + backward, C ABI         ... and aligner_gauss_upsample_backward_f32 (dh, dcentre, dprecision, dlog_weight),
                                      g_out and dh rotated likewise
    backward (dh only), C ABI         the backward call with only dh asked for
    forward, autograd                 gaussian_upsample(h, d, T_mel, t_x, t_y, ...)                  (nothing requires grad)
    forward + backward, autograd      gaussian_upsample(...).backward(G)           (h, durations and sigma require grad)
    composed forward / + backward     the torch path

at [B,C,T_text,T_mel] = [64,256,200,1000] and [64,512,200,1000], or B C Tx Ty from the command line, in the delta form
(0.1) and the sigma form (sigma drawn from [0.5, 3]), ragged lengths, durations summing to t_y.  Device events around 50
calls, seven interleaved rounds after a warm-up, the median (and minimum) of the per-call GPU time.  The compulsory bytes
are h read and out written for forward (4 B C (T_text + T_mel)); G and h read and dh written on top for backward; they
are stated over the time as a share of the 6.29 TB/s a copy reaches.  Prints a table and, last, one JSON line:
python tools/gaussup_time.py | tee profiles/gaussup_times.txt.  Fails without a GPU."""
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


def rounds(variants, n_rounds=7, it=50, warm=5):
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


def draw(B, C, Tx, Ty, seed=0):
    rng = np.random.default_rng(seed)
    t_x = rng.integers((3 * Tx) // 4, Tx + 1, B)
    t_y = rng.integers((3 * Ty) // 4, Ty + 1, B)
    t_x[0], t_y[0] = Tx, Ty
    dur = np.zeros((B, Tx), np.float32)
    for b in range(B):
        w = rng.uniform(0.3, 1.7, int(t_x[b]))
        dur[b, :int(t_x[b])] = w / w.sum() * t_y[b]
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))      # noqa: E731
    return (f(rng.standard_normal((B, C, Tx))), f(dur), f(rng.uniform(0.5, 3.0, (B, Tx))), f(rng.standard_normal((B, C, Ty))),
            torch.from_numpy(t_x.astype(np.int32)), torch.from_numpy(t_y.astype(np.int32)))


def composed(h, d, Ty, t_x, t_y, delta, sigma):
    B, C, Tx = h.shape
    d = d.clamp_min(0)
    c = torch.cumsum(d, dim=1) - 0.5 * d
    tau = torch.arange(Ty, device=h.device, dtype=torch.float32)
    dist2 = (tau[None, :, None] - c[:, None, :]) ** 2
    e = -delta * dist2 if sigma is None else -torch.log(sigma)[:, None, :] - (0.5 / (sigma * sigma))[:, None, :] * dist2
    tok = torch.arange(Tx, device=h.device)[None, :] < t_x[:, None]
    frm = torch.arange(Ty, device=h.device)[None, :] < t_y[:, None]
    p = torch.softmax(e.masked_fill(~tok[:, None, :], float("-inf")), dim=2) * frm[:, :, None]
    return torch.bmm(h, p.transpose(1, 2))


def one_shape(B, C, Tx, Ty, form, dev):
    h, d, sigma, G, t_x, t_y = (a.to(dev) for a in draw(B, C, Tx, Ty))
    sig = sigma if form == "sigma" else None
    hg, dg_, sg = h.clone().requires_grad_(), d.clone().requires_grad_(), sigma.clone().requires_grad_()

    def fused(grad):
        if not grad:
            return aligner_amd.gaussian_upsample(h, d, Ty, t_x, t_y, 0.1, sig)
        hg.grad = dg_.grad = sg.grad = None
        aligner_amd.gaussian_upsample(hg, dg_, Ty, t_x, t_y, 0.1, None if sig is None else sg).backward(G)

    def torch_path(grad):
        if not grad:
            return composed(h, d, Ty, t_x, t_y, 0.1, sig)
        hg.grad = dg_.grad = sg.grad = None
        composed(hg, dg_, Ty, t_x, t_y, 0.1, None if sig is None else sg).backward(G)

    # the C ABI on buffers allocated once
    lib = _lib.load()
    dp = d.clamp_min(0)
    cen = (torch.cumsum(dp, dim=1) - 0.5 * dp).contiguous()
    a = (0.5 / (sigma * sigma) if sig is not None else torch.full_like(cen, 0.1)).contiguous()
    lw = (-torch.log(sigma)).contiguous() if sig is not None else None
    ws_f = torch.empty(lib.aligner_gauss_upsample_workspace_bytes(B, C, Tx, Ty), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(lib.aligner_gauss_upsample_backward_workspace_bytes(B, C, Tx, Ty), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ncopies = int(CACHE_BYTES * 2.25 / (4.0 * B * C * Ty)) + 1
    outs = [torch.empty(B, C, Ty, device=dev) for _ in range(ncopies)]
    Gs = [G.clone() for _ in range(ncopies)]
    hs = [h.clone() for _ in range(ncopies)]
    dhs = [torch.empty_like(h) for _ in range(ncopies)]
    dc, da, dlw = (torch.empty_like(cen) for _ in range(3))
    turn = [0]
    lwp = None if lw is None else lw.data_ptr()

    def raw(fwd, bwd, params=True):
        i = turn[0] = (turn[0] + 1) % ncopies
        if fwd:
            _lib.check(lib.aligner_gauss_upsample_f32(hs[i].data_ptr(), cen.data_ptr(), a.data_ptr(), lwp, t_x.data_ptr(),
                                                      t_y.data_ptr(), 0.0, outs[i].data_ptr(), ws_f.data_ptr(), ws_f.numel(),
                                                      B, C, Tx, Ty, stream))
        if bwd:
            pp = (dc.data_ptr(), da.data_ptr(), None if lw is None else dlw.data_ptr()) if params else (None, None, None)
            _lib.check(lib.aligner_gauss_upsample_backward_f32(hs[i].data_ptr(), cen.data_ptr(), a.data_ptr(), lwp, t_x.data_ptr(),
                                                               t_y.data_ptr(), 0.0, Gs[i].data_ptr(), dhs[i].data_ptr(), *pp,
                                                               ws_b.data_ptr(), ws_b.numel(), B, C, Tx, Ty, stream))

    variants = {
        "forward, C ABI": lambda: raw(True, False),
        "forward + backward, C ABI": lambda: raw(True, True),
        "backward (dh only), C ABI": lambda: raw(False, True, params=False),
        "forward, autograd": lambda: fused(False),
        "forward + backward, autograd": lambda: fused(True),
        "composed forward": lambda: torch_path(False),
        "composed forward + backward": lambda: torch_path(True),
    }
    res = rounds(variants)
    # the two paths agree (fp32 against fp32)
    fused(True)
    grads = [g.grad.clone() for g in ((hg, dg_, sg) if sig is not None else (hg, dg_))]
    out_f = fused(False)
    torch_path(True)
    diff = max(((x - y.grad).abs().max() / y.grad.abs().max().clamp_min(1e-30)).item()
               for x, y in zip(grads, (hg, dg_, sg)))
    out_diff = ((out_f - torch_path(False)).abs().max() / out_f.abs().max()).item()
    fwd_bytes = 4.0 * B * C * (Tx + Ty)
    nbytes = {"forward, C ABI": fwd_bytes, "forward + backward, C ABI": fwd_bytes + 4.0 * B * C * (Ty + 2 * Tx),
              "backward (dh only), C ABI": 4.0 * B * C * (Ty + Tx)}
    rec = {"shape": [B, C, Tx, Ty], "form": form, "max_rel_out_difference": out_diff, "max_rel_grad_difference": diff, "us": {},
           "copy_share": {}}
    print(f"[{B},{C},{Tx},{Ty}] {form}: largest |fused - composed| / largest: out {out_diff:.2e}, gradients {diff:.2e}")
    for name, (med, lo) in res.items():
        line = "    %-34s median %8.1f us  min %8.1f us" % (name, med, lo)
        rec["us"][name] = {"median": round(med, 2), "min": round(lo, 2)}
        if name in nbytes:
            share = nbytes[name] / (med * 1e-6) / COPY_BYTES_PER_S
            rec["copy_share"][name] = round(share, 4)
            line += "  %6.1f MB compulsory: %4.1f %% of 6.29 TB/s" % (nbytes[name] / 1e6, 100.0 * share)
        print(line)
    rec["composed_over_fused_forward"] = round(res["composed forward"][0] / res["forward, autograd"][0], 3)
    rec["composed_over_fused_forward_backward"] = round(res["composed forward + backward"][0] / res["forward + backward, autograd"][0], 3)
    print("    composed / fused: forward %.2fx, forward + backward %.2fx"
          % (rec["composed_over_fused_forward"], rec["composed_over_fused_forward_backward"]))
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("gaussup_time.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(a) for a in sys.argv[1:5])] if len(sys.argv) > 4 else [(64, 256, 200, 1000), (64, 512, 200, 1000)]
    out = [one_shape(*shape, form, dev) for shape in shapes for form in ("delta", "sigma")]
    print(json.dumps({"tool": "gaussup_time", "device": torch.cuda.get_device_name(0), "results": out}))


if __name__ == "__main__":
    main()
