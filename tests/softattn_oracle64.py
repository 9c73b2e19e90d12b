"""Float64 restatement of the soft-attention front end, for the tests of aligner_amd.soft_attention.

    logit[b,i,j] = -T sum_c (q[b,c,j] - k[b,c,i])^2          (L2)
                 =  T sum_c  k[b,c,i] q[b,c,j]               (dot)
    logp = log_softmax over the text rows i < clamp(t_x, 0, Tx)  (+ log(prior + 1e-8));  -inf in the rows beyond
    soft = softmax over text of logp; 0 in the rows beyond

on the fp32 input values (and the fp32 value of the temperature, which is what the C ABI receives), and beside it the
magnitude of what the kernel's expanded logit |k|^2 + |q|^2 - 2 k.q adds up,

    S[b,i,j] = T (2 sum_c |k_ci| |q_cj| + sum_c k_ci^2 + sum_c q_cj^2)     (L2)
             = T  sum_c |k_ci| |q_cj|                                      (dot)

which is what a relative error of the split products is relative to.  An error in any row's logit moves the column's
log-sum, so bounds are per column: Scol[b,j] = max over the valid rows of S.

simulate_split / simulate_fp32_chain restate the two product forms of the kernels (three bf16 split products / an fp32
fma chain) with everything else exact: the tests take the GPU bounds from them."""
import numpy as np
import torch


def _f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float32).astype(np.float64)


def _kq(a, b):
    """sum_c a[b,c,i] b[b,c,j] -> [B,Tx,Ty]."""
    return np.matmul(a.transpose(0, 2, 1), b)


def _rows(t_x, B, Tx):
    if t_x is None:
        return np.full(B, Tx, np.int64)
    if isinstance(t_x, torch.Tensor):
        t_x = t_x.detach().cpu().numpy()
    return np.clip(np.asarray(t_x, np.int64), 0, Tx)


def logits(k, q, temperature, sim):
    """(logit, S) [B,Tx,Ty] float64."""
    k, q = _f64(k), _f64(q)
    T = float(np.float32(temperature))
    B, C, Tx = k.shape
    Ty = q.shape[2]
    aa = _kq(np.abs(k), np.abs(q))
    if sim == "dot":
        return T * _kq(k, q), T * aa
    # the expanded sum, in float64: its cancellation costs a few 2^-53 S, ten orders below what the tests measure
    # (triple_loop() is the direct difference form it is checked against)
    nn = (k * k).sum(1)[:, :, None] + (q * q).sum(1)[:, None, :]
    return -T * (nn - 2.0 * _kq(k, q)), T * (2.0 * aa + nn)


def finish(logit, t_x=None, prior=None):
    """log-softmax over the valid text rows of float64 logits (+ prior), the softmax of that, and the mask."""
    B, Tx, Ty = logit.shape
    tx = _rows(t_x, B, Tx)
    valid = np.broadcast_to(np.arange(Tx)[None, :, None] < tx[:, None, None], logit.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lg = np.where(valid, logit, -np.inf)
        m = lg.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        lse = m + np.log(np.exp(lg - m).sum(1, keepdims=True))
        logp = np.where(valid, lg - np.where(np.isfinite(lse), lse, 0.0), -np.inf)
        if prior is not None:
            logp = np.where(valid, logp + np.log(_f64(prior) + 1e-8), -np.inf)
        m2 = logp.max(1, keepdims=True)
        m2 = np.where(np.isfinite(m2), m2, 0.0)
        e = np.where(valid, np.exp(logp - m2), 0.0)
        den = e.sum(1, keepdims=True)
        soft = np.where(valid, e / np.where(den > 0, den, 1.0), 0.0)
    return logp, soft, valid


def soft_attention(k, q, t_x=None, prior=None, temperature=0.0005, sim="l2"):
    """keys [B,C,Tx], queries [B,C,Ty] -> (logp, soft, S [B,Tx,Ty], Scol [B,Ty], valid [B,Tx,Ty] bool), float64."""
    logit, S = logits(k, q, temperature, sim)
    logp, soft, valid = finish(logit, t_x, prior)
    Scol = np.where(valid, S, 0.0).max(1)
    return logp, soft, S, Scol, valid


def triple_loop(k, q, t_x, prior, temperature, sim):
    """The formulas cell by cell, channel by channel (tiny shapes only): logp, soft, S."""
    k, q = _f64(k), _f64(q)
    T = float(np.float32(temperature))
    B, C, Tx = k.shape
    Ty = q.shape[2]
    tx = _rows(t_x, B, Tx)
    logp = np.full((B, Tx, Ty), -np.inf)
    soft = np.zeros((B, Tx, Ty))
    S = np.zeros((B, Tx, Ty))
    for b in range(B):
        for j in range(Ty):
            lg = np.zeros(Tx)
            for i in range(Tx):
                for c in range(C):
                    if sim == "l2":
                        lg[i] -= T * (q[b, c, j] - k[b, c, i]) ** 2
                        S[b, i, j] += T * (2 * abs(k[b, c, i]) * abs(q[b, c, j]) + k[b, c, i] ** 2 + q[b, c, j] ** 2)
                    else:
                        lg[i] += T * k[b, c, i] * q[b, c, j]
                        S[b, i, j] += T * abs(k[b, c, i]) * abs(q[b, c, j])
            n = int(tx[b])
            if n == 0:
                continue
            lse = np.log(sum(np.exp(lg[i] - lg[:n].max()) for i in range(n))) + lg[:n].max()
            for i in range(n):
                logp[b, i, j] = lg[i] - lse
                if prior is not None:
                    logp[b, i, j] += np.log(float(np.float32(prior[b, i, j])) + 1e-8)
            den = sum(np.exp(logp[b, i, j] - logp[b, :n, j].max()) for i in range(n))
            for i in range(n):
                soft[b, i, j] = np.exp(logp[b, i, j] - logp[b, :n, j].max()) / den
    return logp, soft, S


def bf16(x):
    """float64 array -> the nearest bf16 value (round to nearest even, through fp32 as the kernels do), as float64."""
    u = np.asarray(x, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def simulate_split(k, q, temperature, sim, drop=()):
    """The logit with k.q as the kernels' three split products -- hi = bf16(x), lo = bf16(x - hi), hi*hi + hi*lo + lo*hi --
    accumulated exactly (float64); the norms and the rest of the formula in float64.  `drop` leaves products out (for the
    tests of the tests): names among "hh", "hl", "lh"."""
    k, q = _f64(k), _f64(q)
    T = float(np.float32(temperature))
    kh, qh = bf16(k), bf16(q)
    kl, ql = bf16(k - kh), bf16(q - qh)
    dot = np.zeros((k.shape[0], k.shape[2], q.shape[2]))
    for name, a, b in (("hh", kh, qh), ("hl", kh, ql), ("lh", kl, qh)):
        if name not in drop:
            dot += _kq(a, b)
    if sim == "dot":
        return T * dot
    return -T * ((k * k).sum(1)[:, :, None] + (q * q).sum(1)[:, None, :] - 2.0 * dot)


def simulate_fp32_chain(k, q, temperature, sim):
    """The logit with k.q and the norms accumulated channel by channel in np.float32 (the exact-product kernel's fma chain
    without the fused rounding: an upper estimate), the rest of the formula in float64."""
    k32 = np.asarray(_f64(k), np.float32)
    q32 = np.asarray(_f64(q), np.float32)
    T = float(np.float32(temperature))
    B, C, Tx = k32.shape
    Ty = q32.shape[2]
    dot = np.zeros((B, Tx, Ty), np.float32)
    kk = np.zeros((B, Tx), np.float32)
    qq = np.zeros((B, Ty), np.float32)
    for c in range(C):
        dot += k32[:, c, :, None] * q32[:, c, None, :]
        kk += k32[:, c] * k32[:, c]
        qq += q32[:, c] * q32[:, c]
    dot = dot.astype(np.float64)
    if sim == "dot":
        return T * dot
    return -T * (kk.astype(np.float64)[:, :, None] + qq.astype(np.float64)[:, None, :] - 2.0 * dot)


# what the GPU tests (tests/test_softattn_inputs_gpu.py) run, and the figures tests/test_softattn_host.py derives for them
GPU_SHAPES = [(80, 200, 132),      # (C, Tx, Ty): the row-tile form applies
              (80, 225, 130),      # two row groups
              (128, 224, 257),
              (256, 129, 96),      # KS = 16, two groups
              (81, 33, 31), (129, 40, 65),     # C one past a 16-step table boundary
              (1, 1, 1), (7, 31, 1), (16, 500, 33)]
GPU_CHANNELS = tuple(sorted({C for C, _, _ in GPU_SHAPES}))
GPU_TEMPERATURES = {"l2": (0.0005, 0.002), "dot": (0.11, 0.2)}        # the temperatures the split-product forms are given


def split_bound(C):
    """Bound on max |simulate_split - oracle| / Scol.  2^-17 from 80 channels on (measured at most 0.26 * 2^-16 at C = 80 / 81,
    0.18 at C = 128 / 129, 0.12 at C = 256: the products' errors average out over the channels, about 1/sqrt(C)).  Below
    that a column's error is that of a few products and the maximum over a few thousand cells reaches 2^-17 (0.56 * 2^-16
    at C = 1 and 7, 0.49 to 0.55 at [16,500,33]): the worst case of a single product instead, which holds for any C --
    x = hi + lo + r with |lo| <= 2^-8 |x| and |r| <= 2^-16 |x| (bf16 keeps 8 bits), so hi*hi + hi*lo + lo*hi misses lo*lo
    and the two r terms: 3 * 2^-16 |x y|."""
    return 2.0 ** -17 if C >= 80 else 3 * 2.0 ** -16


# max |simulate_fp32_chain - oracle| / Scol per channel count, over GPU_SHAPES, every family and both similarities
CHAIN_RATIO = {C: r * 2.0 ** -24 for C, r in {1: 0.7, 7: 1.6, 16: 3.6, 80: 9.5, 81: 8.5, 128: 14.5, 129: 11.0, 256: 16.0}.items()}
# four times what fp32 torch.log_softmax loses on exact logits (test_lse_floor: 4 x 1.61e-6)
F_LSE = 6.5e-6
# (similarity, family) on which include/aligner_amd.h keeps the 1e-4 absolute bound for the split-product kernels
PROMISED_1E_4 = {("l2", "unit"), ("l2", "scale3"), ("l2", "offset3"), ("dot", "unit")}

FAMILIES = ("unit", "offset3", "scale3", "scale10", "relu", "planted")


def planted_rows(Tx, Ty):
    """The monotonic i(j) of the `planted` family: frame j belongs to text row i(j)."""
    return (np.arange(Ty) * Tx) // max(Ty, 1)


def draw(family, rng, B, C, Tx, Ty):
    """(keys [B,C,Tx], queries [B,C,Ty]) fp32 of one input family."""
    n = lambda *s: rng.standard_normal(s)  # noqa: E731
    if family == "unit":
        k, q = n(B, C, Tx), n(B, C, Ty)
    elif family == "offset3":
        k, q = 3.0 + n(B, C, Tx), 3.0 + n(B, C, Ty)
    elif family == "scale3":
        k, q = 3.0 * n(B, C, Tx), 3.0 * n(B, C, Ty)
    elif family == "scale10":
        k, q = 10.0 * n(B, C, Tx), 10.0 * n(B, C, Ty)
    elif family == "relu":
        k, q = 2.0 * np.abs(n(B, C, Tx)), 2.0 * np.abs(n(B, C, Ty))
    elif family == "planted":
        k = 3.0 * n(B, C, Tx)
        q = k[:, :, planted_rows(Tx, Ty)] + 0.05 * n(B, C, Ty)
    else:
        raise ValueError(family)
    return k.astype(np.float32), q.astype(np.float32)
