"""TEST INFRASTRUCTURE -- the forward-sum recursion restated in float32, on the CPU.

Not a model of the HIP kernels: a yardstick for what the documented numerical scheme (csrc/forwardsum.hip's header
note) can resolve on a given input when every value of the recursion is a float32, so that a test can tell "the
kernel is wrong" from "float32 cannot do better here".  The scheme, and nothing of the kernels' organisation:

  * base-2 logs (the log-probs are scaled by log2 e on the way in);
  * FS_NEG = -1e30 stands for log 0 (a -inf log-prob is clamped to it; it absorbs every finite addend);
  * logaddexp(a, b) = max + log2(1 + exp2(-|a - b|));
  * every RB = 8 frames the column maximum is subtracted and added to a float64 offset (C forward, D backward);
    a column that is all log 0 is re-based by 0;
  * posterior = exp2(alpha + beta + float32(C_y + D_y - log2 Z)).

One offset per frame (no per-wave offsets, no drift estimate).  numpy's exp2 / log2 are correctly rounded where the
hardware's are good to ~1 ulp, and the kernels group their sums differently: tests allow the kernels a stated margin
over this restatement's error (tests/test_forward_sum_inputs.py).  log2 Z below FS_NEG / 2 is "no alignment": loss
+inf, posterior 0 -- what the float64 oracle gives for an utterance whose every path crosses a -inf cell.

Only tests/ and tools/ may import this module.  About 0.04 s per [200,1000] utterance.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
FS_NEG = F32(-1e30)
LOG2E = F32(1.4426950408889634)
LN2 = 0.6931471805599453
RB = 8


def _lae2(a, b):
    m = np.maximum(a, b)
    return m + np.log2(F32(1.0) + np.exp2(-np.abs(a - b)))


def forward_sum_one(logp: np.ndarray, tx: int, ty: int):
    """(log Z in nats as float64 -- -inf without an alignment --, posterior[Tx,Ty] float32) of one utterance."""
    Tx, Ty = logp.shape
    post = np.zeros((Tx, Ty), F32)
    if not (1 <= tx <= ty):
        return -np.inf, post
    with np.errstate(over="ignore", invalid="ignore"):
        lp = np.maximum(logp[:tx, :ty].astype(F32) * LOG2E, FS_NEG)
        lp = np.where(np.isnan(lp), FS_NEG, lp).astype(F32)      # (a NaN has no business here; -inf * log2 e is -inf)
    neg1 = np.full(1, FS_NEG, F32)
    alpha = np.empty((tx, ty), F32)
    C = np.zeros(ty, np.float64)
    a = np.full(tx, FS_NEG, F32)
    a[0] = lp[0, 0]
    c = 0.0
    for y in range(ty):
        if y:
            a = np.maximum(_lae2(a, np.concatenate((neg1, a[:-1]))) + lp[:, y], FS_NEG)
        alpha[:, y] = a
        C[y] = c
        if y % RB == RB - 1:
            m = a.max()
            if m < F32(0.5) * FS_NEG:
                m = F32(0.0)
            c += float(m)
            a = np.maximum(a - m, FS_NEG)
    lz2 = float(alpha[tx - 1, ty - 1]) + C[ty - 1]
    if lz2 < 0.5 * float(FS_NEG):
        return -np.inf, post
    beta = np.empty((tx, ty), F32)
    D = np.zeros(ty, np.float64)
    g = None
    d = 0.0
    for y in range(ty - 1, -1, -1):
        if y == ty - 1:
            b = np.full(tx, FS_NEG, F32)
            b[tx - 1] = F32(0.0)
        else:
            b = _lae2(g, np.concatenate((g[1:], neg1)))
        beta[:, y] = b
        D[y] = d
        g = np.maximum(b + lp[:, y], FS_NEG)
        if y % RB == 0:
            m = g.max()
            if m < F32(0.5) * FS_NEG:
                m = F32(0.0)
            d += float(m)
            g = np.maximum(g - m, FS_NEG)
    st = (C + D - lz2).astype(F32)
    with np.errstate(under="ignore"):
        post[:tx, :ty] = np.exp2(alpha + beta + st[None, :])
    return lz2 * LN2, post


def forward_sum(logp: np.ndarray, t_x: np.ndarray, t_y: np.ndarray):
    """loss[B] (float64 holding the float32 the scheme would output; +inf without an alignment) and
    grad[B,Tx,Ty] = -posterior (float64 holding float32 values)."""
    B = logp.shape[0]
    loss = np.zeros(B, np.float64)
    grad = np.zeros(logp.shape, np.float64)
    for b in range(B):
        lz, post = forward_sum_one(logp[b], int(t_x[b]), int(t_y[b]))
        loss[b] = np.inf if np.isneginf(lz) else float(F32(-lz))
        grad[b] = -post.astype(np.float64)
    return loss, grad
