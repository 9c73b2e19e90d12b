"""Float64 restatement of the Glow-TTS / VITS log-likelihood tensor, for the tests of aligner_amd.gaussian_logp.

    value[b,i,j] = sum_c ( -1/2 ln 2pi - s[b,c,i] - 1/2 (z[b,c,j] - m[b,c,i])^2 exp(-2 s[b,c,i]) )

in the direct (z - m)^2 form -- not the expanded sum the kernel contracts -- and, beside it, the per-cell magnitude of
what the expanded sum adds up on the raw inputs,

    S[b,i,j] = sum_c ( 1/2 z^2 w + |z m| w + 1/2 m^2 w + |s| + 1/2 ln 2pi ),   w = exp(-2 s)

which is what a relative error of the split products is relative to.  Cells outside the lengths hold 0.0 in `value`."""
import functools

import numpy as np

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)


def gaussian_logp(z, mean, logstd, t_x=None, t_y=None):
    """z [B,C,Ty], mean / logstd [B,C,Tx] -> (value [B,Tx,Ty], S [B,Tx,Ty], valid [B,Tx,Ty] bool), float64."""
    z = np.asarray(z, np.float64)
    m = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64)
    B, C, Ty = z.shape
    Tx = m.shape[2]
    value = np.zeros((B, Tx, Ty))
    S = np.zeros((B, Tx, Ty))
    for c in range(C):                                  # one channel at a time: [B,Tx,Ty] temporaries only
        zc = z[:, c, None, :]
        mc = m[:, c, :, None]
        sc = s[:, c, :, None]
        w = np.exp(-2.0 * sc)
        d = zc - mc
        value += -HALF_LN_2PI - sc - 0.5 * d * d * w
        S += 0.5 * zc * zc * w + np.abs(zc * mc) * w + 0.5 * mc * mc * w + np.abs(sc) + HALF_LN_2PI
    tx = np.full(B, Tx) if t_x is None else np.clip(np.asarray(t_x, np.int64), 0, Tx)
    ty = np.full(B, Ty) if t_y is None else np.clip(np.asarray(t_y, np.int64), 0, Ty)
    empty = (tx <= 0) | (ty <= 0)
    tx = np.where(empty, 0, tx)
    ty = np.where(empty, 0, ty)
    valid = (np.arange(Tx)[None, :, None] < tx[:, None, None]) & (np.arange(Ty)[None, None, :] < ty[:, None, None])
    return np.where(valid, value, 0.0), S, valid


def triple_loop(z, mean, logstd):
    """The formula cell by cell, channel by channel (tiny shapes only): value and S."""
    z = np.asarray(z, np.float64)
    m = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64)
    B, C, Ty = z.shape
    Tx = m.shape[2]
    value = np.zeros((B, Tx, Ty))
    S = np.zeros((B, Tx, Ty))
    for b in range(B):
        for i in range(Tx):
            for j in range(Ty):
                for c in range(C):
                    w = np.exp(-2.0 * s[b, c, i])
                    value[b, i, j] += -HALF_LN_2PI - s[b, c, i] - 0.5 * (z[b, c, j] - m[b, c, i]) ** 2 * w
                    S[b, i, j] += (0.5 * z[b, c, j] ** 2 * w + abs(z[b, c, j] * m[b, c, i]) * w + 0.5 * m[b, c, i] ** 2 * w
                                   + abs(s[b, c, i]) + HALF_LN_2PI)
    return value, S


def _bf16(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def simulate_split(z, mean, logstd):
    """The expanded sum with the kernel's number formats on the CPU: fp32 operands w = exp(-2 s), m w, -1/2 z^2 and z, each
    split into two bf16 halves, the three products hi*hi + hi*lo + lo*hi -- multiplied and accumulated in float64 (the
    kernel accumulates in fp32), plus the per-token constant.  [B,Tx,Ty] float64, no lengths."""
    z = np.asarray(z, np.float32)
    m = np.asarray(mean, np.float32)
    s = np.asarray(logstd, np.float32)
    w = np.exp(np.float32(-2.0) * s)
    mw = m * w
    k = ((-np.float32(HALF_LN_2PI) - s) - np.float32(0.5) * (m * mw)).astype(np.float64).sum(1)      # [B,Tx]
    A = np.concatenate([w, mw], 1)                                   # [B,2C,Tx]
    Bm = np.concatenate([np.float32(-0.5) * (z * z), z], 1)          # [B,2C,Ty]
    Ah, Bh = _bf16(A), _bf16(Bm)
    Al, Bl = _bf16(A - Ah), _bf16(Bm - Bh)
    Ah, Al, Bh, Bl = (a.astype(np.float64) for a in (Ah, Al, Bh, Bl))
    prod = np.einsum("bki,bkj->bij", Al, Bh) + np.einsum("bki,bkj->bij", Ah, Bl) + np.einsum("bki,bkj->bij", Ah, Bh)
    return prod + k[:, :, None]


def draw_inputs(rng, B, C, Tx, Ty, sigma_lo=0.5, sigma_hi=1.5, t_x=None):
    """The tests' input family: m ~ 1.5 N(0,1), sigma ~ U(sigma_lo, sigma_hi), z a mix of draws from the tokens'
    Gaussians (a random valid token per frame) and unrelated N(0,1) frames.  fp32 arrays (z, mean, logstd)."""
    m = 1.5 * rng.standard_normal((B, C, Tx))
    sig = rng.uniform(sigma_lo, sigma_hi, (B, C, Tx))
    tx = np.full(B, Tx) if t_x is None else np.maximum(np.asarray(t_x), 1)
    z = rng.standard_normal((B, C, Ty))
    for b in range(B):
        tok = rng.integers(0, tx[b], Ty)
        from_tok = rng.random(Ty) < 0.5
        zt = m[b][:, tok] + sig[b][:, tok] * rng.standard_normal((C, Ty))
        z[b] = np.where(from_tok[None, :], zt, z[b])
    return z.astype(np.float32), m.astype(np.float32), np.log(sig).astype(np.float32)


def planted(rng, C, Tx, Ty, t_x, t_y, sigma_lo, sigma_hi):
    """A planted alignment for lengths t_x / t_y [B] (1 <= t_x <= t_y): durations >= 1 for the tokens < t_x summing to t_y,
    z[:, j] = m[:, tok[j]] + sigma[:, tok[j]] eps on the frames < t_y, N(0,1) beyond.  Returns fp32 (z, mean, logstd) and
    int32 durations [B,Tx] (0 for tokens >= t_x)."""
    B = len(t_x)
    m = 1.5 * rng.standard_normal((B, C, Tx))
    sig = rng.uniform(sigma_lo, sigma_hi, (B, C, Tx))
    dur = np.zeros((B, Tx), np.int32)
    z = rng.standard_normal((B, C, Ty))
    for b in range(B):
        tx, ty = int(t_x[b]), int(t_y[b])
        extra = rng.integers(0, tx, ty - tx)
        dur[b, :tx] = 1 + np.bincount(extra, minlength=tx)
        tok = np.repeat(np.arange(tx), dur[b, :tx])
        z[b, :, :ty] = m[b][:, tok] + sig[b][:, tok] * rng.standard_normal((C, ty))
    return z.astype(np.float32), m.astype(np.float32), np.log(sig).astype(np.float32), dur


# End-to-end cases of the tests (C, Tx, Ty, sigma range, seed), B = 2: the first utterance at full size, the second
# shorter in both axes.  tests/test_gausslogp_host.py checks on the CPU that, for these seeds, the search on the float64
# values rounded to fp32 returns the planted durations and that the split products' error does not move the path.
PLANTED_CASES = [(80, 70, 200, 0.5, 1.5, 11), (80, 70, 200, 0.05, 2.0, 12), (192, 40, 120, 0.5, 1.5, 13), (192, 40, 120, 0.05, 2.0, 14)]


@functools.lru_cache(maxsize=None)
def planted_case(n):
    """Case n of PLANTED_CASES: dict of z, mean, logstd (fp32), t_x, t_y, durations (int32), value (the float64 values
    rounded to fp32, 0.0 outside the lengths) and path (the pinned search's path on them, int32).  Shared: do not modify."""
    C, Tx, Ty, lo, hi, seed = PLANTED_CASES[n]
    rng = np.random.default_rng(seed)
    t_x = np.array([Tx, (3 * Tx) // 4], np.int32)
    t_y = np.array([Ty, (4 * Ty) // 5 + 1], np.int32)
    z, m, s, dur = planted(rng, C, Tx, Ty, t_x, t_y, lo, hi)
    value = gaussian_logp(z, m, s, t_x, t_y)[0].astype(np.float32)
    path = search(value, t_x, t_y)
    return dict(z=z, mean=m, logstd=s, t_x=t_x, t_y=t_y, durations=dur, value=value, path=path)


def search(value, t_x, t_y):
    """The pinned monotonic alignment search (oracle/maxpath_oracle) on fp32 values: int32 path [B,Tx,Ty]."""
    from oracle import maxpath_oracle
    path = np.zeros(value.shape, np.int32)
    maxpath_oracle.maximum_path_c(path, np.ascontiguousarray(value, np.float32).copy(), np.ascontiguousarray(t_x, np.int32),
                                  np.ascontiguousarray(t_y, np.int32))
    return path
