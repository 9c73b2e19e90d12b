"""Float64 restatement of the gradient of the Glow-TTS / VITS log-likelihood tensor (tests/gausslogp_oracle.py), for the
tests of aligner_amd.gaussian_logp_backward.  With G = dL/dvalue, d = z[c,j] - m[c,i] and w = exp(-2 s[c,i]), in the direct
(z - m) form -- not the expanded sums the kernels contract --

    dz[c,j] = - sum_i G[i,j] d w        dm[c,i] = sum_j G[i,j] d w        ds[c,i] = sum_j G[i,j] (d^2 w - 1)

over the cells inside the lengths, and beside them the magnitude of what the expanded sums add up on the raw inputs,

    S_dz[c,j] = sum_i |G[i,j]| w (|z| + |m|)     S_dm[c,i] = sum_j |G[i,j]| w (|z| + |m|)
    S_ds[c,i] = sum_j |G[i,j]| (1 + w (|z| + |m|)^2)

which is what a relative error of the split products is relative to."""
import numpy as np

import gausslogp_oracle as GO


def valid_cells(B, Tx, Ty, t_x=None, t_y=None):
    """[B,Tx,Ty] bool: the forward's clamping (an utterance with either length <= 0 is empty)."""
    tx = np.full(B, Tx) if t_x is None else np.clip(np.asarray(t_x, np.int64), 0, Tx)
    ty = np.full(B, Ty) if t_y is None else np.clip(np.asarray(t_y, np.int64), 0, Ty)
    empty = (tx <= 0) | (ty <= 0)
    tx = np.where(empty, 0, tx)
    ty = np.where(empty, 0, ty)
    return (np.arange(Tx)[None, :, None] < tx[:, None, None]) & (np.arange(Ty)[None, None, :] < ty[:, None, None])


def backward(G, z, mean, logstd, t_x=None, t_y=None, grad_scale=None):
    """G [B,Tx,Ty], z [B,C,Ty], mean / logstd [B,C,Tx] -> dict of float64 dz, dm, ds and S_dz, S_dm, S_ds.  What G holds
    outside the lengths is ignored (NaN included)."""
    z = np.asarray(z, np.float64)
    m = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64)
    B, C, Ty = z.shape
    Tx = m.shape[2]
    valid = valid_cells(B, Tx, Ty, t_x, t_y)
    G = np.where(valid, np.asarray(G, np.float64), 0.0)
    if grad_scale is not None:
        G = G * np.asarray(grad_scale, np.float64)[:, None, None]
    aG = np.abs(G)
    out = {k: np.zeros((B, C, Ty)) for k in ("dz", "S_dz")}
    out.update({k: np.zeros((B, C, Tx)) for k in ("dm", "ds", "S_dm", "S_ds")})
    for c in range(C):                                  # one channel at a time: [B,Tx,Ty] temporaries only
        zc = np.where(valid, z[:, c, None, :], 0.0)     # (a NaN of z or m outside the lengths is not an input)
        mc = np.where(valid, m[:, c, :, None], 0.0)
        w = np.where(valid, np.exp(-2.0 * s[:, c, :, None]), 0.0)
        d = zc - mc
        Gdw = G * d * w
        out["dz"][:, c, :] = -Gdw.sum(1)
        out["dm"][:, c, :] = Gdw.sum(2)
        out["ds"][:, c, :] = (G * (d * d * w - valid)).sum(2)
        mag = np.abs(zc) + np.abs(mc)
        out["S_dz"][:, c, :] = (aG * w * mag).sum(1)
        out["S_dm"][:, c, :] = (aG * w * mag).sum(2)
        out["S_ds"][:, c, :] = (aG * (valid + w * mag * mag)).sum(2)
    return out


def simulate_split(G, z, mean, logstd, t_x=None, t_y=None):
    """The kernels' arithmetic on the CPU: fp32 operands w = exp(-2 s), m w, z, z^2 and G, each split into two bf16
    halves, the three products hi*hi + hi*lo + lo*hi of the four contractions U, V (over tokens) and P, Q (over frames)
    -- multiplied and accumulated in float64 (the kernels accumulate in fp32), rounded to fp32 --, R summed without
    products, then dz = V - z U, dm = w (P - m R), ds = w (Q - 2 m P + m^2 R) - R.  Returns float64 (dz, dm, ds)."""
    z = np.asarray(z, np.float32)
    m = np.asarray(mean, np.float32)
    s = np.asarray(logstd, np.float32)
    B, C, Ty = z.shape
    Tx = m.shape[2]
    valid = valid_cells(B, Tx, Ty, t_x, t_y)
    G = np.where(valid, np.asarray(G, np.float32), np.float32(0))
    tok = valid.any(2)[:, None, :]                       # [B,1,Tx]
    frm = valid.any(1)[:, None, :]                       # [B,1,Ty]
    w = np.where(tok, np.exp(np.float32(-2.0) * s), np.float32(0)).astype(np.float32)
    mw = np.where(tok, m * w, np.float32(0)).astype(np.float32)
    zz = np.where(frm, z, np.float32(0)).astype(np.float32)
    q = zz * zz

    def halves(a):
        hi = GO._bf16(a)
        return hi.astype(np.float64), GO._bf16(a - hi).astype(np.float64)

    def three(spec, a, b):
        ah, al = halves(a)
        bh, bl = halves(b)
        return (np.einsum(spec, al, bh) + np.einsum(spec, ah, bl) + np.einsum(spec, ah, bh)).astype(np.float32).astype(np.float64)

    U = three("bci,bij->bcj", w, G)
    V = three("bci,bij->bcj", mw, G)
    P = three("bcj,bij->bci", zz, G)
    Q = three("bcj,bij->bci", q, G)
    R = G.astype(np.float64).sum(2).astype(np.float32).astype(np.float64)[:, None, :]
    m64, w64 = m.astype(np.float64), w.astype(np.float64)
    dz = np.where(frm, V - zz.astype(np.float64) * U, 0.0)
    dm = np.where(tok, w64 * (P - m64 * R), 0.0)
    ds = np.where(tok, w64 * ((Q - 2.0 * m64 * P) + m64 * m64 * R) - R, 0.0)
    return dz, dm, ds


def dense_cotangent(rng, B, Tx, Ty):
    """A dense Gaussian cotangent, fp32."""
    return rng.standard_normal((B, Tx, Ty)).astype(np.float32)


def posterior_cotangent(rng, durations, Ty):
    """A posterior-like cotangent around a planted path (durations [B,Tx]): three cells a frame -- the path's token and
    its neighbours -- negative, summing to -1 per frame; 0 elsewhere.  fp32 [B,Tx,Ty]."""
    B, Tx = durations.shape
    G = np.zeros((B, Tx, Ty), np.float32)
    for b in range(B):
        tok = np.repeat(np.arange(Tx), durations[b])
        n = len(tok)
        p = rng.dirichlet([4.0, 1.0, 1.0], n)
        for k, off in enumerate((0, -1, 1)):
            i = np.clip(tok + off, 0, max(int((durations[b] > 0).sum()) - 1, 0))
            np.add.at(G[b], (i, np.arange(n)), -p[:, k].astype(np.float32))
    return G
