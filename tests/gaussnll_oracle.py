"""Float64 restatement of the Glow-TTS / VITS likelihood loss on the hard path, for the tests of aligner_amd.gaussian_nll.

Token x of utterance b owns the frames ends[x-1] <= y < ends[x], ends = cumsum(max(durations[b], 0)); a frame counts when
it has an owner, y < T_mel and y < t_y[b].  With w = exp(-2 s[b,c,x]), d = z[b,c,y] - m[b,c,x] on a counting frame and
n_x the counting frames of token x:

    nll[b]    = sum over the counting frames and the channels of ( 1/2 ln 2pi + s[b,c,x] + 1/2 d^2 w )
    count[b]  = number of counting frames
    dz[b,c,y] =  scale[b] d w                    (0 on a frame that does not count)
    dm[b,c,x] = -scale[b] sum_{y of x} d w       (0 for a token without a counting frame)
    ds[b,c,x] =  scale[b] ( n_x - w sum_{y of x} d^2 )

and the magnitudes the fp32 kernel's error is relative to: S_nll[b] = sum ( 1/2 ln 2pi + |s| + 1/2 d^2 w ),
A_m[b,c,x] = sum |d w|, A_s[b,c,x] = n_x + w sum d^2, absdw[b,c,y] = |d w| (all without the scale)."""
from types import SimpleNamespace

import numpy as np

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)
U = 2.0 ** -24


def owners(durations_b, T_mel, t_y=None):
    """The owner of every counting frame of one utterance, in frame order: np.repeat over the clipped durations, cut at
    T_mel and t_y.  int64 [count]."""
    d = np.maximum(np.asarray(durations_b, np.int64), 0)
    limit = T_mel if t_y is None else min(T_mel, max(int(t_y), 0))
    ends = np.minimum(np.cumsum(d), limit)                   # clipping the ends first keeps np.repeat small
    n = np.diff(np.concatenate([[0], ends]))
    return np.repeat(np.arange(len(d)), n)


def gaussian_nll(z, mean, logstd, durations, t_y=None, scale=None):
    """z [B,C,Ty], mean / logstd [B,C,Tx], durations [B,Tx] -> namespace of float64 nll [B], count [B] (int64), dz, dm,
    ds, S_nll [B], A_m, A_s [B,C,Tx], absdw [B,C,Ty], n [B,Tx] (int64) and counts [B,Ty] (bool)."""
    z = np.asarray(z, np.float64)
    m = np.asarray(mean, np.float64)
    s = np.asarray(logstd, np.float64)
    B, C, Ty = z.shape
    Tx = m.shape[2]
    sc = np.ones(B) if scale is None else np.asarray(scale, np.float64)
    r = SimpleNamespace(nll=np.zeros(B), count=np.zeros(B, np.int64), dz=np.zeros((B, C, Ty)), dm=np.zeros((B, C, Tx)),
                        ds=np.zeros((B, C, Tx)), S_nll=np.zeros(B), A_m=np.zeros((B, C, Tx)), A_s=np.zeros((B, C, Tx)),
                        absdw=np.zeros((B, C, Ty)), n=np.zeros((B, Tx), np.int64), counts=np.zeros((B, Ty), bool))
    for b in range(B):
        tok = owners(durations[b], Ty, None if t_y is None else t_y[b])
        cnt = len(tok)
        r.count[b] = cnt
        r.counts[b, :cnt] = True
        r.n[b] = np.bincount(tok, minlength=Tx)
        if cnt == 0:
            continue
        w = np.exp(-2.0 * s[b][:, tok])                      # [C,cnt]
        d = z[b][:, :cnt] - m[b][:, tok]
        r.nll[b] = (HALF_LN_2PI + s[b][:, tok] + 0.5 * d * d * w).sum()
        r.S_nll[b] = (HALF_LN_2PI + np.abs(s[b][:, tok]) + 0.5 * d * d * w).sum()
        r.dz[b][:, :cnt] = sc[b] * d * w
        r.absdw[b][:, :cnt] = np.abs(d * w)
        xs = np.flatnonzero(r.n[b])                          # the tokens with a counting frame, and where each one's
        starts = np.concatenate([[0], np.cumsum(r.n[b][xs])[:-1]])      # frames begin (tok is sorted): all channels at once

        def per_token(a):
            out = np.zeros((C, Tx))
            out[:, xs] = np.add.reduceat(a, starts, axis=1)
            return out
        sum_dw, sum_dd = per_token(d * w), per_token(d * d)
        wx = np.exp(-2.0 * s[b])                             # [C,Tx]
        r.dm[b] = -sc[b] * sum_dw
        r.ds[b] = sc[b] * (r.n[b][None, :] - wx * sum_dd)
        r.A_m[b] = per_token(np.abs(d * w))
        r.A_s[b] = r.n[b][None, :] + wx * sum_dd
        has = r.n[b] > 0
        r.dm[b][:, ~has] = 0.0
        r.ds[b][:, ~has] = 0.0
        r.A_s[b][:, ~has] = 0.0
    return r


def edge_durations(rng, B, Tx, Ty, flip=0):
    """The durations the GPU tests run every shape with, and their t_y.  Utterance 0: a sum above T_mel (clipped), full
    t_y.  Utterance 1 (shorter): a sum below T_mel, t_y below the sum.  Both: zeros in the middle (skipped tokens) and one
    negative entry, where T_text has room for them: from T_text = 3 on (there the first token owns every frame; T_text < 3
    holds neither).  flip = 1 swaps the two kinds (a batch of one utterance runs with
    either).  int32 [B,Tx], int32 [B]."""
    dur = np.zeros((B, Tx), np.int32)
    t_y = np.zeros(B, np.int32)
    for b in range(B):
        first = (b + flip) % 2 == 0
        target = Ty + max(Ty // 8, 2) if first else max((2 * Ty) // 3, 1)
        cuts = np.sort(rng.integers(0, target + 1, Tx - 1))
        d = np.diff(np.concatenate([[0], cuts, [target]])).astype(np.int32)
        if Tx >= 4:                                          # a skipped token in the middle and one negative entry
            d[Tx // 2 - 1] += d[Tx // 2]
            d[Tx // 2] = 0
            neg = Tx // 3 + 1 if Tx // 3 + 1 != Tx // 2 else Tx - 1       # (T_text = 4, 5: the last token)
            d[neg - 1 if neg - 1 != Tx // 2 else Tx // 2 - 1] += d[neg]
            d[neg] = -3
        elif Tx == 3:                                        # both, behind the one token that keeps the frames
            d[:] = (target, 0, -3)
        dur[b] = d
        total = int(np.maximum(d, 0).sum())
        t_y[b] = Ty if first else max(min(total, Ty) - max(Ty // 10, 1), 0)
    return dur, t_y
