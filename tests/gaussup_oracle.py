"""Float64 oracle of Gaussian upsampling (aligner_amd/gaussup.py, csrc/gaussup.hip), the quantities its error bounds are
made of, an np.float32 restatement of the kernels' arithmetic, and the input generators of the tests.

Definition (on the fp32 input values, in float64), per utterance b with tx = clamp(t_x[b], 0, T_text),
ty = clamp(t_y[b], 0, T_mel), tau_y = y + frame_offset:

    e[y,x]   = g[x] - a[x] (tau_y - c[x])^2         x < tx
    p[y,.]   = softmax over those x
    out[:,y] = sum_x p[y,x] h[:,x]                   y < ty; 0 beyond, and everywhere when tx = 0
    q[y,x] = sum_c G[c,y] h[c,x]    r[y] = sum_x p q    de = p (q - r)                (G = 0 on a frame y >= ty)
    dh[c,x] = sum_y p[y,x] G[c,y]   dg[x] = sum_y de    da[x] = -sum_y de (tau_y - c_x)^2    dc[x] = sum_y de 2 a_x (tau_y - c_x)

Error bounds of an fp32 evaluation that follows the kernels' operation count (u = 2^-24; CUT = 30: a token whose energy
is more than CUT below the frame's maximum may count as zero).

  The energy.  d = tau - c carries u (tau = y + frame_offset is exact for the offsets used), a d d two products on top of
  d twice: 4 u of a d^2; the subtraction from g: u |e|.  |de| <= 5 u (|g| + a d^2).  The weight is exp(e - m) with m the
  frame's maximum as the kernel found it -- the same m in the numerator and in every term of the denominator, so its
  error cancels in p; e - m adds u |e - m| <= 2 u E.  With E_y = max over the tokens inside CUT of (|g| + a d^2) a weight
  is off by a relative 7 u E_y, p -- numerator against denominator -- by K' u E_y with K' = 14.

  out.  expf: 1 ulp = 2 u, in the numerator and in the denominator: 4 u; the denominator is summed in double and rounded
  once: u; the division: u; the numerator is a chain of fused multiply-adds over the band, one rounding each: a token
  inside CUT costs u of the sum of magnitudes (n_y of them), a token outside CUT has p <= e^-30 and adding it -- or not --
  moves the sum by at most its own magnitude: the truncation term covers both, hence its 2.  K = 6 <= 8:

      |out - exact| <= ((n_y + K) u + K' u E_y) sum_x p |h| + 2 T_text e^-30 max |h|

  dh[c,x] = sum_y p G, p = expf(e - m) * (1 / float(den)): expf 2 u, den's expf 2 u, its rounding u, the reciprocal u,
  the product u: 7 u <= K; the chain over the frames as above with n_x the frames on which the token is inside CUT:

      |dh - exact| <= (n_x + K) u sum_y p |G| + K' u sum_y E_y p |G| + 2 T_mel e^-30 max |G|

  dg, da, dc.  The kernel sums p q f and p r f apart (f = 1, d, d^2; r is complete only after the tile's last token) and
  subtracts per frame tile.  q: a wave's chain of fused multiply-adds holds the products of its own channels only, 16 of
  every 64 -- n_w = min(C, 16 ceil(C / 64)) of them -- and the four waves' partial sums take three additions (the first
  product and the first addition are exact): |dq| <= (n_w + 2) u Qa, Qa[y,x] = sum_c |G| |h|.  This is the one term that
  is worst-case in the channels; every other term stands on the magnitudes |q|, |r| themselves.
  r = sum_x p q: q's error summed, (n_w + 2) u Ra with Ra[y] = sum_x p Qa; p's 7 u + K' u E_y and the chain with its three
  additions, (n_y + 3) u, of Rq[y] = sum_x p |q|.
  A term p q f: q's error; p's 7 u + K' u E_y, f's 3 u and the two products' 2 u of p |q| |f|.  A term p r f: r's error;
  the same 12 u + K' u E_y of p |r| |f|.  The sums over y: six levels of the wave's butterfly, one addition per frame tile
  (nt = ceil(T_mel / 64)), the subtraction, and for da / dc the final factor: (10 + nt) u of p (|q| + |r|) |f|.  Together

      |dg - exact| <= u sum_y p |f| ( (n_w + 2) (Qa + Ra) + (22 + nt + K' E_y) (|q| + |r|) + (10 + n_y + K' E_y) Rq )
                      +  2 e^-30 sum_y (max_x Qa + Ra) |f|

  and da, dc likewise with f = d^2 and 2 a |d|.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

CUT = 30.0
U = 2.0 ** -24
K_SUM = 8
K_ENERGY = 14
TILE = 64          # frames per tile of the kernels (csrc/gaussup.hip: GU_TILE), tokens per staged chunk: 32
CHUNK = 32


def _clamp(t, B, T):
    if t is None:
        return np.full(B, T, np.int64)
    return np.clip(np.asarray(t, np.int64).reshape(B), 0, T)


def gaussian_upsample(h, c, a, g=None, t_x=None, t_y=None, frame_offset=0.0, T_mel=None, G=None, bounds=True):
    """The definition in float64.  h [B,C,Tx], c / a / g [B,Tx] (a may be a scalar), G [B,C,T_mel] or None.
    Returns out, (dh, dc, da, dg with G), p [B,Ty,Tx], and with bounds: b_out (b_dh, b_dc, b_da, b_dg), n_y, E_y."""
    h = np.asarray(h, np.float64)
    B, C, Tx = h.shape
    Ty = int(T_mel)
    c = np.asarray(c, np.float64)
    a = np.broadcast_to(np.asarray(a, np.float64), (B, Tx))
    g = np.zeros((B, Tx)) if g is None else np.broadcast_to(np.asarray(g, np.float64), (B, Tx))
    tx, ty = _clamp(t_x, B, Tx), _clamp(t_y, B, Ty)
    tau = np.arange(Ty, dtype=np.float64) + float(frame_offset)
    d = tau[None, :, None] - c[:, None, :]                                  # [B,Ty,Tx]
    e = g[:, None, :] - a[:, None, :] * d * d
    tok = np.arange(Tx)[None, :] < tx[:, None]                              # [B,Tx]
    frm = np.arange(Ty)[None, :] < ty[:, None]                              # [B,Ty]
    e = np.where(tok[:, None, :], e, -np.inf)
    with np.errstate(invalid="ignore"):
        emax = e.max(axis=2, keepdims=True) if Tx else np.zeros((B, Ty, 1))
        w = np.where(tok[:, None, :], np.exp(e - np.where(np.isfinite(emax), emax, 0.0)), 0.0)
    den = w.sum(axis=2, keepdims=True)
    p = np.where(den > 0, w / np.where(den > 0, den, 1.0), 0.0)
    p = p * frm[:, :, None]                                                 # a frame that does not count: no weights
    out = np.einsum("byx,bcx->bcy", p, h)
    res = SimpleNamespace(out=out, p=p, tx=tx, ty=ty, counts=frm & (tx > 0)[:, None])
    inside = tok[:, None, :] & (e >= emax - CUT) & frm[:, :, None]          # the tokens inside CUT
    mag = np.abs(g)[:, None, :] + a[:, None, :] * d * d
    n_y = inside.sum(axis=2)
    E_y = np.where(inside, mag, 0.0).max(axis=2) if Tx else np.zeros((B, Ty))
    res.n_y, res.E_y, res.inside = n_y, E_y, inside
    res.Sph = np.einsum("byx,bcx->bcy", p, np.abs(h))
    hmax = np.abs(h * tok[:, None, :]).max(axis=(1, 2)) if h.size else np.zeros(B)
    if bounds:
        res.b_out = (((n_y + K_SUM) * U + K_ENERGY * U * E_y)[:, None, :] * res.Sph
                     + (2 * Tx * math.exp(-CUT) * hmax)[:, None, None] * res.counts[:, None, :])
    if G is None:
        return res
    G = np.asarray(G, np.float64) * frm[:, None, :]
    q = np.einsum("bcy,bcx->byx", G, h)
    r = (p * q).sum(axis=2, keepdims=True)
    de = p * (q - r)
    res.dh = np.einsum("byx,bcy->bcx", p, G)
    res.dg = de.sum(axis=1)
    res.da = -(de * d * d).sum(axis=1)
    res.dc = (de * 2.0 * a[:, None, :] * d).sum(axis=1)
    res.q, res.r = q, r[:, :, 0]
    if bounds:
        aG = np.abs(G)
        gmax = aG.max(axis=(1, 2)) if G.size else np.zeros(B)
        n_x = inside.sum(axis=1)                                            # [B,Tx]
        res.b_dh = ((n_x + K_SUM) * U)[:, None, :] * np.einsum("byx,bcy->bcx", p, aG) \
            + K_ENERGY * U * np.einsum("byx,bcy->bcx", p * E_y[:, :, None], aG) \
            + (2 * Ty * math.exp(-CUT) * gmax)[:, None, None] * tok[:, None, :]
        Qa = np.einsum("bcy,bcx->byx", aG, np.abs(h)) * tok[:, None, :]
        Ra = (p * Qa).sum(axis=2, keepdims=True)
        nt = -(-Ty // TILE)
        nw = min(C, 16 * -(-C // 64)) + 2
        KE = K_ENERGY * E_y[:, :, None]
        aq, ar = np.abs(q), np.abs(r)
        Rq = (p * aq).sum(axis=2, keepdims=True)
        coef = U * p * (nw * (Qa + Ra) + (22 + nt + KE) * (aq + ar) + (10 + n_y[:, :, None] + KE) * Rq)
        trunc = 2 * math.exp(-CUT) * (Qa.max(axis=2, keepdims=True) + Ra) * frm[:, :, None] * tok[:, None, :]
        tot = coef + trunc
        res.b_dg = tot.sum(axis=1)
        res.b_da = (tot * d * d).sum(axis=1)
        res.b_dc = (tot * 2.0 * a[:, None, :] * np.abs(d)).sum(axis=1)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The kernels' arithmetic in np.float32 (csrc/gaussup.hip), the CUT rule and the tiles' token intervals included.
# sabotage: None, "drop_chunk_edge" (the last token of every staged chunk of 32 is left out), "drop_band_edge" (the first
# token of every tile's interval), "frame_offset" (the frames one off), "skip_r" (de = p q), "partials_off_by_1e-3" (every
# tile's sums of p q f a relative 1e-3 too large: an error at the scale of fp32 roundings gone wrong, not of a missing term).

def _f32(x):
    return np.asarray(x, np.float32)


def _energy32(tau, c, a, g):
    d = _f32(tau - c)
    return _f32(g - _f32(_f32(a * d) * d))


def band32(c, a, g, tx, ty, off, Ty):
    """[ntiles, 2] token intervals of one utterance, the way gauss_up_band_kernel finds them, and whether the
    utterance took the full range."""
    nt = -(-Ty // TILE)
    band = np.zeros((nt, 2), np.int64)
    c, a, g = _f32(c[:tx]), _f32(a[:tx]), _f32(g[:tx])
    bad = tx == 0 or not (np.all(a > 0) and np.all(np.isfinite(a)) and np.all(np.isfinite(c)) and np.all(np.isfinite(g))
                          and np.all(c[:-1] <= c[1:]))
    full = bool(bad)
    for t in range(nt):
        y0 = t * TILE
        if tx == 0 or y0 >= ty:
            continue
        band[t] = (0, tx)
        if bad:
            continue
        ys = np.arange(y0, min(y0 + TILE, ty))
        tau = _f32(_f32(ys) + np.float32(off))
        l = np.searchsorted(c, tau, side="left")
        x1, x0 = np.minimum(l, tx - 1), np.maximum(l - 1, 0)
        L = np.maximum(_energy32(tau, c[x0], a[x0], g[x0]), _energy32(tau, c[x1], a[x1], g[x1])).min()
        gmax, amin = g.max(), a.min()
        tau0, tau1 = np.float32(y0) + np.float32(off), np.float32(ys[-1]) + np.float32(off)
        span = np.float32(np.float32(gmax - L) + np.float32(CUT))
        R2 = np.float32((span + np.float32(1.0) + np.float32(1e-5) * (abs(gmax) + abs(L))) / amin)
        R = np.float32(np.sqrt(R2) * np.float32(1.0001) + np.float32(1e-6) * (abs(tau0) + abs(tau1)) + np.float32(0.01))
        if R2 >= 0 and np.isfinite(R):
            band[t] = (np.searchsorted(c, np.float32(tau0 - R), side="left"),
                       np.searchsorted(c, np.float32(tau1 + R), side="right"))
    return band, full


def restated(h, c, a, g=None, t_x=None, t_y=None, frame_offset=0.0, T_mel=None, G=None, sabotage=None):
    """out (and dh, dc, da, dg) in np.float32 the way the kernels compute them; .full[b]: the utterance took the full
    token range."""
    h = _f32(h)
    B, C, Tx = h.shape
    Ty = int(T_mel)
    c = _f32(c)
    a = _f32(np.broadcast_to(_f32(a), (B, Tx)))
    g = np.zeros((B, Tx), np.float32) if g is None else _f32(np.broadcast_to(_f32(g), (B, Tx)))
    tx, ty = _clamp(t_x, B, Tx), _clamp(t_y, B, Ty)
    off = np.float32(frame_offset + (1.0 if sabotage == "frame_offset" else 0.0))
    out = np.zeros((B, C, Ty), np.float32)
    res = SimpleNamespace(out=out, full=[], bands=[])
    if G is not None:
        G = _f32(G)
        res.dh, res.dc = np.zeros((B, C, Tx), np.float32), np.zeros((B, Tx), np.float32)
        res.da, res.dg = np.zeros((B, Tx), np.float32), np.zeros((B, Tx), np.float32)
    for b in range(B):
        band, full = band32(c[b], a[b], g[b], int(tx[b]), int(ty[b]), frame_offset, Ty)
        res.full.append(full)
        res.bands.append(band)
        for t, (lo, hi) in enumerate(band):
            if hi <= lo:
                continue
            ys = np.arange(t * TILE, min(t * TILE + TILE, int(ty[b])))
            xs = np.arange(lo, hi)
            if sabotage == "drop_band_edge":
                xs = xs[1:]
            if sabotage == "drop_chunk_edge":
                xs = xs[(xs - lo) % CHUNK != CHUNK - 1]
            if len(xs) == 0:
                continue
            tau = _f32(_f32(ys) + off)
            e = _energy32(tau[:, None], c[b, xs][None, :], a[b, xs][None, :], g[b, xs][None, :])    # [y,x]
            m = e.max(axis=1, keepdims=True)
            w = np.exp(_f32(e - m)).astype(np.float32)
            den = _f32(w.astype(np.float64).sum(axis=1, keepdims=True))
            acc = np.zeros((C, len(ys)), np.float32)
            for k, x in enumerate(xs):                                       # the chain of fused multiply-adds
                acc = _f32(acc.astype(np.float64) + w[:, k].astype(np.float64)[None, :] * h[b, :, x].astype(np.float64)[:, None])
            out[b][:, ys] = _f32(acc / den.T)
            if G is None:
                continue
            p = _f32(w * _f32(np.float32(1.0) / den))
            Gt = G[b][:, ys]                                                 # [C,y]
            qw = [np.zeros((len(ys), len(xs)), np.float32) for _ in range(4)]   # a wave: 16 of every 64 channels
            for cc in range(C):
                w4 = (cc % 64) // 16
                qw[w4] = _f32(qw[w4].astype(np.float64) + Gt[cc].astype(np.float64)[:, None] * h[b, cc, xs].astype(np.float64)[None, :])
            q = _f32(_f32(_f32(qw[0] + qw[1]) + qw[2]) + qw[3])
            d = _f32(tau[:, None] - c[b, xs][None, :])
            t0 = _f32(p * q)
            r = np.zeros(len(ys), np.float32)
            for k in range(len(xs)):
                r = _f32(r + t0[:, k])
            if sabotage == "skip_r":
                r = np.zeros_like(r)
            u0 = _f32(p * r[:, None])
            t1, u1 = _f32(t0 * d), _f32(u0 * d)
            t2, u2 = _f32(t1 * d), _f32(u1 * d)
            slip = np.float32(1.001 if sabotage == "partials_off_by_1e-3" else 1.0)
            s = [_f32(_f32(tt.sum(axis=0, dtype=np.float32) * slip) - _f32(uu.sum(axis=0, dtype=np.float32)))
                 for tt, uu in ((t0, u0), (t1, u1), (t2, u2))]
            res.dg[b, xs] = _f32(res.dg[b, xs] + s[0])
            res.dc[b, xs] = _f32(res.dc[b, xs] + s[1])
            res.da[b, xs] = _f32(res.da[b, xs] + s[2])
            for k, x in enumerate(xs):                                       # (the kernel sums a token's frames in one chain)
                res.dh[b, :, x] = _f32(res.dh[b, :, x] + _f32(Gt.astype(np.float64) * p[:, k].astype(np.float64)[None, :])
                                       .sum(axis=1, dtype=np.float32))
        if G is not None:
            res.dc[b] = _f32(_f32(np.float32(2.0) * a[b]) * res.dc[b])
            res.da[b] = _f32(-res.da[b])
    return res


# ---------------------------------------------------------------------------------------------------------------------
# Inputs

def edge_durations(rng, B, Tx, Ty, flip=0):
    """Float durations [B,Tx] fp32 (quarters of a frame, so that their sums are exact) with, in every utterance, runs of
    zero-duration tokens (coincident centres) and one negative entry (counts as 0); one token longer than two frame
    tiles where T_mel allows; utterance `flip`: a sum above T_mel and t_x < T_text (Tx > 1); the other utterances: a sum
    below T_mel, and utterance 1 - flip a t_y below its sum.  Returns durations, t_x, t_y (int32)."""
    dur = np.zeros((B, Tx), np.float32)
    t_x = np.full(B, Tx, np.int32)
    t_y = np.full(B, Ty, np.int32)
    for b in range(B):
        over = (b == flip)
        target = Ty * (1.15 if over else 0.8)
        w = rng.uniform(0.2, 1.8, Tx)
        if Tx >= 8:
            z0 = int(rng.integers(1, Tx - 4))
            w[z0:z0 + 3] = 0.0                                              # a run of zero durations
            w[int(rng.integers(0, Tx))] *= 0.0
        d = w / max(w.sum(), 1e-9) * target
        if Tx >= 3 and Ty >= 4 * TILE:
            k = int(rng.integers(0, Tx))
            d = d * (target - 2.2 * TILE) / max(target, 1e-9)
            d[k] += 2.2 * TILE                                              # longer than two frame tiles
        d = np.round(d * 4) / 4
        if Tx >= 8:
            neg = int(rng.integers(0, Tx))
            d[neg] = -1.5                                                   # counts as 0
        dur[b] = d
        tot = np.maximum(d, 0).sum()
        if over and Tx > 1:
            t_x[b] = max(Tx - max(Tx // 7, 1), 1)
        if b == 1 - flip or (B == 1 and flip == 1):
            t_y[b] = max(int(min(tot, Ty) * 0.9), 1)
    return dur, t_x, t_y


def centres_of(dur):
    """cumsum(max(d, 0)) - d / 2 in float64, rounded to fp32: what the kernels are handed."""
    d = np.maximum(np.asarray(dur, np.float64), 0)
    return (np.cumsum(d, axis=1) - 0.5 * d).astype(np.float32)


def draw_inputs(rng, B, C, Tx, Ty, form="delta", flip=0):
    """h, centres, precision, log_weight (None in the delta form), t_x, t_y, G, durations: all fp32 / int32.
    form: "delta" (a = 0.1), "sigma" (sigma in [0.5, 3]: a = 1 / (2 sigma^2), g = -ln sigma), "flat" (a = 1e-4: the band is
    everything), "shuffled" (the delta form on centres in a random order: the full-range path)."""
    h = rng.standard_normal((B, C, Tx)).astype(np.float32)
    h *= rng.uniform(0.5, 2.0, (B, 1, Tx)).astype(np.float32)
    G = rng.standard_normal((B, C, Ty)).astype(np.float32)
    dur, t_x, t_y = edge_durations(rng, B, Tx, Ty, flip)
    cen = centres_of(dur)
    a = np.full((B, Tx), 0.1, np.float32)
    g = None
    if form == "sigma":
        sigma = rng.uniform(0.5, 3.0, (B, Tx)).astype(np.float32)
        a = (0.5 / (sigma.astype(np.float64) ** 2)).astype(np.float32)
        g = (-np.log(sigma.astype(np.float64))).astype(np.float32)
    elif form == "flat":
        a = np.full((B, Tx), 1e-4, np.float32)
    elif form == "shuffled":
        for b in range(B):
            cen[b] = cen[b][rng.permutation(Tx)]
    elif form != "delta":
        raise ValueError(form)
    return dict(h=h, centres=cen, precision=a, log_weight=g, t_x=t_x, t_y=t_y, G=G, durations=dur)


# ---------------------------------------------------------------------------------------------------------------------
# The cases the host and the GPU tests share: (B, C, T_text, T_mel) at the edges of the kernels' structure -- one element;
# odd sizes, three frame tiles, no full chunk; a whole number of frame tiles and one frame past it, two channel slabs;
# tokens longer than several tiles; a large one (three channel slabs, ten chunks when the band is everything); the largest
# T_text.  The launch has one form: no shape takes another path by itself; the full token range (the path of centres out
# of order) is reached by the "shuffled" form and pinned by the library's "gaussup_full_range" switch.
SHAPES = [(1, 1, 1, 1), (3, 7, 31, 130), (2, 80, 70, 256), (2, 80, 70, 257), (2, 16, 3, 1030), (2, 192, 300, 1000),
          (1, 5, 2048, 2100)]
FORMS = ["delta", "sigma", "flat", "shuffled"]
OFFSETS = [0.0, 0.5]
CASES = [(s, f, o) for s in SHAPES for f in FORMS for o in OFFSETS]

_cache = {}


def make_case(shape, form="delta", off=0.0, flip=0):
    """The inputs and the oracle's answer, computed once and shared: never modified."""
    key = (shape, form, off, flip)
    if key not in _cache:
        B, C, Tx, Ty = shape
        rng = np.random.default_rng(1000003 * C + 1009 * Tx + 7 * Ty + FORMS.index(form) * 31 + int(off * 2) + 977 * flip)
        case = draw_inputs(rng, B, C, Tx, Ty, form, flip)
        case["off"] = off
        case["ref"] = gaussian_upsample(case["h"], case["centres"], case["precision"], case["log_weight"], case["t_x"],
                                        case["t_y"], off, Ty, case["G"])
        _cache[key] = case
    return _cache[key]


def ratio(got, want, bound):
    """max |got - want| / bound over the elements with a nonzero bound; where the bound is 0 the two must be equal."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    zero = bound == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def ratios(ref, got):
    """error / bound of out and, where `got` has them, of dh, dc, da, dg."""
    r = {"out": ratio(got.out, ref.out, ref.b_out)}
    for k in ("dh", "dc", "da", "dg"):
        if getattr(got, k, None) is not None:
            r[k] = ratio(getattr(got, k), getattr(ref, k), getattr(ref, "b_" + k))
    return r
