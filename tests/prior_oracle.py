"""High-precision oracle of the beta-binomial alignment prior (aligner_amd.beta_binomial_prior, csrc/prior.hip), the
bound an fp32 result has to meet, a float64 emulation of the kernel's two evaluation forms, and the cases the host and
the GPU tests share.

Definition (the header of csrc/prior.hip and include/aligner_amd.h), per utterance with n = t_x, per frame y < t_y:

    a = s (y + 1)      b = s (t_y - y)      s = the fp32 value of `scaling` (the C argument is a float)
    prior[x, y] = C(n, x) B(x + a, n - x + b) / B(a, b)       for x < n;   0 for x >= n and for y >= t_y

pmf(n), the mass of the (n+1)-point distribution the prior leaves out, is returned beside the column.  The lengths are
clamped, t_x to [0, Tx] and t_y to [0, Ty], as include/aligner_amd.h states for aligner_beta_binomial_prior_f32; an
utterance whose clamped t_x is 0 is all zero.

Evaluation, in mpmath at 80 digits: pmf(0) = G(n + b) G(a + b) / (G(n + a + b) G(b)) from loggamma, once per column, then

    pmf(x + 1) = pmf(x) (n - x) (x + a) / ((x + 1) (n - x - 1 + b))

which is the ratio of two neighbouring terms of the formula above; nothing of the kernel's arithmetic (log-factorial
table, walked lgamma) is used.  7679 steps lose at most 7679 * 4 roundings of 1e-80 each.

Bound of an fp32 result computed as (float) exp(lp), lp a sum of nine lgamma terms in double:

    |got - want| <= 0.5 ulp32(want) + K 2^-53 S want                                               (VALUE)

S = the sum of the magnitudes of the nine lgamma terms of the cell, ulp32 the fp32 spacing at `want` (2^-149 below
2^-126).  K counts, in units of 2^-53 S, what the double evaluation of lp and the exp can be off by.  ROCm ships no
statement of the accuracy of the device's double lgamma / log / exp, so each call is taken as good to E = 16 ulp -- an
assumption, generous for a libm, that the printed ratios are there to test -- and the rest is counted from the kernel's text:

  table form.  lp is nine table entries, each lgamma(k+1) off by E ulp of itself: E 2^-53 S in all.  Eight additions,
  each half an ulp of a partial sum that is at most S: 4.  exp: E ulp of the result, a relative E 2^-53 (S >= 0.69 on
  every cell: lgamma(n+a+b) - ... never vanish together; the host test asserts S >= 0.5, so 2 E covers it).
      K_TABLE = E + 4 + 2 E = 52
  recurrence form.  The same nine terms, but lgamma(x+a) and lgamma(n-x+b) are walked: lgamma at x = 0 plus x logs.
  The logs of one walk have one sign once their argument is past 1, so their magnitudes sum to at most
  |lgamma(x+a)| + |lgamma(a)| + 2 |log a| <= 2 S: 2 E per walk.  Each step of each walk adds once (half an ulp of a
  partial value <= S) and rounds the log's argument (half an ulp, relative, i.e. 2^-54 absolute on the log): 1 per step
  and walk.
      K_REC(x) = K_TABLE + 4 E + 2 x = 116 + 2 x

Both come from the operation count, none from a run of the kernel.  With S of order 1e2..1e5 the second term is of order
1e-12..1e-9 relative: the test is "correctly rounded to half an fp32 ulp, give or take a part in 1e9".
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import mpmath
import numpy as np

DPS = 80
E_CALL = 16                                      # ulp of one device lgamma / log / exp call (assumed; see above)
K_TABLE = E_CALL + 4 + 2 * E_CALL
TABLE_DOUBLES = 7680                             # 60 KiB of LDS in doubles
TX_MAX = TABLE_DOUBLES - 1                       # logfact[0..Tx] has to fit
MIN_NORMAL = 2.0 ** -126
_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def k_rec(x):
    return K_TABLE + 4 * E_CALL + 2.0 * np.asarray(x, np.float64)


def f32_scaling(scaling) -> float:
    """The value the kernel sees: the C argument is a float."""
    return float(np.float32(scaling))


def clamp(t, T):
    return min(max(int(t), 0), int(T))


def takes_table(Tx, Ty, scaling) -> bool:
    """The host's choice, restated from the inequality: integer scaling >= 1 and Tx + s (Ty + 1) + 2 doubles fit."""
    s = f32_scaling(scaling)
    return s >= 1.0 and s == math.floor(s) and Tx + s * (Ty + 1) + 2 <= TABLE_DOUBLES


def column_mp(n, ty, y, s, dps=DPS):
    """[pmf(0), ..., pmf(n)] of frame y as mpmath numbers; s a Python float taken exactly."""
    with mpmath.workdps(dps):
        s = mpmath.mpf(s)
        a, b = s * (y + 1), s * (ty - y)
        lg = mpmath.loggamma
        p = mpmath.exp(lg(n + b) + lg(a + b) - lg(n + a + b) - lg(b))
        out = [p]
        for x in range(n):
            p = p * (n - x) * (x + a) / ((x + 1) * (n - x - 1 + b))
            out.append(p)
        return out


def term_magnitudes(n, ty, y, s):
    """S[x], x < n: the summed magnitudes of the nine lgamma terms of log pmf(x) (float64: it only scales a bound)."""
    a, b = s * (y + 1), s * (ty - y)
    x = np.arange(n, dtype=np.float64)
    fixed = sum(abs(math.lgamma(v)) for v in (n + 1.0, n + a + b, a, b, a + b))
    per = sum(np.abs(_lgamma(v).astype(np.float64)) for v in (x + 1.0, n - x + 1.0, x + a, n - x + b))
    return fixed + per


def column(n, ty, y, scaling):
    """(values float64 [n], pmf(n) float64, S float64 [n]) of frame y of an utterance with (clamped) lengths n, ty."""
    s = f32_scaling(scaling)
    col = column_mp(n, ty, y, s)
    return np.array([float(v) for v in col[:n]]), float(col[n]), term_magnitudes(n, ty, y, s)


def sample_columns(ty):
    """The frames a large case is evaluated at: both ends, both sides of every multiple of 256, a few inside."""
    ys = {0, 1, ty - 2, ty - 1, ty // 3, ty // 2, (2 * ty) // 3 + 1, ty // 2 + 77}
    for k in range(256, ty + 1, 256):
        ys.update((k - 1, k))
    return sorted(y for y in ys if 0 <= y < ty)


def ulp32(w):
    """The fp32 spacing at w >= 0 (float64 in, float64 out): 2^(e-23) in [2^e, 2^(e+1)), 2^-149 below 2^-126."""
    w = np.asarray(w, np.float64)
    _, e = np.frexp(np.maximum(w, MIN_NORMAL))
    return np.ldexp(1.0, e - 24)


def value_bound(want, S, K):
    return 0.5 * ulp32(want) + K * 2.0 ** -53 * S * want


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's two forms in float64 (host libm in place of the device's): what a correct implementation delivers

def emulate(Tx, Ty, t_x, t_y, scaling, form=None, mutation=None):
    """prior [Tx, Ty] fp32 of one utterance as csrc/prior.hip computes it.  form: "table" / "rec" (None: the host's
    choice).  mutation: None, "top_index", "walk_b" or "lgamma32" -- the wrong kernels the bound must catch."""
    s = f32_scaling(scaling)
    n, ty = clamp(t_x, Tx), clamp(t_y, Ty)
    out = np.zeros((Tx, Ty), np.float32)
    if n < 1:
        return out
    if form is None:
        form = "table" if takes_table(Tx, Ty, scaling) else "rec"
    lgam = (lambda v: float(np.float32(math.lgamma(np.float32(v))))) if mutation == "lgamma32" else math.lgamma
    lg = np.frompyfunc(lgam, 1, 1)
    top = int(n + s * (ty + 1)) + 2
    logfact = lg(np.arange(max(n, top) + 1, dtype=np.float64) + 1.0).astype(np.float64)
    x = np.arange(n)
    with np.errstate(under="ignore"):
        for y in range(ty):
            a, b = s * (y + 1.0), s * (ty - y + 0.0)
            if form == "table":
                ia, ib = int(a), int(b)
                t = n + ia + ib - 1 + (1 if mutation == "top_index" else 0)
                frame = logfact[n] - logfact[t] - logfact[ia - 1] - logfact[ib - 1] + logfact[ia + ib - 1]
                lp = frame - logfact[x] - logfact[n - x] + logfact[x + ia - 1] + logfact[n - x + ib - 1]
            else:
                frame = logfact[n] - lgam(n + a + b) - lgam(a) - lgam(b) + lgam(a + b)
                step_b = (n - x) if mutation == "walk_b" else (n - x - 1)
                # np.cumsum adds in order, as the kernel's loop does
                l1 = np.cumsum(np.concatenate(([lgam(a)], np.log(x[:-1] + a))))
                l2 = np.cumsum(np.concatenate(([lgam(n + b)], -np.log(step_b[:-1] + b))))
                lp = frame - logfact[x] - logfact[n - x] + l1 + l2
            out[:n, y] = np.exp(lp).astype(np.float32)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# cases

def _case(name, Tx, Ty, t_x, t_y, scaling=1.0, cols="all"):
    t_x, t_y = tuple(np.atleast_1d(t_x).tolist()), tuple(np.atleast_1d(t_y).tolist())
    assert len(t_x) == len(t_y)
    return SimpleNamespace(name=name, B=len(t_x), Tx=Tx, Ty=Ty, t_x=t_x, t_y=t_y, scaling=scaling, cols=cols)


# The smallest shapes that reach each mechanism of prior_kernel.  Integer scaling takes the log-factorial table while
# Tx + s (Ty + 1) + 2 <= 7680: for s = 1 and Tx = 8 the last table shape is Ty = 7669, for s = 2 it is Ty = 3834.
SWITCH = {1.0: ((8, 7669), (8, 7670), (8, 7000)), 2.0: ((8, 3834), (8, 3835), (8, 3500))}   # table, rec, (t_x, t_y)
SCALINGS = (1.0, 2.0, 3.0, 0.5, 1.5, 0.1, 64.0)
CASES = (
    [_case(f"switch_s{int(s)}_{form}", *shape, *lens, scaling=s, cols="sampled")
     for s, (tab, rec, lens) in SWITCH.items() for form, shape in (("table", tab), ("rec", rec))]
    # the table's top index n + s (t_y + 1) - 1 on the last table shapes
    + [_case("top_index_s1", 8, 7669, 8, 7669, cols="sampled"),
       _case("top_index_s2", 8, 3834, 8, 3834, scaling=2.0, cols="sampled"),
       _case("top_index_s3", 5, 2556, 5, 2556, scaling=3.0, cols="sampled")]
    # frame blocks of 256
    + [_case(f"frames{Ty}", 5, Ty, (5, 3), (Ty, max(1, Ty - 2))) for Ty in (1, 255, 256, 257, 513)]
    + [_case("ty_one", 6, 4, 6, 1),
       _case("tx_one", 4, 300, 1, 300),                       # pmf(0) = b / (a + b)
       _case("square", 40, 40, 40, 40),
       _case("tall", 50, 20, 50, 20),                         # t_x > t_y
       # t_x: full, 0, negative, past Tx, short;  t_y: full, short, short, short, 0, past Ty, one past a block
       _case("ragged", 12, 300, (12, 0, -3, 20, 7, 9, 5), (300, 200, 100, 280, 0, 400, 257)),
       _case("largest_text", TX_MAX, 40, TX_MAX, 40, cols=(0, 1, 19, 38, 39)),
       _case("underflow", 500, 4000, 500, 4000, cols="sampled")]
    + [_case(f"scaling_{s:g}", 30, 260, (30, 11), (260, 130), scaling=s) for s in SCALINGS]
)
CASE_NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.cols == "all"]


def case(name):
    return CASES[CASE_NAMES.index(name)]


def lengths(c, b):
    return clamp(c.t_x[b], c.Tx), clamp(c.t_y[b], c.Ty)


def columns_of(c, b):
    n, ty = lengths(c, b)
    if n < 1 or ty < 1:
        return []
    if c.cols == "all":
        return list(range(ty))
    if c.cols == "sampled":
        return sample_columns(ty)
    return [y for y in c.cols if y < ty]


def form_of(c):
    return "table" if takes_table(c.Tx, c.Ty, c.scaling) else "rec"


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per utterance of a named case: SimpleNamespace(n, ty, ys, want [n, len(ys)], left_out [len(ys)], S [n, len(ys)]),
    float64, computed once per process and never modified."""
    c = case(name)
    refs = []
    for b in range(c.B):
        n, ty = lengths(c, b)
        ys = columns_of(c, b)
        want, left, S = np.zeros((n, len(ys))), np.zeros(len(ys)), np.zeros((n, len(ys)))
        for j, y in enumerate(ys):
            want[:, j], left[j], S[:, j] = column(n, ty, y, c.scaling)
        for a in (want, left, S):
            a.setflags(write=False)
        refs.append(SimpleNamespace(n=n, ty=ty, ys=np.array(ys, np.int64), want=want, left_out=left, S=S))
    return refs


def check(name, got, what, form=None):
    """Compare an fp32 prior [B, Tx, Ty] of a named case with the reference on the evaluated cells, inside VALUE and the
    consumer's log bound; prints observed / bound and returns (worst value ratio, worst log ratio, subnormal verdict).
    A cell with want < 2^-126 may also be an exact +0 (a device that flushes): the verdict says which was seen."""
    c = case(name)
    form = form or form_of(c)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (c.B, c.Tx, c.Ty)
    worst_v = worst_l = 0.0
    kept = flushed = 0
    for b, r in enumerate(reference(name)):
        if not len(r.ys):
            continue
        g = got[b, :r.n][:, r.ys].astype(np.float64)
        assert np.isfinite(g).all() and (g >= 0).all() and not np.signbit(g).any(), (name, b)
        K = K_TABLE if form == "table" else k_rec(np.arange(r.n))[:, None]
        bound = value_bound(r.want, r.S, K)
        err = np.abs(g - r.want)
        sub = r.want < MIN_NORMAL
        zero_ok = sub & (g == 0.0)
        ratio = np.where(zero_ok, 0.0, err / bound)
        tiny = sub & (r.want >= 2.0 ** -149)                  # where keeping or flushing is visible
        kept += int((tiny & (g > 0)).sum())
        flushed += int((tiny & (g == 0)).sum())
        lerr = np.abs(np.log(g + 1e-8) - np.log(r.want + 1e-8)) / 2.0 ** -22
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{what} {name}[{b}] {form} n={r.n} t_y={r.ty} s={c.scaling:g} {len(r.ys)} columns: value err / bound = "
              f"{ratio.max():.4f} at x={i[0]} y={r.ys[i[1]]} (want {r.want[i]:.6e}, err {err[i]:.3e}, bound {bound[i]:.3e}); "
              f"log err / 2^-22 = {lerr.max():.4f}; want < 2^-126: {int(sub.sum())} cells, {int((sub & (g > 0)).sum())} nonzero")
        worst_v, worst_l = max(worst_v, float(ratio.max())), max(worst_l, float(lerr.max()))
    verdict = "kept" if kept and not flushed else "flushed" if flushed and not kept else "mixed" if kept else "none seen"
    return worst_v, worst_l, verdict
