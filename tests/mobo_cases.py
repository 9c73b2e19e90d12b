"""Inputs, error bounds and an np.float32 restatement for the boundary search (aligner_amd/mobo.py, csrc/mobo.hip), shared by
tests/test_mobo_inputs_host.py and tests/test_mobo_inputs_gpu.py.  The reference is oracle/mobo_oracle.py (float64, pinned to
brute-force enumeration in tests/test_mobo.py); this file adds what a comparison with it needs.  No GPU, no torch.

The recursion, per utterance with energies e[i, y] (nats), window D, positions j = 0..J, bands [lo_i, hi_i] (see the oracle):

    L_i(k)  = logsumexp_{m in (k, k+D], lo_i <= m <= hi_i} e_i(m)
    u_i(k)  = la_{i-1}(k) - L_i(k)                la_i(j) = e_i(j) + logsumexp_{k in [j-D, j)} u_i(k)
    v_i(k)  = de_{i-1}(k) - L_i(k)                de_i(j) = e_i(j) +    max    _{k in [j-D, j)} v_i(k)
    log_alpha[i, j-1] = la_i(j),  map_score = de_{I-1}(J),  gamma[i, y] = sum_{j<=y} exp la_{i-1}(j) - sum_{j<=y} exp la_i(j)

Error bounds of an fp32 evaluation in the kernels' form.  The kernels work in base 2: x' = x log2(e).  u = 2^-24; exp2, log2 and
rcp are good to 1 ulp = 2 u relative; every rounding below is counted to first order.  A window is summed as terms
2^(x' - ref) against an integer reference: x' - ceil(x') and every power-of-two scaling are exact, so a term carries its
exp2's 2 u.  The exact (M, s) sum adds a window's terms one after the other, the fast sums add them in trees of eight, and
adding a dead term (0) is exact: a sum of n live terms is off by at most (n - 1) u relative in either order, n at most
n_i = min(D, hi_i - lo_i + 1) for the normaliser of row i and m_i = n_{i-1} (m_0 = 1) for the window over the previous row.
A relative error r of a sum is r / ln 2 = 1.4427 r in its log2.

  One row, in base-2 units, at a live cell (k as the previous boundary, j as the new one):

    scaled energy   e' = fl(fl(e) fl(log2 e)): 2 u |e'|.  It enters la_i(j) directly and once more through L_i, as an
                    average over L's window: 2 u |e'_i(j)| + 2 u E_i, E_i = the largest live |e'| of the row
    normaliser      its terms and additions 1.4427 (n_i + 1) u;  log2 acc to 2 u |log2 acc|, and acc lies between the
                    window's smallest live term, at most min(101, spread_i + 1) + 1 below the block's reference (the fast
                    sum is only taken while every live entry is within 100 of it; spread_i = the row's largest minus its
                    smallest live e'), and D: 2 u NLOG_i, NLOG_i = min(101, spread_i + 1) + 1 + log2 D;  the add to the
                    reference u |L'_i(k)|
    u = la - L      u |u'_i(k)|
    second window   terms and additions 1.4427 (m_i + 1) u;  log2 acc: the exact sum's acc is between 1/2 and D; the fast
                    sum's is 2^(lse - R), lse = la'_i(j) - e'_i(j) the window's value and R the workgroup's reference, which
                    starts at 0 and becomes the M = ceil(u') of a live entry of an earlier row (of the row before, once a
                    workgroup has live entries; the leftmost live lane's, so often a deep tail's), and the sum is taken only
                    while every live M is within 100 of R.  With [r_lo, r_hi] the range of 0 and of every live u' of
                    the rows before (+ 1 for the ceil): 2 u CLOG_i,
                    CLOG_i = min(102 + log2 D, max(max lse - r_lo, r_hi - min lse, 1, log2 D) + 1);  the add to the
                    reference u |la'_i(j) - e'_i(j)|
    e' + (...)      u |la'_i(j)|

    cu_i(k) = u (2 E_i + 1.4427 (n_i + 1) + 2 NLOG_i + |L'_i(k)| + |u'_i(k)|)            (what forming u_i(k) adds)
    cj_i(j) = u (2 |e'_i(j)| + 1.4427 (m_i + 1) + 2 CLOG_i + |la'_i(j) - e'_i(j)| + |la'_i(j)|)   (what the cell itself adds)

  log_alpha.  An operand error passes through a logsumexp undiminished at most, so the error of row i is at most the running
  sum of the rows' largest cell bounds, c_r = max_k cu_r(k) + max_j cj_r(j) over the live cells of row r; the result is then
  scaled to nats, fl(la' fl(ln 2)): 2 u |la|.

      |log_alpha[i, j-1] - exact| <= ln 2 sum_{r <= i} c_r + 2 u |log_alpha[i, j-1]|                       (LA)

  map_score.  The max-product chain has no second window sum: v = de - L adds u |v'|, e' + best adds u |de'|, a maximum
  passes an operand error undiminished at most, and L is the same normaliser.  For EVERY boundary sequence the chain's value
  is within

      MAP = ln 2 sum_r u (4 E_r + 1.4427 (n_r + 1) + 2 NLOG_r + max |L'_r| + max |v'_r| + max |de'_r|) + 2 u |map_score|

  of its float64 log-probability.  The score the kernel returns is compared with the float64 log-probability lp of the
  kernel's OWN sequence: |score - lp| <= MAP; and its sequence is optimal within the margin want - lp <= 2 MAP (the
  kernel preferred it to the optimum by values that are each within MAP of the truth).

  gamma.  The gamma kernel sums alpha_i(j) = exp(la_i(j)) over j <= y, so what matters is the error of la weighted by
  alpha, not its maximum: deep tails carry large magnitudes and no mass.  To first order the error of la_i(j) is its own
  cj_i(j) plus the posterior average sum_k r_i(k | j) (error of la_{i-1}(k) + cu_i(k)), r_i(k | j) the derivative of the
  logsumexp; and sum_j alpha_i(j) r_i(k | j) = alpha_{i-1}(k), the chain being normalised row by row.  So the alpha-weighted
  error of row i is the running sum of the alpha-weighted cell bounds,

      A_i = A_{i-1} + sum_k alpha_{i-1}(k) cu_i(k) + sum_j alpha_i(j) cj_i(j)            (A_{-1} = 0, base-2 units)

  and the error of a partial sum of alpha_i is at most ln 2 A_i, times exp(3 LA_i) for what the first order leaves out
  (expm1(d) <= d e^d, a posterior moved by e^(2d) at most).  On top, per partial sum: the scaling to nats and __expf's own
  scaling of its argument, 4 u |la| each cell, weighted by alpha: 4 u H, H = -sum alpha ln alpha <= ln J; exp2 2 u; the
  block scan, 6 steps in a wave, up to 4 wave totals and the carry, 2 more for the exclusive sum, and 10 a chunk of 256 frames
  for the carry: SCAN = (12 + 10 ceil(Ty / 256)) u on sums that are at most 1.  The difference of the two partial sums: u.

      |gamma[i, y] - exact| <= exp(3 LA_i) ln 2 (A_{i-1} + A_i) + 2 (4 u ln J + 2 u + SCAN) + u              (GAMMA)

  Every constant comes from the operation count above, none from a run of the kernels.  The cap: no bound that is asserted
  exceeds the tolerance the older tests fitted -- 2e-3 + 2e-5 I for log_alpha and map_score, 2e-4 + 2e-6 I for gamma.  LA (at
  its largest cell) and MAP are under theirs on every case.  GAMMA is under gamma's on the cases of GAMMA_DERIVED_UNDER_CAP
  (one- and two-entry bands, D = 1, the [12, 40] shapes).  On the others the count itself is larger: the deep tails
  that the reference R may come from put log2 acc at 2 u 60 to 2 u 108 a row, the rounding of e' at 128 nats is 2^-17 a
  cell, and gamma collects two rows' worth of every row before it (GAMMA is 1.6 to 14 times the fitted tolerance there;
  the host test prints it).  Their shapes are what reaches the mechanisms, so they stay, and compare() asserts
  min(GAMMA, 2e-4 + 2e-6 I): never a weaker check than the fitted one.  The host test asserts all of this.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view as swv

from oracle import mobo_oracle as M

U = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
NEG = -np.inf
ST_BAD_LENGTHS = 1
GAMMA_DERIVED_UNDER_CAP = ("tight_ones", "tight_full", "window_one", "degenerate_lengths", "masked_runs", "constant", "two_valued")


def fitted_la_tolerance(I):
    """what tests/test_mobo.py allows on log_alpha and on map_score"""
    return 2e-3 + 2e-5 * I


def fitted_gamma_tolerance(I):
    return 2e-4 + 2e-6 * I


# ----------------------------------------------------------------------------------------------------------------------
# inputs

def _case(name, B, Tx, Ty, D, tx=None, ty=None, kind="normal", dtypes=("float32",), reaches=""):
    tx = tuple([Tx] * B if tx is None else tx)
    ty = tuple([Ty] * B if ty is None else ty)
    assert len(tx) == B and len(ty) == B
    return SimpleNamespace(name=name, B=B, Tx=Tx, Ty=Ty, D=D, tx=tx, ty=ty, kind=kind, dtypes=dtypes, reaches=reaches)


# The smallest shapes that still reach each mechanism of the kernels.  The lanes-per-position and helper-wave figures follow
# mobo_plan on 256 CUs; as in tests/test_mobo.py nothing asserts where a shape landed.
CASES = (
    _case("tight_ones", 2, 40, 40, 8, (40, 33), (40, 33), reaches="one-entry bands, all durations 1"),
    _case("tight_full", 2, 12, 96, 8, (12, 11), (96, 88), reaches="all durations D"),
    _case("slack_one", 2, 40, 41, 8, (40, 5), (41, 39), reaches="bands of two; t_y = t_x D - 1"),
    _case("window_one", 1, 65, 65, 1, reaches="D = 1 across a wave edge"),
    _case("window_clamped", 2, 20, 90, 1000, (20, 20), (90, 20), reaches="D clamped to Ty"),
    _case("short_in_long", 6, 80, 300, 4, (80, 5, 2, 1, 1, 75), (300, 20, 7, 1, 4, 300),
          reaches="fewer segments than the launch; a last segment of one position (J = 20: 5, 5, 5, 5, 1); P / D < S"),
    _case("last_segment_short", 1, 10, 1001, 250, reaches="a last segment of 249 positions, shorter than the window"),
    _case("degenerate_lengths", 6, 12, 40, 8, (12, 0, 12, 12, 99, 4), (40, 40, 0, 11, 999, 40),
          reaches="t_x = 0, t_y = 0, t_y < t_x, lengths beyond the tensor (clamped), t_y > t_x D"),
    _case("offsets_h4_helper", 3, 40, 300, 16, (40, 31, 25), (300, 280, 300), kind="offsets", reaches="4 lanes a position, helper"),
    _case("offsets_h4", 4, 12, 40, 8, (12, 9, 12, 5), (40, 40, 33, 40), kind="offsets", reaches="4 lanes a position"),
    _case("offsets_h2_helper", 2, 30, 1100, 64, (30, 24), (1100, 1000), kind="offsets", reaches="2 lanes a position, helper"),
    _case("offsets_h2", 1, 4, 100, 60, kind="offsets", reaches="2 lanes a position"),
    _case("offsets_h1_helper", 1, 12, 600, 100, kind="offsets", reaches="1 lane a position, helper"),
    _case("offsets_h1", 1, 4, 300, 200, kind="offsets", reaches="1 lane a position"),
    _case("offsets_several", 1, 6, 2600, 1300, kind="offsets", reaches="several positions per thread"),
    _case("cliff_block_edge", 2, 30, 1100, 64, (30, 25), (1100, 1060), kind="cliff",
          reaches="a step of 160 nats inside a window, across the normaliser's 1024-position block and a segment halo"),
    _case("masked_runs", 3, 12, 90, 10, kind="masked_runs", reaches="random -inf; a masked run of D - 1 frames; one of D"),
    _case("masked_sixteen_bit", 2, 20, 150, 16, (20, 13), (150, 90), kind="masked16", dtypes=("bfloat16", "float16"),
          reaches="random -inf in 16-bit energies"),
    _case("constant", 2, 12, 40, 8, (12, 9), (40, 33), kind="constant", reaches="every sequence ties"),
    _case("two_valued", 2, 12, 40, 8, (12, 9), (40, 33), kind="two_valued", reaches="near-ties for the MAP search"),
)
CASE_NAMES = [c.name for c in CASES]
OFFSET_CASES = [c.name for c in CASES if c.kind == "offsets"]
CLIFF_FRAME, CLIFF_DROP = 1027, 160.0


def case(name):
    return CASES[CASE_NAMES.index(name)]


def row_offsets(Tx):
    """128 ((i // 3) % 3 - 1) nats: the reference of the fast sums is stale at every third row and tracks in between"""
    i = np.arange(Tx)
    return (128.0 * ((i // 3) % 3 - 1)).astype(np.float32)


def _quantised(rng, shape, step=256.0, clip=None):
    e = np.round(rng.standard_normal(shape) * 2.0 * step) / step
    if clip is not None:
        e = np.clip(e, -clip, clip)
    return e.astype(np.float32)


@functools.lru_cache(maxsize=None)
def energies(name, twin=False):
    """[B,Tx,Ty] fp32, deterministic from the name, multiples of 2^-8 (so that adding a row offset is exact in fp32; the
    16-bit case: multiples of 2^-4 within +-15, exact in bf16 and fp16).  twin: an offset case without its offsets."""
    c = case(name)
    rng = np.random.default_rng(sum(ord(ch) for ch in name) * 7919 + c.Tx * 31 + c.Ty)
    shape = (c.B, c.Tx, c.Ty)
    if c.kind == "constant":
        e = np.zeros(shape, np.float32)
    elif c.kind == "two_valued":
        e = rng.integers(0, 2, shape).astype(np.float32)
    elif c.kind == "masked16":
        e = _quantised(rng, shape, 16.0, 15.0)
        e[rng.random(shape) < 0.05] = NEG
        e[:, :, -1] = np.where(np.isfinite(e[:, :, -1]), e[:, :, -1], 0.0)
        for b in range(c.B):                                   # the last token must be able to end at the utterance's end
            e[b, c.tx[b] - 1, c.ty[b] - 1] = 0.5
    else:
        e = _quantised(rng, shape)
    if c.kind == "offsets" and not twin:
        e = e + row_offsets(c.Tx)[None, :, None]
    if c.kind == "cliff":
        e[:, :, CLIFF_FRAME:] -= np.float32(CLIFF_DROP)
    if c.kind == "masked_runs":
        mask = rng.random((c.Tx, c.Ty)) < 0.1
        mask[:, -1] = False
        e[0][mask] = NEG
        e[1, :, 30:30 + c.D - 1] = NEG                          # a run of D - 1 frames: a token of D frames steps over it
        e[2, :, 30:30 + c.D] = NEG                              # a run of D: nothing does
    e.setflags(write=False)
    return e


def clamped_lengths(c, b):
    """(I, J, has_lengths): the lengths as the kernels clamp them, and whether a segmentation can exist at all"""
    I, J = min(int(c.tx[b]), c.Tx), min(int(c.ty[b]), c.Ty)
    return I, J, M.feasible(I, J, min(c.D, c.Ty))


# ----------------------------------------------------------------------------------------------------------------------
# the float64 rows and the bounds

def rows64(e, D):
    """la [I+1, J+1], de [I+1, J+1] (row 0: the start), L [I, J+1] in float64 nats, -inf = log 0."""
    e = np.asarray(e, np.float64)
    I, J = e.shape
    la = np.full((I + 1, J + 1), NEG)
    la[0, 0] = 0.0
    de = la.copy()
    Ls = np.full((I, J + 1), NEG)
    pos = np.arange(J + 1)
    for i in range(I):
        lo, hi = M.band(I, J, D, i)
        s = np.full(J + 1, NEG)
        s[1:] = e[i]
        feas = (pos >= lo) & (pos <= hi)
        sm = np.where(feas, s, NEG)
        L = np.full(J + 1, NEG)
        L[:J] = M.lse_rows(swv(np.concatenate([sm[1:], np.full(D, NEG)]), D)[:J])
        Ls[i] = L
        idx = np.nonzero(feas)[0]
        for prev, out, reduce in ((la, la, M.lse_rows), (de, de, lambda w: w.max(axis=1))):
            with np.errstate(invalid="ignore"):
                x = np.where(np.isfinite(L) & np.isfinite(prev[i]), prev[i] - L, NEG)
            xw = swv(np.concatenate([np.full(D, NEG), x]), D)[:J + 1]
            row = np.full(J + 1, NEG)
            row[idx] = s[idx] + reduce(xw[idx])
            out[i + 1] = row
    return la, de, Ls


def bounds(e, D, Ty=None):
    """LA [I] (ln 2 sum_{r<=i} c_r: add 2 u |log_alpha| per cell), GAMMA [I] and MAP (add 2 u |map_score|) of one utterance
    e [I, J], from the module docstring; float64 nats."""
    e = np.asarray(e, np.float64)
    I, J = e.shape
    Ty = J if Ty is None else Ty
    la, de, Ls = rows64(e, D)
    lg = math.log2(D)
    r_lo, r_hi = 0.0, 0.0                 # what the fast sums' reference R can be: 0, or an M of a live u' of a row before
    pos = np.arange(J + 1)
    c_row = np.zeros(I)
    cm_row = np.zeros(I)
    a_row = np.zeros(I)
    n_prev = 1
    for i in range(I):
        lo, hi = M.band(I, J, D, i)
        n_i = min(D, hi - lo + 1)
        s = np.full(J + 1, NEG)
        s[1:] = e[i]
        live_e = (pos >= lo) & (pos <= hi) & np.isfinite(s)
        if not live_e.any():
            n_prev = n_i
            continue
        e2 = s[live_e] * LOG2E
        E_i = np.abs(e2).max()
        nlog = min(101.0, e2.max() - e2.min() + 1.0) + 1.0 + lg
        live_k = np.isfinite(Ls[i]) & np.isfinite(la[i])
        live_j = np.isfinite(la[i + 1])
        cu = np.zeros(J + 1)
        cu[live_k] = U * (2 * E_i + LOG2E * (n_i + 1) + 2 * nlog
                          + (np.abs(Ls[i][live_k]) + np.abs(la[i][live_k] - Ls[i][live_k])) * LOG2E)
        clog = 102.0 + lg
        if live_j.any():
            lse = (la[i + 1][live_j] - s[live_j]) * LOG2E
            clog = min(clog, max(lse.max() - r_lo, r_hi - lse.min(), 1.0, lg) + 1.0)
        if live_k.any():
            u2 = (la[i][live_k] - Ls[i][live_k]) * LOG2E
            r_lo, r_hi = min(r_lo, u2.min()), max(r_hi, u2.max() + 1.0)
        cj = np.zeros(J + 1)
        cj[live_j] = U * (LOG2E * (n_prev + 1) + 2 * clog
                          + (2 * np.abs(s[live_j]) + np.abs(la[i + 1][live_j] - s[live_j]) + np.abs(la[i + 1][live_j])) * LOG2E)
        c_row[i] = cu.max() + cj.max()
        a_row[i] = (np.exp(la[i][live_k]) * cu[live_k]).sum() + (np.exp(la[i + 1][live_j]) * cj[live_j]).sum()
        live_v = np.isfinite(Ls[i]) & np.isfinite(de[i])
        live_d = np.isfinite(de[i + 1])
        if live_v.any() and live_d.any():
            cm_row[i] = U * (4 * E_i + LOG2E * (n_i + 1) + 2 * nlog
                             + (np.abs(Ls[i][live_v]).max() + np.abs(de[i][live_v] - Ls[i][live_v]).max()
                                + np.abs(de[i + 1][live_d]).max()) * LOG2E)
        n_prev = n_i
    LA = LN2 * np.cumsum(c_row)
    A = np.concatenate([[0.0], LN2 * np.cumsum(a_row)])
    per_sum = 4 * U * math.log(max(J, 2)) + 2 * U + (12 + 10 * math.ceil(Ty / 256)) * U
    GAMMA = np.exp(3 * LA) * (A[:-1] + A[1:]) + 2 * per_sum + U
    return SimpleNamespace(LA=LA, GAMMA=GAMMA, MAP=float(LN2 * cm_row.sum()))


@functools.lru_cache(maxsize=None)
def reference(name, twin=False):
    """Per utterance of a named case None (its lengths allow no segmentation) or a namespace with I, J, the energies
    e [I,J] float64, the oracle's result `want`, `has_answer` (False: masked frames leave no segmentation) and the bounds
    `bd`.  Computed once per process and never modified."""
    c = case(name)
    e = energies(name, twin)
    D = min(c.D, c.Ty)
    out = []
    for b in range(c.B):
        I, J, ok = clamped_lengths(c, b)
        if not ok:
            out.append(None)
            continue
        e64 = e[b, :I, :J].astype(np.float64)
        want = M.boundary_search_fast(e64, D)
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out.append(SimpleNamespace(I=I, J=J, e=e64, want=want, has_answer=bool(np.isfinite(want["map_score"])),
                                   bd=bounds(e64, D, c.Ty)))
    return tuple(out)


def compare(name, got, what):
    """Compare a batch of results (dict of numpy arrays: log_alpha, gamma [B,Tx,Ty], boundaries, durations [B,Tx], map_score
    [B]) with the reference inside LA, GAMMA and MAP.  Prints observed / bound per utterance and returns the list of what is
    wrong (empty: all inside)."""
    c = case(name)
    D = min(c.D, c.Ty)
    wrong = []
    la_all = np.asarray(got["log_alpha"], np.float64)
    ga_all = np.asarray(got["gamma"], np.float64)
    for b, ref in enumerate(reference(name)):
        bnd, dur, sc = np.asarray(got["boundaries"][b]), np.asarray(got["durations"][b]), float(got["map_score"][b])
        if ref is None or not ref.has_answer:
            if bnd.any() or dur.any() or sc != NEG:
                wrong.append(f"{name}[{b}]: no segmentation exists, yet boundaries / durations / score are not 0 / 0 / -inf")
        if ref is None:
            if not np.all(np.isneginf(la_all[b])) or ga_all[b].any():
                wrong.append(f"{name}[{b}]: lengths without a segmentation, yet log_alpha is not all -inf or gamma not all 0")
            print(f"{what} {name}[{b}]: lengths ({c.tx[b]}, {c.ty[b]}) allow no segmentation")
            continue
        I, J, want, bd = ref.I, ref.J, ref.want, ref.bd
        la, ga = la_all[b, :I, :J], ga_all[b, :I, :J]
        if not (np.all(np.isneginf(la_all[b, I:])) and np.all(np.isneginf(la_all[b, :I, J:]))):
            wrong.append(f"{name}[{b}]: log_alpha is not -inf outside the lengths")
        if ga_all[b, I:].any() or ga_all[b, :, J:].any():
            wrong.append(f"{name}[{b}]: gamma is not 0 outside the lengths")
        fin = np.isfinite(want["log_alpha"])
        if not np.array_equal(np.isfinite(la), fin) or not np.all(np.isneginf(la[~fin])):
            wrong.append(f"{name}[{b}]: the finite entries of log_alpha are not the oracle's")
            continue
        la_bound = bd.LA[:, None] + 2 * U * np.abs(want["log_alpha"])
        r_la = float(np.max(np.where(fin, np.abs(np.where(fin, la, 0.0) - np.where(fin, want["log_alpha"], 0.0)), 0.0)
                            / np.where(fin, la_bound, 1.0)))
        e_ga = np.abs(ga - want["gamma"]).max(axis=1)
        ga_bound = np.minimum(bd.GAMMA, fitted_gamma_tolerance(I))           # (the cap: the module docstring)
        r_ga = float(np.max(e_ga / ga_bound))
        line = (f"{what} {name}[{b}] I={I} J={J}: log_alpha err / bound = {r_la:.4f} (bound {bd.LA[-1]:.2e} at the last row);  "
                f"gamma err {e_ga.max():.2e} / bound = {r_ga:.4f} (bound {ga_bound.max():.2e}, derived {bd.GAMMA.max():.2e})")
        if r_la > 1.0:
            wrong.append(f"{name}[{b}]: log_alpha outside LA, err / bound = {r_la:.3f}")
        if r_ga > 1.0:
            wrong.append(f"{name}[{b}]: gamma outside GAMMA, err / bound = {r_ga:.3f}")
        if ref.has_answer:
            bb = bnd[:I]
            valid = (np.array_equal(np.diff(np.concatenate([[0], bb])), dur[:I]) and bb[-1] == J and dur[:I].min() >= 1
                     and dur[:I].max() <= D and np.all(bnd[I:] == J) and not dur[I:].any())
            lp = M.sequence_log_prob(ref.e, D, bb) if valid else NEG
            if not valid or not np.isfinite(lp):
                wrong.append(f"{name}[{b}]: the MAP sequence is not a segmentation of positive probability")
            else:
                mb = bd.MAP + 2 * U * abs(lp)
                r_sc, r_opt = abs(sc - lp) / mb, (want["map_score"] - lp) / (2 * mb)
                line += f";  map_score err {abs(sc - lp):.2e} / bound {mb:.2e} = {r_sc:.4f};  optimum - own / margin = {r_opt:.4f}"
                if not r_sc <= 1.0:
                    wrong.append(f"{name}[{b}]: map_score outside MAP, err / bound = {r_sc:.3f}")
                if not r_opt <= 1.0:
                    wrong.append(f"{name}[{b}]: the MAP sequence is {want['map_score'] - lp:.3e} below the optimum, margin {2 * mb:.3e}")
        else:
            line += ";  masked frames leave no segmentation"
        print(line)
    return wrong


# ----------------------------------------------------------------------------------------------------------------------
# the recursion in np.float32: base 2, every window summed against its own maximum (not the kernels' (M, s) encoding)

SABOTAGES = ("window_shifted", "lo_without_reach", "normaliser_of_previous_row", "row_max_reference")


def _lse2_rows32(w, ref=None):
    """log2 sum 2^w along the last axis in fp32, against each window's own maximum (or against `ref`, one number)."""
    f = np.float32
    m = w.max(axis=1) if ref is None else np.full(w.shape[0], ref, f)
    ok = np.isfinite(m) & np.isfinite(w.max(axis=1))
    out = np.full(w.shape[0], NEG, f)
    if ok.any():
        with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
            acc = np.exp2(w[ok] - m[ok, None]).astype(f).sum(axis=1, dtype=f)
            out[ok] = m[ok] + np.log2(acc)
    return out


def boundary_search32(e, D, sabotage=None):
    """log_alpha, gamma [I,J] fp32, boundaries, durations [I] int32 and map_score of ONE utterance e [I,J], every operation in
    np.float32.  sabotage: None or one of SABOTAGES -- the wrong kernels the bounds must catch:
    "window_shifted" the window over the previous row is [j-D+1, j] instead of [j-D, j); "lo_without_reach" lo_i = i + 1;
    "normaliser_of_previous_row" u_i = la_{i-1} - L_{i-1}; "row_max_reference" every window is summed against the row's
    maximum, which loses the deep tails."""
    assert sabotage is None or sabotage in SABOTAGES
    f = np.float32
    e = np.asarray(e, f)
    I, J = e.shape
    with np.errstate(invalid="ignore"):
        e2 = (e * f(LOG2E)).astype(f)
    la_prev = np.full(J + 1, NEG, f)
    la_prev[0] = 0
    de_prev = la_prev.copy()
    L_before = None
    log_alpha = np.full((I, J), NEG, f)
    back = np.zeros((I, J + 1), np.int64)
    pos = np.arange(J + 1)
    shift = 1 if sabotage == "window_shifted" else 0
    for i in range(I):
        lo, hi = M.band(I, J, D, i)
        if sabotage == "lo_without_reach":
            lo = i + 1
        s = np.full(J + 1, NEG, f)
        s[1:] = e2[i]
        feas = (pos >= lo) & (pos <= hi)
        sm = np.where(feas, s, f(NEG))
        row_ref = sm.max() if sabotage == "row_max_reference" else None
        L = np.full(J + 1, NEG, f)
        L[:J] = _lse2_rows32(swv(np.concatenate([sm[1:], np.full(D, NEG, f)]), D)[:J], row_ref)
        Lu = L_before if (sabotage == "normaliser_of_previous_row" and L_before is not None) else L
        L_before = L
        with np.errstate(invalid="ignore"):
            u = np.where(np.isfinite(Lu) & np.isfinite(la_prev), la_prev - Lu, f(NEG)).astype(f)
            v = np.where(np.isfinite(Lu) & np.isfinite(de_prev), de_prev - Lu, f(NEG)).astype(f)
        pad = np.full(D, NEG, f)
        uw = swv(np.concatenate([pad, u, pad[:1]]), D)[shift:J + 1 + shift]
        vw = swv(np.concatenate([pad, v, pad[:1]]), D)[shift:J + 1 + shift]
        idx = np.nonzero(feas)[0]
        la = np.full(J + 1, NEG, f)
        de = np.full(J + 1, NEG, f)
        la[idx] = s[idx] + _lse2_rows32(uw[idx], u.max() if sabotage == "row_max_reference" else None)
        vmax = vw[idx].max(axis=1)
        last = D - 1 - np.argmax(vw[idx][:, ::-1], axis=1)
        okv = np.isfinite(vmax) & np.isfinite(s[idx])
        de[idx[okv]] = s[idx[okv]] + vmax[okv]
        back[i, idx[okv]] = idx[okv] - D + last[okv] + shift
        log_alpha[i] = la[1:] * f(LN2)
        la_prev, de_prev = la, de
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):      # (a sabotaged chain may overflow)
        alpha = np.exp(log_alpha).astype(f)
        cdf = np.cumsum(alpha, axis=1, dtype=f) - alpha
        gamma = (np.concatenate([np.ones((1, J), f), cdf[:-1]]) - cdf).astype(f)
    bnd = np.zeros(I, np.int32)
    score = f(NEG)
    if np.isfinite(de_prev[J]):
        score = de_prev[J] * f(LN2)
        j = J
        for i in range(I - 1, -1, -1):
            bnd[i] = j
            j = int(np.clip(back[i, j], 0, J))
    dur = np.diff(np.concatenate([[0], bnd])).astype(np.int32)
    if not np.isfinite(de_prev[J]):
        dur[:] = 0
    return dict(log_alpha=log_alpha, gamma=gamma, boundaries=bnd, durations=dur, map_score=float(score))


def batch32(name, sabotage=None):
    """boundary_search32 on every utterance of a named case, laid out as the GPU path lays its results out."""
    c = case(name)
    e = energies(name)
    D = min(c.D, c.Ty)
    la = np.full((c.B, c.Tx, c.Ty), NEG, np.float32)
    ga = np.zeros((c.B, c.Tx, c.Ty), np.float32)
    bnd = np.zeros((c.B, c.Tx), np.int32)
    dur = np.zeros((c.B, c.Tx), np.int32)
    sc = np.full(c.B, NEG, np.float32)
    for b in range(c.B):
        I, J, ok = clamped_lengths(c, b)
        if not ok:
            continue
        r = boundary_search32(e[b, :I, :J], D, sabotage)
        la[b, :I, :J], ga[b, :I, :J] = r["log_alpha"], r["gamma"]
        sc[b] = r["map_score"]
        if np.isfinite(sc[b]):
            bnd[b, :I], dur[b, :I] = r["boundaries"], r["durations"]
            bnd[b, I:] = J
    return dict(log_alpha=la, gamma=ga, boundaries=bnd, durations=dur, map_score=sc)
