"""Forward-sum kernels on sharp, masked and degenerate log-probs, and at every dispatch edge.

tests/test_objective.py feeds the forward-sum kernels one distribution (Gaussian noise x 3 through a log-softmax:
log-probs of -1 .. -15, every column like every other).  The kernels' numerical machinery -- drift estimate, re-basing
into double offsets, one offset per 63-row wave, ghost-row conversion, the all-log-0 column rule, the clamp of -inf to
FS_NEG -- exists for inputs that distribution never produces.  This module holds

  * FAMILIES: seeded, pure-numpy generators of such inputs (tools/soak_objective.py imports them too);
  * CPU tests of the yardsticks: the float64 oracle's structure, and a float32 restatement of the documented scheme
    (oracle/forward_sum_fp32.py) which says what float32 can resolve on a given input;
  * GPU tests of aligner_amd.forward_sum against the float64 oracle on every family, kernel form and dispatch edge.

Tolerance of the GPU tests: the project's (loss 5e-4 + 2e-7 |loss|, gradient 1e-3 |g| + 2e-5; CTC form: loss
5e-4 + 1e-6 |loss|, gradient 5e-3 occupancy + 2e-5) times a per-case scale s = max(1, 3 r), where r is the float32
restatement's own error on that very input in units of the project's tolerance.  The 3 covers: hardware exp2 / log2 are
good to ~1 ulp where numpy rounds correctly; the kernels group their sums differently (per-wave offsets, drift); the one
documented data point (tools/soak_objective.py, scale 8 at [643,663]) has the kernel at 3.6x where the restatement gives
2.0x.  s is capped at S_CAP = 10: a family member that needs more is replaced by a milder one (DESIGN.md 5.2 lists them).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import forward_sum_fp32 as F32R
from oracle import forward_sum_oracle as FS

S_CAP = 10.0
MARGIN = 3.0
CU_COUNT = 256          # MI355X; the side-by-side form runs while 2 B <= the CU count (aligner_amd.h)


# --------------------------------------------------------------------------- the input families
def _log_softmax(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        m = z.max(axis=-2, keepdims=True)
        return z - (m + np.log(np.exp(z - m).sum(axis=-2, keepdims=True)))


def ragged_lengths(rng, B, Tx, Ty):
    """t_x <= t_y per utterance, the first utterance full-size (the rule of tests/test_objective.py)."""
    ty = rng.integers(max(Tx // 2, 2), Ty + 1, size=B) if Ty >= 2 else np.full(B, Ty)
    tx = np.minimum(rng.integers(1, Tx + 1, size=B), ty)
    tx[0], ty[0] = Tx, Ty
    return tx.astype(np.int64), ty.astype(np.int64)


def _ridge(tx, ty, Tx, Ty):
    """centre[y] of the diagonal x = (tx-1) y / (ty-1), and the row index column."""
    y = np.arange(Ty, dtype=np.float64)
    return (tx - 1) * np.minimum(y, ty - 1) / max(ty - 1, 1), np.arange(Tx, dtype=np.float64)[:, None]


def _gauss(rng, tx, ty, Tx, Ty, scale):
    return _log_softmax(rng.standard_normal((Tx, Ty)) * scale)


def _diag(rng, tx, ty, Tx, Ty, w, depth, step=1):
    c, x = _ridge(tx, ty, Tx, Ty)
    if step > 1:
        c = step * np.floor(c / step)                        # the ridge advances `step` tokens at a time
    z = -np.minimum(((x - c[None, :]) / w) ** 2, 1.0) * depth + rng.standard_normal((Tx, Ty))
    return _log_softmax(z)


def _stuck(rng, tx, ty, Tx, Ty, depth):
    z = rng.standard_normal((Tx, Ty))
    z[0] += depth                                            # collapsed attention: every frame looks at token 0
    return _log_softmax(z)


def _level(rng, tx, ty, Tx, Ty, drop):
    z = _log_softmax(rng.standard_normal((Tx, Ty)))
    z[:, ty // 3:(2 * ty) // 3] -= drop                      # unnormalised: legal for the plain form
    return z


def _band(rng, tx, ty, Tx, Ty, half):
    c, x = _ridge(tx, ty, Tx, Ty)
    z = rng.standard_normal((Tx, Ty)) * 3.0
    z[np.abs(x - c[None, :]) > half] = -np.inf               # floor(c) is still a monotonic path (slope <= 1)
    return _log_softmax(z)


# name -> (generator, keyword arguments).  `finite`: no -inf anywhere (the CTC form's oracle, torch's ctc_loss, returns
# NaN gradients for -inf inside the valid block).  `plain_tol`: the float32 restatement stays within 0.6 of the project's
# tolerance on it, so the kernels are held to the plain tolerance (s = 1).
STUCK_DEEP = 60     # deepest of 150 / 100 / 80 / 60 whose s = 3 r stays under S_CAP over the shape list
FAMILIES = {
    "gauss3": (_gauss, dict(scale=3.0)),
    "gauss8": (_gauss, dict(scale=8.0)),
    "diag_w3_d150": (_diag, dict(w=3.0, depth=150.0)),
    "diag_w8_d40": (_diag, dict(w=8.0, depth=40.0)),
    "jumps_d60": (_diag, dict(w=3.0, depth=60.0, step=7)),
    "stuck_d10": (_stuck, dict(depth=10.0)),
    "stuck_d40": (_stuck, dict(depth=40.0)),
    f"stuck_d{STUCK_DEEP}": (_stuck, dict(depth=float(STUCK_DEEP))),
    "level_80": (_level, dict(drop=80.0)),
    "level_up_80": (_level, dict(drop=-80.0)),    # RAISED: the column maximum climbs 115 bits a frame, past any cap on the drift
    "band_12": (_band, dict(half=12.0)),
}
PLAIN_TOL = ("gauss3", "diag_w3_d150", "diag_w8_d40", "jumps_d60", "level_80", "level_up_80", "band_12")
EARNED_TOL = ("gauss8", "stuck_d10", "stuck_d40", f"stuck_d{STUCK_DEEP}")
FINITE = ("gauss8", "diag_w3_d150", "diag_w8_d40", "jumps_d60", "stuck_d10", "stuck_d40", f"stuck_d{STUCK_DEEP}")


def _seed(name, B, Tx, Ty):
    return [sum(map(ord, name)), B, Tx, Ty]


def make(name, B, Tx, Ty, lengths=None, seed=None):
    """(logp[B,Tx,Ty] float32, t_x[B], t_y[B]) of a family; `lengths` = (t_x, t_y) arrays instead of the ragged draw."""
    rng = np.random.default_rng(_seed(name, B, Tx, Ty) if seed is None else seed)
    tx, ty = ragged_lengths(rng, B, Tx, Ty) if lengths is None else (np.asarray(lengths[0]), np.asarray(lengths[1]))
    gen, kw = FAMILIES[name]
    lp = np.stack([gen(rng, int(tx[b]), int(ty[b]), Tx, Ty, **kw) for b in range(B)]).astype(np.float32)
    return lp, tx, ty


def make_blocked(B, Tx, Ty, blocked, seed=0):
    """gauss3 with, for the utterances in `blocked`, one frame whose valid rows are all -inf (t_x <= t_y all the same):
    (logp with the blocks, the same batch without them, t_x, t_y)."""
    plain, tx, ty = make("gauss3", B, Tx, Ty, seed=[seed, B, Tx, Ty])
    lp = plain.copy()
    for b in blocked:
        lp[b, :tx[b], (int(ty[b]) * (1 + b % 3)) // 4] = -np.inf
    return lp, plain, tx, ty


def pipeline_like(B, Tx, Ty, temperature, prior, kq=3.0, seed=0, C=80):
    """What soft_attention() hands the objective, restated in numpy for the CPU tests: log-softmax over the valid text rows
    of -temperature |q - k|^2 (k, q: kq x Gaussian; tests/test_softattn_gpu.py draws them at 3), -inf in rows >= t_x, plus
    log(prior + 1e-8) of the beta-binomial prior if asked."""
    rng = np.random.default_rng([seed, B, Tx, Ty])
    tx, ty = ragged_lengths(rng, B, Tx, Ty)
    k = rng.standard_normal((B, C, Tx)) * kq
    q = rng.standard_normal((B, C, Ty)) * kq
    d = (k ** 2).sum(1)[:, :, None] + (q ** 2).sum(1)[:, None, :] - 2.0 * np.einsum("bci,bcj->bij", k, q)
    z = -temperature * d
    for b in range(B):
        z[b, tx[b]:] = -np.inf
    lp = _log_softmax(z)
    if prior:
        from scipy.stats import betabinom
        for b in range(B):
            n, m = int(tx[b]), int(ty[b])
            y = np.arange(m)
            pr = np.zeros((Tx, Ty))
            pr[:n, :m] = betabinom.pmf(np.arange(n)[:, None], n, (y + 1.0)[None, :], (m - y + 0.0)[None, :])
            lp[b] = lp[b] + np.log(pr + 1e-8)
    return lp.astype(np.float32), tx, ty


# (temperature, prior, scale of the random k and q).  At temperature 0.05 the logits of 3 x Gaussian encodings have a
# spread of ~11 with no structure along time -- Gaussian noise x 11, past gauss8: the float32 restatement itself is at 1.9x
# the tolerance at [504,1100] -- so WITHOUT the prior that member draws k and q at 1.25 (a spread of ~2, |logp| to ~20);
# with the prior (which puts the ridge near the diagonal) it stays at 3 and |logp| reaches ~150.
PIPELINE = [(0.0005, False, 3.0), (0.0005, True, 3.0), (0.05, False, 1.25), (0.05, True, 3.0)]


# --------------------------------------------------------------------------- error in units of the project's tolerance
def tol_units(loss, grad, want_loss, want_grad):
    """(loss error, gradient error) in units of the plain form's tolerance; utterances without an alignment (oracle loss
    +inf) must have loss +inf -- an error of inf otherwise."""
    fin = np.isfinite(want_loss)
    el = 0.0
    if fin.any():
        el = float((np.abs(loss[fin] - want_loss[fin]) / (5e-4 + 2e-7 * np.abs(want_loss[fin]))).max())
    if not np.array_equal(np.isposinf(loss), ~fin):
        el = np.inf
    eg = float((np.abs(grad - want_grad) / (1e-3 * np.abs(want_grad) + 2e-5)).max())
    return el, eg


def restatement_error(lp, tx, ty, want_loss, want_grad):
    return max(tol_units(*F32R.forward_sum(lp, tx, ty), want_loss, want_grad))


def scale_of(r, name):
    """s of a case: 1 for the families the restatement resolves (PLAIN_TOL, the pipeline, blocked); gauss8 and stuck earn
    max(1, 3 r)."""
    return max(1.0, MARGIN * r) if name in EARNED_TOL else 1.0


def trapezoid(Tx, Ty, tx, ty):
    """reachable[x, y]: cells some monotonic alignment of (tx, ty) passes (x <= y and tx-1-x <= ty-1-y, inside the block)."""
    x, y = np.arange(Tx)[:, None], np.arange(Ty)[None, :]
    return (x < tx) & (y < ty) & (x <= y) & (tx - 1 - x <= ty - 1 - y)


# --------------------------------------------------------------------------- the shape lists, and the dispatch rule
# (B, T_text, T_mel).  MAIN: every family, every form.  EDGES: wave boundaries (63 rows per wave) and dispatch thresholds.
# stuck: the restatement's error grows with depth x T_text (the only paths to the last token run that far below the column
# maximum, where a float32 has few fraction bits left), so its members run where s = 3 r stays under S_CAP: the four- and
# eight-wave shapes below and the forced one-wave kernel on them; depth 10 also on a natural one-wave shape.
MAIN_SHAPES = [(2, 200, 1000), (2, 400, 700), (1, 600, 1000)]
STUCK_SHAPES = [(2, 200, 1000), (2, 260, 1000)]
SOAK_HARD_CASE = ("gauss8", 1, 643, 663)                     # tools/soak_objective.py's documented worst: near-square, one wave


def shapes_of(fam):
    if fam.startswith("stuck"):
        return STUCK_SHAPES + ([(1, 520, 1100)] if fam == "stuck_d10" else [])
    return MAIN_SHAPES + ([SOAK_HARD_CASE[1:]] if fam == "gauss8" else [])


EDGE_SHAPES = [(2, 63, 150), (2, 64, 150), (2, 252, 300), (2, 253, 300), (2, 256, 300), (2, 257, 300), (2, 504, 560),
               (2, 505, 560), (1, 512, 560), (1, 513, 560), (1, 1024, 1100)]
EDGE_FAMILIES = ("gauss8", "diag_w3_d150", "band_12")
CTC_EDGE_SHAPES = [(2, 62, 150), (2, 63, 150), (2, 251, 300), (2, 252, 300), (2, 255, 300), (2, 256, 300), (2, 503, 560),
                   (2, 504, 560), (1, 511, 560), (1, 512, 560), (1, 1023, 1200)]    # (gauss8 at [1023,1100]: r = 5.3, past the cap)
CTC_EDGE_FAMILIES = ("gauss8", "diag_w3_d150")
SMALL_T_MEL = [1, 2, 7, 8, 9, 15, 16, 17]
BENCH_SHAPE = (64, 200, 1000)
BIG_BATCH = (130, 20, 64)                                    # past half the CU count: the serial form, whatever is asked
FORMS = ("sys", "sys_serial", "one_wave", "one_wave_serial")


def bucket(B, Tx, form, ctc=False):
    """The kernel a call lands on, from the public limits only (aligner_amd.h, tests/test_objective.py): rows = T_text
    (+ 1 in the CTC form: the blank after the last token); <= 252 rows four waves, <= 504 eight, else one wave with
    R = 4 / 8 / 16 rows per lane for <= 256 / 512 / 1024 rows; `fwdsum_one_wave` forces the latter; the systolic kernels run
    both sweeps side by side while 2 B <= the CU count unless `fwdsum_serial`.  None: no such call (refused, or the form
    asks for what the shape already is)."""
    rows = Tx + 1 if ctc else Tx
    if rows > 1024:
        return None
    one = form.startswith("one_wave")
    if rows > 504 and not one:
        return None                                          # (listed under one_wave)
    if one:
        if form == "one_wave_serial":
            return None                                      # the one-wave kernels have one form
        return ("one_wave", 4 if rows <= 256 else 8 if rows <= 512 else 16)
    return ("four_wave" if rows <= 252 else "eight_wave", "side_by_side" if form == "sys" and 2 * B <= CU_COUNT else "serial")


ALL_BUCKETS = {("one_wave", 4), ("one_wave", 8), ("one_wave", 16), ("four_wave", "side_by_side"), ("four_wave", "serial"),
               ("eight_wave", "side_by_side"), ("eight_wave", "serial")}


def _forms_of(B, Tx, ctc=False):
    return [f for f in FORMS if bucket(B, Tx, f, ctc) is not None]


def _cases(shapes, families, ctc=False):
    return [(fam, B, Tx, Ty, form) for fam in families for (B, Tx, Ty) in (shapes or shapes_of(fam))
            for form in _forms_of(B, Tx, ctc)]


GPU_FAMILIES = [f for f in FAMILIES if f != "gauss3"]        # (gauss3 is tests/test_objective.py's own input)
PLAIN_CASES = (_cases(None, GPU_FAMILIES) + _cases(EDGE_SHAPES, EDGE_FAMILIES) +
               _cases([BENCH_SHAPE], ["jumps_d60"]) + _cases([BIG_BATCH], ["gauss8", "band_12"]))
CTC_CASES = _cases(None, FINITE, ctc=True) + _cases(CTC_EDGE_SHAPES, CTC_EDGE_FAMILIES, ctc=True)


# --------------------------------------------------------------------------- CPU: the yardsticks
def test_restatement_equals_the_oracle_on_easy_input_and_brute_force():
    rng = np.random.default_rng(0)
    tx, ty = 3, 6
    lp = _gauss(rng, tx, ty, tx, ty, 3.0).astype(np.float32)
    total, occ = 0.0, np.zeros((tx, ty))
    for adv in itertools.combinations(range(1, ty), tx - 1):          # a monotonic alignment = the frames it advances at
        x, w, cells = 0, 0.0, []
        for y in range(ty):
            x += y in adv
            w += float(lp[x, y])
            cells.append((x, y))
        total += np.exp(w)
        for c in cells:
            occ[c] += np.exp(w)
    lz, post = F32R.forward_sum_one(lp, tx, ty)
    assert abs(lz - np.log(total)) < 1e-6 and np.abs(post - occ / total).max() < 1e-6
    # tiny inputs (|log Z| of a few units: one float32 rounding there is ~2e-7): the oracle to 1e-6
    for (B, Tx, Ty) in [(3, 3, 4), (2, 1, 3), (2, 3, 3), (3, 2, 4)]:
        txs, tys = ragged_lengths(rng, B, Tx, Ty)
        lp = np.stack([_gauss(rng, 0, 0, Tx, Ty, 1.0) for _ in range(B)]).astype(np.float32)
        wl, wg = FS.forward_sum(lp, txs, tys)
        gl, gg = F32R.forward_sum(lp, txs, tys)
        assert np.abs(gl - wl).max() < 1e-6 and np.abs(gg - wg).max() < 1e-6
    # degenerate lengths and a blocked utterance: no alignment, as the oracle says
    lp, plain, txs, tys = make_blocked(3, 6, 11, blocked=[1])
    wl, wg = FS.forward_sum(lp, txs, tys)
    gl, gg = F32R.forward_sum(lp, txs, tys)
    assert np.isposinf(wl[1]) and not wg[1].any() and np.isposinf(gl[1]) and not gg[1].any()
    assert np.isfinite(wl[[0, 2]]).all() and np.abs(gl[[0, 2]] - wl[[0, 2]]).max() < 1e-5
    assert F32R.forward_sum_one(np.zeros((4, 3), np.float32), 4, 3)[0] == -np.inf


YARD_SHAPES = [(1, 200, 1000, None), (1, 200, 1000, (120, 777)), (1, 504, 1100, None)]


def _yard_input(name, B, Tx, Ty, lengths):
    ln = None if lengths is None else (np.array([lengths[0]]), np.array([lengths[1]]))
    if name.startswith("pipeline"):
        lp, tx, ty = pipeline_like(B, Tx, Ty, *PIPELINE[int(name[-1])])
        if ln is not None:
            tx, ty = ln                                      # (rows the attention saw stay valid: t_x only shrinks)
            tx = np.minimum(tx, Tx)
        return lp, tx, ty
    return make(name, B, Tx, Ty, lengths=ln)


@functools.lru_cache(maxsize=None)
def _yard(name, B, Tx, Ty, lengths):
    lp, tx, ty = _yard_input(name, B, Tx, Ty, lengths)
    wl, wg = FS.forward_sum(lp, tx, ty)
    return lp, tx, ty, wl, wg, restatement_error(lp, tx, ty, wl, wg)


@pytest.mark.parametrize("name", list(PLAIN_TOL) + [f"pipeline{i}" for i in range(len(PIPELINE))])
def test_yardstick_stays_within_the_plain_tolerance(name):
    """The float32 restatement's error, in units of the project's tolerance, is <= 0.6 on every family that the GPU tests
    hold to the plain tolerance: float32 itself leaves room there, so s = 1 asks nothing impossible of the kernels."""
    for (B, Tx, Ty, lengths) in YARD_SHAPES:
        r = _yard(name, B, Tx, Ty, lengths)[-1]
        print(f"yardstick {name} [{Tx},{Ty}] lengths={lengths}: r = {r:.3f}")
        assert r <= 0.6, (name, Tx, Ty, lengths, r)


@pytest.mark.parametrize("name", EARNED_TOL)
def test_yardstick_of_the_hard_families_stays_under_the_cap(name):
    """gauss8 and stuck earn a scale s = 3 r; a member whose s would pass S_CAP on a shape the GPU tests use is not in the
    list (stuck at depth 150 / 100 / 80: replaced by STUCK_DEEP)."""
    for (B, Tx, Ty) in shapes_of(name):
        lp, tx, ty = make(name, B, Tx, Ty)
        wl, wg = FS.forward_sum(lp, tx, ty)
        r = restatement_error(lp, tx, ty, wl, wg)
        print(f"yardstick {name} [{B},{Tx},{Ty}]: r = {r:.3f}, s = {scale_of(r, name):.2f}")
        assert scale_of(r, name) <= S_CAP, (name, Tx, Ty, r)


@pytest.mark.parametrize("name", [f for f in FAMILIES] + ["pipeline1", "pipeline2", "blocked"])
def test_oracle_posterior_is_a_distribution_on_the_reachable_trapezoid(name):
    """What the GPU structural checks rest on: per valid frame the oracle's posterior sums to 1, and it is EXACTLY 0
    outside the reachable trapezoid (and everywhere for an utterance without an alignment)."""
    B, Tx, Ty = 3, 40, 130
    if name == "blocked":
        lp, _, tx, ty = make_blocked(B, Tx, Ty, blocked=[1])
    elif name.startswith("pipeline"):
        lp, tx, ty = pipeline_like(B, Tx, Ty, *PIPELINE[int(name[-1])])
    else:
        lp, tx, ty = make(name, B, Tx, Ty)
    assert tx[0] == Tx and ty[0] == Ty and (tx <= ty).all() and lp.dtype == np.float32 and lp.shape == (B, Tx, Ty)
    loss, grad = FS.forward_sum(lp, tx, ty)
    for b in range(B):
        reach = trapezoid(Tx, Ty, int(tx[b]), int(ty[b]))
        assert not grad[b][~reach].any()
        if name == "blocked" and b == 1:
            assert np.isposinf(loss[b]) and not grad[b].any()
        else:
            assert np.isfinite(loss[b]) and np.allclose(-grad[b, :, :ty[b]].sum(axis=0), 1.0, atol=1e-9)


def test_families_are_seeded_and_have_the_advertised_features():
    a, b = make("jumps_d60", 2, 50, 120), make("jumps_d60", 2, 50, 120)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    lp, tx, ty = make("band_12", 2, 100, 300)
    assert np.isneginf(lp[0]).any() and np.isfinite(FS.forward_sum(lp, tx, ty)[0]).all()      # -inf inside, a path left
    lp, tx, ty = make("diag_w3_d150", 1, 100, 300)
    assert lp.min() < -140 and np.exp(lp.astype(np.float64)).sum(1).max() < 1 + 1e-6          # sharp and normalised
    lp, tx, ty = make("jumps_d60", 1, 100, 300)
    assert np.diff(lp[0].argmax(axis=0)).max() >= 5                                            # the peak is no path
    lp, tx, ty = make(f"stuck_d{STUCK_DEEP}", 1, 100, 300)
    assert (lp[0].argmax(axis=0) == 0).all()
    lp, tx, ty = make("level_80", 1, 100, 300)
    assert lp[0, :, 150].max() < -80 < lp[0, :, 10].min() - 60
    lp, tx, ty = make("level_up_80", 1, 100, 300)
    assert lp[0, :, 150].min() > 60 and lp[0, :, 10].max() <= 0
    lp, tx, ty = pipeline_like(2, 60, 200, 0.05, True)
    assert np.isneginf(lp[1, tx[1]:]).all() and np.isfinite(lp[1, :tx[1]]).all() and lp[np.isfinite(lp)].min() < -50


def test_shape_lists_reach_every_dispatch_bucket_and_edge():
    """A later edit of the lists cannot silently drop a kernel form or a boundary."""
    for ctc, cases in ((False, PLAIN_CASES), (True, CTC_CASES)):
        seen = {bucket(B, Tx, form, ctc) for (_, B, Tx, _, form) in cases}
        assert seen == ALL_BUCKETS, (ctc, ALL_BUCKETS - seen)
        rows = {Tx + ctc for (_, _, Tx, _, _) in cases}
        assert {63, 64, 252, 253, 256, 257, 504, 505, 512, 513, 1024} <= rows, ctc
        # both sides of each one-wave width actually run on the one-wave kernel
        one = {Tx + ctc for (_, _, Tx, _, form) in cases if form == "one_wave"}
        assert {256, 257, 512, 513, 1024} <= one, ctc
        for fam in (FINITE if ctc else GPU_FAMILIES):         # (a natural 16-rows-per-lane shape is past what stuck resolves)
            need = ALL_BUCKETS - ({("one_wave", 16)} if fam.startswith("stuck") and fam != "stuck_d10" else set())
            assert {bucket(B, Tx, form, ctc) for (f, B, Tx, _, form) in cases if f == fam} >= need, fam
    assert bucket(1, 1025, "sys") is None and bucket(1, 1024, "one_wave", ctc=True) is None
    assert bucket(*BIG_BATCH[:2], "sys") == ("four_wave", "serial") and bucket(*BENCH_SHAPE[:2], "sys") == ("four_wave", "side_by_side")
    assert len([f for f in FAMILIES if f.startswith("stuck")]) == 3 and set(PLAIN_TOL) | set(EARNED_TOL) == set(FAMILIES)


# --------------------------------------------------------------------------- HIP path (GPU)
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import aligner_amd  # noqa: F401
    from aligner_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _set_form(request, form):
    from aligner_amd import _lib
    lib = _lib.load()
    request.addfinalizer(lambda: (lib.aligner_debug_set_option(b"fwdsum_one_wave", 0),
                                  lib.aligner_debug_set_option(b"fwdsum_serial", 0)))
    _lib.check(lib.aligner_debug_set_option(b"fwdsum_one_wave", 1 if form.startswith("one_wave") else 0))
    _lib.check(lib.aligner_debug_set_option(b"fwdsum_serial", 1 if form.endswith("serial") else 0))


def _run(dev, lp, tx, ty, blank=None, want_grad=True):
    import aligner_amd
    lp_d = lp if isinstance(lp, torch.Tensor) else torch.from_numpy(lp).to(dev)
    loss, grad = aligner_amd.forward_sum(lp_d, torch.from_numpy(np.asarray(tx)), torch.from_numpy(np.asarray(ty)),
                                         want_grad=want_grad, blank_logprob=blank)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), None if grad is None else grad.cpu().numpy()


@functools.lru_cache(maxsize=8)
def _reference(fam, B, Tx, Ty):
    """(input, oracle, restatement error r) of a case: the same for every kernel form, worked out once."""
    lp, tx, ty = make(fam, B, Tx, Ty)
    wl, wg = FS.forward_sum(lp, tx, ty)
    return lp, tx, ty, wl, wg, restatement_error(lp, tx, ty, wl, wg)


def _check_plain(tag, form, lp, tx, ty, wl, wg, r, loss, grad, loss2, grad2):
    """Everything a plain-form case asserts; prints the figures first (DESIGN.md 5.2 is made of these lines)."""
    B, Tx, Ty = lp.shape
    s = scale_of(r, tag)
    el, eg = tol_units(loss.astype(np.float64), grad.astype(np.float64), wl, wg)
    print(f"FSFIG plain {tag} [{B},{Tx},{Ty}] {form}: r = {r:.3f}  s = {s:.2f}  kernel loss {el:.3f}  grad {eg:.3f}")
    assert s <= S_CAP, "the case needs a milder parameter (DESIGN.md 5.2)"
    assert tag in EARNED_TOL or r <= 0.6, "a plain-tolerance case on which float32 itself has no room: change its parameters"
    assert np.isfinite(grad).all() and np.array_equal(np.isfinite(loss), np.isfinite(wl))
    assert el <= s and eg <= s, (tag, form, el, eg, s)
    for b in range(B):
        reach = trapezoid(Tx, Ty, int(tx[b]), int(ty[b]))
        assert not grad[b][~reach].any(), (tag, form, b, "gradient outside the reachable trapezoid / in the padding")
        if np.isfinite(wl[b]):
            assert np.abs(-grad[b, :, :ty[b]].astype(np.float64).sum(axis=0) - 1.0).max() <= s * 1e-3, (tag, form, b)
    assert np.array_equal(loss.view(np.int32), loss2.view(np.int32)) and np.array_equal(grad.view(np.int32), grad2.view(np.int32))


@gpu
@pytest.mark.parametrize("fam,B,Tx,Ty,form", PLAIN_CASES)
def test_forward_sum_families_match_the_oracle(dev, request, fam, B, Tx, Ty, form):
    if 2 * B > CU_COUNT:                                     # the big batch must really be past half of THIS device's CUs
        assert 2 * B > torch.cuda.get_device_properties(dev).multi_processor_count
    lp, tx, ty, wl, wg, r = _reference(fam, B, Tx, Ty)
    _set_form(request, form)
    loss, grad = _run(dev, lp, tx, ty)
    loss2, grad2 = _run(dev, lp, tx, ty)
    _check_plain(fam, form, lp, tx, ty, wl, wg, r, loss, grad, loss2, grad2)   # (the oracle on EVERY utterance)


@gpu
@pytest.mark.parametrize("form", ["sys", "sys_serial", "one_wave"])
@pytest.mark.parametrize("fam", ["gauss8", "diag_w3_d150"])
@pytest.mark.parametrize("Ty", SMALL_T_MEL)
def test_forward_sum_on_fewer_frames_than_a_tile(dev, request, fam, Ty, form):
    """T_mel below one tile (16 frames) and below one re-basing group (8): t_x = t_y (one path), t_x = 1 (one path),
    and something between."""
    tx, ty = np.array([Ty, 1, max(Ty // 2, 1)]), np.array([Ty, Ty, Ty])
    lp, _, _ = make(fam, 3, Ty, Ty, lengths=(tx, ty))
    wl, wg = FS.forward_sum(lp, tx, ty)
    r = restatement_error(lp, tx, ty, wl, wg)
    _set_form(request, form)
    loss, grad = _run(dev, lp, tx, ty)
    loss2, grad2 = _run(dev, lp, tx, ty)
    _check_plain(fam, form, lp, tx, ty, wl, wg, r, loss, grad, loss2, grad2)


@gpu
@pytest.mark.parametrize("fam,B,Tx,Ty", [(f, *sh) for f in GPU_FAMILIES for sh in shapes_of(f) if sh[1] <= 504])
def test_families_side_by_side_sweeps_equal_the_serial_form(dev, request, fam, B, Tx, Ty):
    """The rule of test_objective.py::test_forward_sum_side_by_side_sweeps_equal_the_serial_form, on every family: the same
    loss bits, and gradients within 2e-4 |g| + 2e-6 -- for the stuck members times the case's s, which LOOSENS the rule
    there.  (The rule is one float32 rounding of the exponent's sum at |alpha| ~ 300 below the wave's column maximum;
    collapsed attention keeps its posterior thousands of units below it, which is what r measures.  Measured on an MI355X:
    stuck d40 / d60 0.84 .. 2.1 x the rule against s = 5.5 .. 8; every other family, gauss8 included, <= 0.6 x.)"""
    lp, tx, ty, wl, wg, r = _reference(fam, B, Tx, Ty)
    s = scale_of(r, fam) if fam.startswith("stuck") else 1.0
    _set_form(request, "sys_serial")
    loss_s, grad_s = _run(dev, lp, tx, ty)
    _set_form(request, "sys")
    loss_p, grad_p = _run(dev, lp, tx, ty)
    assert np.array_equal(loss_s.view(np.int32), loss_p.view(np.int32))
    u = float((np.abs(grad_s.astype(np.float64) - grad_p) / (2e-4 * np.abs(grad_s) + 2e-6)).max())
    print(f"FSFIG forms {fam} [{B},{Tx},{Ty}]: |serial - side by side| = {u:.3f} x (2e-4 |g| + 2e-6), s = {s:.2f}")
    assert u <= s


def _pipeline_input(dev, B, Tx, Ty, temperature, prior, kq, C=80):
    import aligner_amd
    rng = np.random.default_rng([int(temperature * 1e4), int(prior), B, Tx, Ty])
    tx, ty = ragged_lengths(rng, B, Tx, Ty)
    k = torch.from_numpy((rng.standard_normal((B, C, Tx)) * kq).astype(np.float32)).to(dev)
    q = torch.from_numpy((rng.standard_normal((B, C, Ty)) * kq).astype(np.float32)).to(dev)
    tx_d, ty_d = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    pr = aligner_amd.beta_binomial_prior(tx_d, ty_d, Tx, Ty) if prior else None
    lp_d, _ = aligner_amd.soft_attention(k, q, t_x=tx_d, prior=pr, temperature=temperature)
    torch.cuda.synchronize()
    return lp_d, tx, ty


@gpu
@pytest.mark.parametrize("temperature,prior,kq", PIPELINE)
@pytest.mark.parametrize("B,Tx,Ty", [(3, 200, 1000), (2, 400, 700), (1, 600, 1000)])
def test_forward_sum_on_the_projects_own_attention(dev, request, B, Tx, Ty, temperature, prior, kq):
    """soft_attention() -> forward_sum(): the log-probs the objective really gets (-inf in rows >= t_x, |logp| of ~150 at
    the sharper temperature), on every kernel form; the oracle runs on the same log-probs copied to the host.  Both forms
    of the objective, the CTC form at blank -1 and -6 on every shape (four waves, eight waves and the one-wave kernel
    all see the -inf padding rows: they lie outside the valid block, which torch's ctc_loss accepts)."""
    lp_d, tx, ty = _pipeline_input(dev, B, Tx, Ty, temperature, prior, kq)
    lp = lp_d.cpu().numpy()
    for b in range(B):
        assert np.isneginf(lp[b, tx[b]:]).all() and np.isfinite(lp[b, :tx[b]]).all()
    wl, wg = FS.forward_sum(lp, tx, ty)
    r = restatement_error(lp, tx, ty, wl, wg)
    tag = f"pipeline_T{temperature}_{'prior' if prior else 'noprior'}"
    for form in _forms_of(B, Tx):
        _set_form(request, form)
        loss, grad = _run(dev, lp_d, tx, ty)
        loss2, grad2 = _run(dev, lp_d, tx, ty)
        _check_plain(tag, form, lp, tx, ty, wl, wg, r, loss, grad, loss2, grad2)
    for blank in (-1.0, -6.0):
        cl, cg = FS.ctc_forward_sum(np.where(np.isfinite(lp), lp, 0.0), tx, ty, blank)  # (rows >= t_x are not read)
        for form in _forms_of(B, Tx, ctc=True):
            _set_form(request, form)
            loss, grad = _run(dev, lp_d, tx, ty, blank=blank)
            _check_ctc(tag, form, lp, tx, ty, blank, cl, cg, r, loss, grad)


def _check_ctc(tag, form, x, tx, ty, blank, wl, wg, r, loss, grad):
    """The CTC form's existing tolerance (tests/test_objective.py) times the same s."""
    B, Tx, Ty = x.shape
    s = scale_of(r, tag)
    loss, grad = loss.astype(np.float64), grad.astype(np.float64)
    el = float((np.abs(loss - wl) / (5e-4 + 1e-6 * np.abs(wl))).max())
    eg = ec = 0.0
    for b in range(B):
        K, T = int(tx[b]), int(ty[b])
        z = np.concatenate([np.full((1, T), blank), x[b, :K, :T].astype(np.float64)], 0)
        occ = _log_softmax_exp(z)[1:] - wg[b, :K, :T]
        assert occ.min() > -1e-9
        eg = max(eg, float((np.abs(grad[b, :K, :T] - wg[b, :K, :T]) / (5e-3 * np.maximum(occ, 0.0) + 2e-5)).max()))
        assert not grad[b, K:].any() and not grad[b, :, T:].any(), (tag, form, b)
        ec = max(ec, float(np.abs(grad[b, :K, :T].sum(axis=0)).max()) - 1.0)
    print(f"FSFIG ctc{blank:g} {tag} [{B},{Tx},{Ty}] {form}: r = {r:.3f}  s = {s:.2f}  kernel loss {el:.3f}  grad {eg:.3f}"
          f"  max |column sum| - 1 = {ec:.2e}")
    assert s <= S_CAP
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    assert el <= s and eg <= s, (tag, form, el, eg, s)
    # per frame: softmax mass of the text rows minus the tokens' occupancy = occupancy(blank) - softmax(blank), in [-1, 1].
    # The tokens' occupancies sum to <= 1 and each is allowed a relative error of s x 5e-3 above, so their sum is held to
    # that too (a COMMON error of all rows -- a wrong offset or log Z -- shows here at 5e-3 where the rows' own bound,
    # summed, would let 5e-3 + t_x x 2e-5 pass; tests/test_objective.py holds its gentle input to 1e-3).
    assert ec < s * 5e-3, (tag, form, ec)


def _log_softmax_exp(z):
    return np.exp(_log_softmax(z))


@functools.lru_cache(maxsize=4)
def _ctc_reference(fam, B, Tx, Ty, blank):
    x, tx, ty, _, _, r = _reference(fam, B, Tx, Ty)         # the same s as the plain form earns on this input
    cl, cg = FS.ctc_forward_sum(x, tx, ty, blank)
    return x, tx, ty, cl, cg, r


@gpu
@pytest.mark.parametrize("blank", [-1.0, -6.0])
@pytest.mark.parametrize("fam,B,Tx,Ty,form", CTC_CASES)
def test_forward_sum_ctc_form_families_match_torch_ctc_loss(dev, request, fam, B, Tx, Ty, form, blank):
    """The CTC form on the finite families against torch's ctc_loss, its tolerance of tests/test_objective.py times the s
    the input earns.

    These cases found the one-wave CTC kernels' float32 states wanting: with one offset per
    frame a state thousands of bits below the column maximum gets the same addend every frame and every add rounds the
    same way -- stuck d40 / d60 came out at 8 .. 56 units of gradient error against s = 5.5 .. 8, jumps_d60 at 1.03 .. 2.8
    and gauss8 [1,600,1000], blank -6, at 1.64 against s = 1.  Those kernels now keep their states in float64."""
    x, tx, ty, cl, cg, r = _ctc_reference(fam, B, Tx, Ty, blank)
    _set_form(request, form)
    loss, grad = _run(dev, x, tx, ty, blank=blank)
    loss2, grad2 = _run(dev, x, tx, ty, blank=blank)
    _check_ctc(fam, form, x, tx, ty, blank, cl, cg, r, loss, grad)
    assert np.array_equal(loss.view(np.int32), loss2.view(np.int32)) and np.array_equal(grad.view(np.int32), grad2.view(np.int32))


@gpu
def test_forward_sum_refuses_text_past_the_limits(dev):
    import aligner_amd
    tx, ty = torch.tensor([1025], dtype=torch.int32), torch.tensor([1030], dtype=torch.int32)
    with pytest.raises(ValueError):
        aligner_amd.forward_sum(torch.zeros((1, 1025, 1030), device=dev), tx, ty)
    with pytest.raises(ValueError):
        aligner_amd.forward_sum(torch.zeros((1, 1024, 1030), device=dev), tx - 1, ty, blank_logprob=-1.0)
    loss, _ = aligner_amd.forward_sum(torch.zeros((1, 1024, 1030), device=dev), tx - 1, ty, want_grad=False)
    assert bool(torch.isfinite(loss).all())


@gpu
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("form", ["sys", "sys_serial", "one_wave"])
@pytest.mark.parametrize("B,Tx,Ty,blocked", [(5, 100, 240, (1, 3)), (3, 300, 500, (0,)), (4, 520, 600, (2, 3)), (4, 9, 14, (1,))])
def test_blocked_utterances_have_no_alignment_and_leave_their_neighbours_alone(dev, request, B, Tx, Ty, blocked, form, want_grad):
    """An utterance whose every path crosses a -inf cell (a frame whose valid rows are all -inf; t_x <= t_y): loss +inf
    and an all-zero gradient, as the oracle gives and as t_x > t_y gives; the other utterances of the batch are bit for bit
    what they are in the same batch with ordinary log-probs in place of the blocked ones."""
    if bucket(B, Tx, form) is None:
        form = "one_wave"
    lp, plain, tx, ty = make_blocked(B, Tx, Ty, blocked)
    wl, wg = FS.forward_sum(lp, tx, ty)
    assert np.isposinf(wl[list(blocked)]).all() and not wg[list(blocked)].any()
    _set_form(request, form)
    loss, grad = _run(dev, lp, tx, ty, want_grad=want_grad)
    loss_o, grad_o = _run(dev, plain, tx, ty, want_grad=want_grad)
    print(f"FSFIG blocked [{B},{Tx},{Ty}] {form} grad={want_grad}: loss of the blocked {loss[list(blocked)]}"
          + ("" if grad is None else f", max |gradient| {np.abs(grad[list(blocked)]).max():.3g}"))
    others = [b for b in range(B) if b not in blocked]
    assert np.isposinf(loss[list(blocked)]).all()
    assert np.array_equal(loss[others].view(np.int32), loss_o[others].view(np.int32))
    if want_grad:
        assert np.isfinite(grad).all() and not grad[list(blocked)].any()
        assert np.array_equal(grad[others].view(np.int32), grad_o[others].view(np.int32))
        el, eg = tol_units(loss.astype(np.float64), grad.astype(np.float64), wl, wg)
        assert el <= 1.0 and eg <= 1.0
    else:
        assert grad is None


@gpu
def test_forward_sum_loss_zero_infinity_drops_a_blocked_utterance(dev):
    """forward_sum_loss(zero_infinity=True): an utterance blocked by its log-probs contributes 0 and no gradient, like the
    t_x > t_y one test_objective.py covers (plain form: -inf scores are outside the CTC form's domain)."""
    import aligner_amd
    B, Tx, Ty = 3, 20, 48
    lp, plain, tx, ty = make_blocked(B, Tx, Ty, blocked=[1])
    z = torch.from_numpy(lp).to(dev).requires_grad_(True)
    txt, tyt = torch.from_numpy(tx), torch.from_numpy(ty)
    each = aligner_amd.forward_sum_loss(z, txt, tyt, blank_logprob=None, reduction="none")
    assert bool(torch.isposinf(each[1])) and bool(torch.isfinite(each[[0, 2]]).all())
    assert bool(torch.isposinf(aligner_amd.forward_sum_loss(z, txt, tyt, blank_logprob=None)))
    safe = aligner_amd.forward_sum_loss(z, txt, tyt, blank_logprob=None, reduction="sum", zero_infinity=True)
    assert abs(float(safe.detach()) - float(each[[0, 2]].detach().sum())) < 1e-3
    safe.backward()
    assert bool(torch.isfinite(z.grad).all()) and float(z.grad[1].abs().max()) == 0.0 and float(z.grad[0].abs().max()) > 0
