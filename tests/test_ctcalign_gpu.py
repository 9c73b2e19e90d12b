"""ctc_forced_align() / aligner_ctc_align on the GPU against the numpy oracle (tests/ctcalign_oracle.py).

All seven outputs must equal the oracle bit for bit: both perform the same fp32 adds and the same strict compares.
Batches are small (B = 2 .. 4), lengths ragged with utterance 0 at full size, labels drawn from three vocabulary entries
(so about a third of neighbouring labels repeat) unless a test says otherwise.  Only where utterance 0's repeats make a
listed T infeasible (L + Rt > T) is T raised, to L + Rt + 1; at the square shapes utterance 0's labels are drawn without
repeats, so (1,1) runs on a one-frame tensor and (5,5) with t_y == t_x == 5.  The shapes (L, T) sit on the kernel's own
edges:

    (1,1), (5,5)                                     smallest and square
    (4,7) all labels equal, V = 2                    every blank mandatory, a single legal path
    (63,140), (64,140), (65,140)                     wave boundary (64 rows)
    (12,31), (12,32), (12,33), (12,65)               32-frame decision tile boundary
    (256,600), (257,600), (512,1100), (513,1100),
    (1024,1500)                                      row groups per thread 1 / 2 / 4 (256 rows each), the largest text
    (600,1500) at B = 2                              decision words in the workspace, walked back by windows
"""
import functools

import numpy as np
import pytest
import torch

import ctcalign_oracle as CO
from aligner_amd import _lib, align_with_pauses, ctc_forced_align, ctc_token_spans
from aligner_amd import objective

pytestmark = pytest.mark.gpu

NAMES = ("tok", "labels", "frame_scores", "durations", "pauses", "state_durations", "score")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


EDGE_SHAPES = [(1, 1), (5, 5), (63, 140), (64, 140), (65, 140), (12, 31), (12, 32), (12, 33), (12, 65), (256, 600), (257, 600),
               (512, 1100), (513, 1100), (1024, 1500)]
ALL_SHAPES = [(4, L, T) for L, T in EDGE_SHAPES] + [(2, 600, 1500)]
VOCABS = [(V, b) for V in (3, 32, 33, 257) for b in sorted({0, V // 2, V - 1})]


def _shrink(lab, t_x, t_y):
    """the largest t_x' <= t_x whose labels fit t_y frames (0 when none does)"""
    while t_x >= 1 and t_x + int(CO.repeats(lab[:t_x])[1][-1]) > t_y:
        t_x -= 1
    return t_x


@functools.lru_cache(maxsize=None)
def make_case(B, L, T, V=32, blank=0, labels="three", seed=0):
    """Gaussian emissions times 2, ragged lengths, the first utterance at full size.  labels: "three" (three vocabulary
    entries at random), "none" (no two neighbours equal), "equal" (one entry), "aabb" (pairs), "distinct" (pairwise
    distinct: V >= L).  Cached and shared: a test that changes a case copies it first."""
    rng = np.random.default_rng(100000 * L + 10 * T + 7 * V + blank + seed)
    alpha = rng.permutation(V)[:3] if V >= 3 else np.arange(V)
    if labels == "three":
        tg = alpha[rng.integers(0, len(alpha), (B, L))]
    elif labels == "none":
        tg = alpha[(np.arange(L)[None, :] + rng.integers(0, 3, (B, 1))) % len(alpha)]
    elif labels == "equal":
        tg = np.broadcast_to(alpha[rng.integers(0, len(alpha), (B, 1))], (B, L)).copy()
    elif labels == "aabb":
        tg = alpha[((np.arange(L)[None, :] // 2) + rng.integers(0, 2, (B, 1))) % 2]
    else:
        tg = np.stack([rng.permutation(V)[:L] for _ in range(B)])
    if labels == "three" and T == L:                                   # square: only a transcript without repeats fits
        tg[0] = alpha[(np.arange(L) + rng.integers(0, 3)) % len(alpha)]
    tg = tg.astype(np.int64)
    need = L + int(CO.repeats(tg[0])[1][-1])
    if need > T:                                                       # utterance 0's repeats make the listed T infeasible
        T = need + 1
    e = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    ty = rng.integers(max(1, T // 2), T + 1, B).astype(np.int32)
    ty[0] = T
    tx = np.array([_shrink(tg[b], int(rng.integers(1, L + 1)), int(ty[b])) for b in range(B)], np.int32)
    tx[0] = L
    if B > 1:
        tx[1] = _shrink(tg[1], L, int(ty[1]))                          # as many rows in use as fit fewer frames
    return e, tg, tx, ty


def run(dev, lp_t, tg, tx, ty, blank, **kw):
    res = ctc_forced_align(lp_t, torch.from_numpy(np.asarray(tg)).to(dev), torch.from_numpy(np.asarray(ty)).to(dev),
                           torch.from_numpy(np.asarray(tx)).to(dev), blank, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def check(got, want, tg, tx, ty, V, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert np.array_equal(g, w, equal_nan=g.dtype == np.float32), f"{what}: {name} differs from the oracle"
    B, L = got[3].shape
    T = got[0].shape[1]
    for b in range(B):
        if CO.feasible(tg[b], tx[b], ty[b], L, T, V):
            assert CO.is_legal(got[0][b], tg[b], tx[b], ty[b]), f"{what}: utterance {b} is not a legal path"
            assert got[3][b].sum() + got[4][b].sum() == ty[b] and (got[3][b, :tx[b]] >= 1).all()
        else:
            assert (got[0][b] == -1).all() and (got[1][b] == -1).all() and not got[2][b].any() and not got[3][b].any()
            assert not got[4][b].any() and not got[5][b].any() and got[6][b] == -np.inf


def oracle_and_gpu(dev, case, blank, V, what, lp_t=None, e=None):
    e0, tg, tx, ty = case
    e = e0 if e is None else e
    want = CO.ctc_align(e, tg, ty, tx, blank)
    got = run(dev, torch.from_numpy(e).to(dev) if lp_t is None else lp_t, tg, tx, ty, blank)
    check(got, want, tg, tx, ty, V, what)
    return got, want


@pytest.mark.parametrize("V,blank", VOCABS)
@pytest.mark.parametrize("B,L,T", ALL_SHAPES)
def test_edge_shapes_equal_the_oracle(dev, B, L, T, V, blank):
    case = make_case(B, L, T, V, blank)
    Rt = CO.repeats(case[1][0])[1][-1]
    assert case[0].shape[1] == (T if L + Rt <= T else L + Rt + 1) and case[2][0] == L and case[3][0] == case[0].shape[1]
    if T == L:
        assert case[0].shape[1] == T
    got, _ = oracle_and_gpu(dev, case, blank, V, f"[{B},{L},{T}] V={V} blank={blank}")
    if (L, T, V) == (12, 65, 32):
        frac = (got[0] <= -2).sum() / case[3].sum()
        assert 0.1 < frac < 0.9, f"blank frames {frac:.2f}: the case does not exercise the blank states"
    if L >= 63:
        r = CO.repeats(case[1][0])[1][-1] / L
        assert 0.1 < r < 0.6, f"repeat fraction {r:.2f}: the case does not exercise the repeat rule"


def test_all_labels_equal_is_a_single_path(dev):
    """(4,7), V = 2: every blank mandatory, t_y = t_x + Rt for utterance 0 -- one legal path whatever the scores."""
    B, L, V = 4, 4, 2
    for blank in (0, 1):
        e, tg, tx, ty = make_case(B, L, 7, V, blank, labels="equal")
        assert e.shape[1] == 7 and tx[0] == 4 and ty[0] == 7
        got, _ = oracle_and_gpu(dev, (e, tg, tx, ty), blank, V, f"all equal blank={blank}")
        assert got[0][0].tolist() == [0, -3, 1, -4, 2, -5, 3]
        en = np.full_like(e, np.nan)
        got, _ = oracle_and_gpu(dev, (en, tg, tx, ty), blank, V, "all equal, all NaN")
        assert got[0][0].tolist() == [0, -3, 1, -4, 2, -5, 3]


@pytest.mark.parametrize("B,L,T", [(4, 5, 12), (4, 65, 140), (3, 257, 600)])
@pytest.mark.parametrize("regime", ["none", "equal", "aabb", "tight", "tight_plus_one"])
def test_repeat_regimes(dev, B, L, T, regime):
    V, blank = 5, 2
    if regime in ("tight", "tight_plus_one"):
        e, tg, tx, ty = make_case(B, L, T, V, blank)
        tx, ty = tx.copy(), ty.copy()
        for b in range(B):
            ty[b] = tx[b] + CO.repeats(tg[b, :tx[b]])[1][-1] + (regime == "tight_plus_one")
            assert ty[b] <= e.shape[1]
    else:
        e, tg, tx, ty = make_case(B, L, 2 * L + 2, V, blank, labels=regime)
        rep = CO.repeats(tg[0])[1][-1]
        assert rep == {"none": 0, "equal": L - 1, "aabb": L // 2}[regime]
    got, _ = oracle_and_gpu(dev, (e, tg, tx, ty), blank, V, regime)
    if regime == "tight":
        assert (got[3][np.arange(L)[None, :] < tx[:, None]] == 1).all()


@pytest.mark.parametrize("B,L,T", [(4, 200, 1000), (2, 600, 1500)])
def test_distinct_labels_equal_align_with_pauses(dev, B, L, T):
    """Pairwise distinct labels: the existing kernel on the gathered scores, the blank column as its pause row."""
    V, blank = L + 5, 3
    e, tg, tx, ty = make_case(B, L, T, V, blank, labels="distinct")
    lp = torch.from_numpy(e).to(dev)
    d_tg, d_tx, d_ty = torch.from_numpy(tg).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    res = ctc_forced_align(lp, d_tg, d_ty, d_tx, blank)
    value = lp.gather(2, d_tg[:, None, :].expand(B, e.shape[1], L)).transpose(1, 2).contiguous()
    ref = align_with_pauses(value, d_tx, d_ty, pause=lp[:, :, blank].contiguous(), want_state_durations=True)
    assert (_lib.load().aligner_ctc_align_workspace_bytes(B, L, e.shape[1]) > 0) == (L == 600)
    for name in ("tok", "durations", "pauses", "state_durations"):
        assert torch.equal(getattr(res, name), getattr(ref, name)), name
    assert torch.equal(res.score.view(torch.int32), ref.score.view(torch.int32))
    assert (res.tok <= -2).any() and torch.isfinite(res.score).all()


@pytest.mark.parametrize("B,L,T", [(4, 5, 5), (4, 12, 33), (4, 65, 140), (3, 257, 600)])
@pytest.mark.parametrize("levels", [2, 3])
def test_ties_keep_the_earlier_candidate(dev, B, L, T, levels):
    """Small-integer emissions: the running sums are exact and equal sums are everywhere, so every decision is made by
    the order stay / advance / skip and the strict compare."""
    V, blank = 4, 1
    e0, tg, tx, ty = make_case(B, L, T, V, blank)
    rng = np.random.default_rng(L + T + levels)
    e = rng.integers(0, levels, e0.shape).astype(np.float32)
    oracle_and_gpu(dev, (e0, tg, tx, ty), blank, V, f"ties [{B},{L},{T}] {levels} levels", e=e)


@pytest.mark.parametrize("B,L,T", [(4, 65, 140), (3, 257, 600)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_emissions_are_upcast_exactly(dev, dtype, B, L, T):
    V, blank = 33, 32
    e0, tg, tx, ty = make_case(B, L, T, V, blank)
    e16 = torch.from_numpy(e0).to(dtype)
    oracle_and_gpu(dev, (e0, tg, tx, ty), blank, V, str(dtype), lp_t=e16.to(dev), e=e16.float().numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L,T", [(4, 65, 140), (3, 12, 33), (2, 257, 600)])
def test_strided_emissions_are_read_in_place(dev, B, L, T, dtype, monkeypatch):
    """A [T,B,V] tensor seen as [B,T,V], and rows at a pitch above V whose padding holds NaN: the contiguous result, and
    the pointer the library is given is the view's own."""
    V, blank = 33, 0
    e0, tg, tx, ty = make_case(B, L, T, V, blank)
    T = e0.shape[1]
    e = torch.from_numpy(e0).to(dtype)
    want = CO.ctc_align(e.float().numpy(), tg, ty, tx, blank)
    lib = _lib.load()
    seen = []
    real = lib.aligner_ctc_align

    def spy(*args):
        seen.append(args[:4])
        return real(*args)
    monkeypatch.setattr(lib, "aligner_ctc_align", spy, raising=False)
    tbv = e.transpose(0, 1).contiguous().to(dev)                      # [T,B,V]
    view = tbv.transpose(0, 1)
    assert not view.is_contiguous() or B == 1
    got = run(dev, view, tg, tx, ty, blank)
    check(got, want, tg, tx, ty, V, "[T,B,V] view")
    assert seen[-1][0] == view.data_ptr() and seen[-1][2:] == (V, B * V)
    pitch = V + 7
    buf = torch.full((B, T, pitch), float("nan"), dtype=dtype, device=dev)
    buf[:, :, :V] = e.to(dev)
    view = buf[:, :, :V]
    assert not view.is_contiguous()
    got = run(dev, view, tg, tx, ty, blank)
    check(got, want, tg, tx, ty, V, "pitched rows")
    assert seen[-1][0] == view.data_ptr() and seen[-1][2:] == (T * pitch, pitch)


@pytest.mark.parametrize("case", ["inf_blank", "inf_labels", "nan_cell", "all_nan"])
def test_unusual_scores_equal_the_oracle_and_stay_legal(dev, case):
    B, L, T, V, blank = 4, 65, 140, 32, 31
    e0, tg, tx, ty = make_case(B, L, T, V, blank)
    e = e0.copy()
    if case == "inf_blank":
        e[:, :, blank] = -np.inf
    elif case == "inf_labels":
        for b in range(B):
            e[b, :, tg[b, 0]] = -np.inf                               # one of the three entries in use
        e[0, 20:40, :] = -np.inf
    elif case == "nan_cell":
        e[0, 30, tg[0, 14]] = np.nan
        e[2, 0, blank] = np.nan
    else:
        e[:] = np.nan
    oracle_and_gpu(dev, (e0, tg, tx, ty), blank, V, case, e=e)


@pytest.mark.parametrize("how", ["short", "no_labels", "label_V", "label_minus_one"])
def test_an_infeasible_utterance_does_not_disturb_the_others(dev, how):
    """The emissions lie between NaN guard bands: a load outside them shows in the scores."""
    B, L, T, V, blank = 4, 65, 140, 32, 5
    e, tg, tx, ty = make_case(B, L, T, V, blank)
    T = e.shape[1]
    base = CO.ctc_align(e, tg, ty, tx, blank)
    tg, tx, ty = tg.copy(), tx.copy(), ty.copy()
    bad = 2
    if how == "short":
        ty[bad] = tx[bad] + CO.repeats(tg[bad, :tx[bad]])[1][-1] - 1
    elif how == "no_labels":
        tx[bad] = 0
    else:
        tg[bad, tx[bad] // 2] = V if how == "label_V" else -1
    guard = 1 << 16
    buf = torch.full((guard + B * T * V + guard,), float("nan"), dtype=torch.float32, device=dev)
    lp = buf[guard:guard + B * T * V].view(B, T, V)
    lp.copy_(torch.from_numpy(e))
    want = CO.ctc_align(e, tg, ty, tx, blank)
    got = run(dev, lp, tg, tx, ty, blank)
    check(got, want, tg, tx, ty, V, how)
    assert got[6][bad] == -np.inf and (got[0][bad] == -1).all() and (got[1][bad] == -1).all() and not got[2][bad].any()
    assert not got[3][bad].any() and not got[4][bad].any() and not got[5][bad].any()
    for b in range(B):
        if b != bad:
            assert np.isfinite(got[6][b]) and np.isfinite(got[2][b]).all()
            for g, w in zip(got, base):
                assert np.array_equal(g[b], w[b])


BAND, CANARY = 4096, 0xA5


class Fenced:
    """nbytes of device memory with a canary band before and after it (as tests/test_pausepath_gpu.py)."""

    def __init__(self, nbytes, dev, align=256):
        self.n = int(nbytes)
        pad = (-self.n) % align
        self.buf = torch.full((BAND + self.n + pad + BAND,), CANARY, dtype=torch.uint8, device=dev)
        self.lo, self.hi = BAND, BAND + self.n
        self.buf[self.lo:self.hi] = 0xFF                               # (an element left unwritten shows as -1 / NaN)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def view(self, dtype, shape):
        return self.buf[self.lo:self.hi].view(dtype).reshape(shape)

    def intact(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.hi:] == CANARY).all())


@pytest.mark.parametrize("B,L,T", [(3, 1, 1), (3, 7, 13), (4, 65, 140), (2, 257, 600), (2, 600, 1500), (0, 7, 13)])
def test_writes_stay_inside_their_buffers(dev, B, L, T):
    lib = _lib.load()
    V, blank = 32, 0
    e, tg, tx, ty = make_case(max(B, 1), L, T, V, blank)
    e, tg, tx, ty = e[:B], tg[:B], tx[:B].copy(), ty[:B].copy()
    assert e.shape[1] == T or L > 1                                   # (3,1,1): a one-frame tensor
    T = e.shape[1]
    if B:
        tx[-1] = 0                                                    # one utterance without a path
    lp = torch.from_numpy(e).to(dev)
    d_tg = torch.from_numpy(tg.astype(np.int32)).to(dev)
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    wsb = lib.aligner_ctc_align_workspace_bytes(B, L, T)
    assert (wsb > 0) == (L == 600)
    want = CO.ctc_align(e, tg, ty, tx, blank) if B else None
    shapes = [(B, T), (B, T), (B, T), (B, L), (B, L + 1), (B, 2 * L + 1), (B,)]
    dtypes = [torch.int32, torch.int32, torch.float32, torch.int32, torch.int32, torch.int32, torch.float32]
    one = torch.zeros(4, device=dev)                                  # (pointers of an empty batch are not looked at)
    for which in [range(7)] + [[i] for i in range(7)]:                # all at once, then one at a time
        ws = Fenced(wsb, dev)
        outs = [Fenced(int(np.prod(shapes[i])) * 4, dev) if i in which else None for i in range(7)]
        _lib.check(lib.aligner_ctc_align(lp.data_ptr() if B else one.data_ptr(), _lib.DT_F32, T * V, V, V, blank, d_tg.data_ptr() if B else one.data_ptr(),
                                         d_tx.data_ptr() if B else one.data_ptr(), d_ty.data_ptr() if B else one.data_ptr(),
                                         *[None if o is None else o.ptr for o in outs], ws.ptr if wsb else None, wsb, B, L, T,
                                         torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert ws.intact(), "workspace: the kernel wrote outside its buffer"
        for i in which:
            assert outs[i].intact(), f"{NAMES[i]}: the kernel wrote outside its buffer"
            if B:
                g = outs[i].view(dtypes[i], shapes[i]).cpu().numpy()
                assert np.array_equal(g, want[i]), f"{NAMES[i]} (requested {'alone' if len(which) == 1 else 'with the others'})"
    # a too small workspace is refused, not overrun
    if wsb:
        tok = Fenced(B * T * 4, dev)
        rc = lib.aligner_ctc_align(lp.data_ptr(), _lib.DT_F32, T * V, V, V, blank, d_tg.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(),
                                   tok.ptr, None, None, None, None, None, None, ws.ptr, wsb - 4, B, L, T,
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.ENOSPC


def test_single_outputs_and_empty_shapes_from_python(dev):
    e, tg, tx, ty = make_case(4, 12, 33)
    lp, d_tg = torch.from_numpy(e).to(dev), torch.from_numpy(tg).to(dev)
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    want = CO.ctc_align(e, tg, ty, tx, 0)
    flags = tuple("want_" + n for n in NAMES)
    for i, name in enumerate(flags):
        res = ctc_forced_align(lp, d_tg, d_ty, d_tx, 0, **{f: f == name for f in flags})
        assert [t is not None for t in res] == [f == name for f in flags]
        assert np.array_equal(res[i].cpu().numpy(), want[i])
    with pytest.raises(ValueError):
        ctc_forced_align(lp, d_tg, d_ty, d_tx, 0, **{f: False for f in flags})
    # lengths given as None mean T and L
    full = ctc_forced_align(lp, d_tg)
    wf = CO.ctc_align(e, tg, np.full(4, e.shape[1]), np.full(4, 12), 0)
    for g, w in zip(full, wf):
        assert np.array_equal(g.cpu().numpy(), w)
    res = ctc_forced_align(lp[:0], d_tg[:0], d_ty[:0], d_tx[:0])
    assert [tuple(t.shape) for t in res] == [(0, 33), (0, 33), (0, 33), (0, 12), (0, 13), (0, 25), (0,)]
    res = ctc_forced_align(lp, d_tg[:, :0], d_ty, d_tx * 0)                                      # no label: no path
    assert (res.tok == -1).all() and (res.labels == -1).all() and not res.frame_scores.any() and (res.score == -float("inf")).all()
    assert tuple(res.pauses.shape) == (4, 1) and not res.pauses.any() and not res.state_durations.any()
    res = ctc_forced_align(lp[:, :0], d_tg, d_ty * 0, d_tx)                                      # no frame: no path
    assert tuple(res.tok.shape) == (4, 0) and not res.durations.any() and (res.score == -float("inf")).all()
    with pytest.raises(ValueError):
        ctc_forced_align(lp, torch.zeros(4, 1025, dtype=torch.int64, device=dev))
    # other dtypes are cast to fp32
    res64 = ctc_forced_align(lp.double(), d_tg, d_ty, d_tx)
    assert np.array_equal(res64.tok.cpu().numpy(), want[0]) and np.array_equal(res64.score.cpu().numpy(), want[6])


def test_one_frame_tensors(dev):
    """T == 1: the frame pitch is never used -- a [B,1,V] tensor is read in place whatever its frame stride says, and the
    library takes any stride_t >= V for it."""
    B, L, V, blank = 4, 3, 5, 2
    rng = np.random.default_rng(17)
    e = rng.standard_normal((B, 1, V)).astype(np.float32)
    tg = rng.integers(0, V, (B, L))
    tx = np.array([1, 1, 2, 0], np.int32)                             # one label fits one frame; two or none do not
    ty = np.array([1, 1, 1, 1], np.int32)
    want = CO.ctc_align(e, tg, ty, tx, blank)
    lp = torch.from_numpy(e).to(dev)
    check(run(dev, lp, tg, tx, ty, blank), want, tg, tx, ty, V, "[B,1,V]")
    assert want[0][:2, 0].tolist() == [0, 0] and (want[0][2:] == -1).all()
    odd = torch.as_strided(lp, (B, 1, V), (V, 1, 1))                  # frame stride 1 < V: legal, there is one frame
    assert odd.stride(1) < V and torch.equal(odd, lp)
    lib = _lib.load()
    seen = []
    real = lib.aligner_ctc_align

    def spy(*args):
        seen.append(args[:4])
        return real(*args)
    lib.aligner_ctc_align = spy
    try:
        got = run(dev, odd, tg, tx, ty, blank)
    finally:
        lib.aligner_ctc_align = real
    check(got, want, tg, tx, ty, V, "[B,1,V] with frame stride 1")
    assert seen[-1][0] == odd.data_ptr() and seen[-1][3] == V
    # the C ABI with a frame stride far above V at T == 1
    d_tg = torch.from_numpy(tg.astype(np.int32)).to(dev)
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    tok = torch.full((B, 1), 7, dtype=torch.int32, device=dev)
    score = torch.zeros(B, device=dev)
    _lib.check(real(lp.data_ptr(), _lib.DT_F32, V, 1 << 40, V, blank, d_tg.data_ptr(), d_tx.data_ptr(), d_ty.data_ptr(),
                    tok.data_ptr(), None, None, None, None, None, score.data_ptr(), None, 0, B, L, 1,
                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(tok.cpu().numpy(), want[0]) and np.array_equal(score.cpu().numpy(), want[6])


def test_score_definitions(dev):
    """score is the fp32 left-to-right sum of frame_scores[:t_y]; frame_scores is log_probs[b, y, labels[b,y]] exactly;
    on normalised emissions the best path is one term of the CTC sum, so score <= -ctc_loss in float64."""
    B, L, T, V, blank = 4, 40, 120, 32, 0
    e, tg, tx, ty = make_case(B, L, T, V, blank)
    T = e.shape[1]
    lp = torch.log_softmax(torch.from_numpy(e).double(), 2).float()
    got = run(dev, lp.to(dev), tg, tx, ty, blank)
    tok, labels, fs, score = got[0], got[1], got[2], got[6]
    assert (tx >= 1).all() and ((tok <= -2).sum(1) > 0).all()
    lpn = lp.numpy()
    acc = fs[:, 0].copy()
    for y in range(1, T):
        acc = np.where(y < ty, (acc + fs[:, y]).astype(np.float32), acc)
    assert np.array_equal(acc, score)
    for b in range(B):
        assert np.array_equal(fs[b, :ty[b]], lpn[b, np.arange(ty[b]), labels[b, :ty[b]]]) and not fs[b, ty[b]:].any()
    # (targets that hold the blank id are not CTC targets: draw the comparison's labels from the other entries)
    tgc = np.where(tg == blank, (blank + 1) % V, tg)
    tyc = np.array([max(int(ty[b]), int(tx[b] + CO.repeats(tgc[b, :tx[b]])[1][-1])) for b in range(B)])
    assert (tyc <= T).all()
    got = run(dev, lp.to(dev), tgc, tx, tyc, blank)
    loss = torch.nn.functional.ctc_loss(lp.double().transpose(0, 1), torch.from_numpy(tgc), torch.from_numpy(tyc).long(),
                                        torch.from_numpy(tx).long(), blank=blank, reduction="none")
    ll = -loss.numpy()
    sc = got[6].astype(np.float64)
    assert np.isfinite(sc).all() and np.isfinite(ll).all()
    assert (sc <= ll).all(), (sc, ll)
    assert (sc > ll - 0.5 * tyc * np.log(2.0 * tx + 1)).all()           # ... and not absurdly far below it


@pytest.mark.parametrize("B,L,T", [(4, 12, 65), (3, 257, 600)])
def test_token_spans(dev, B, L, T):
    V, blank = 32, 0
    e, tg, tx, ty = make_case(B, L, T, V, blank)
    T = e.shape[1]
    tx = tx.copy()
    tx[-1] = 0                                                        # an utterance without a path: no token has frames
    lp = torch.log_softmax(torch.from_numpy(e), 2)
    d_tg, d_tx, d_ty = torch.from_numpy(tg).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    res = ctc_forced_align(lp.to(dev), d_tg, d_ty, d_tx, blank)
    start, end, score, logp = (t.cpu().numpy() for t in ctc_token_spans(res, d_ty))
    assert start.dtype == np.int32 and end.dtype == np.int32 and score.dtype == np.float32 and logp.dtype == np.float32
    assert start.shape == end.shape == score.shape == logp.shape == (B, L)
    want = CO.ctc_align(lp.numpy(), tg, ty, tx, blank)
    fs = res.frame_scores.cpu().numpy()
    p32 = res.frame_scores.exp().cpu().numpy()                        # the fp32 values the reduction sums
    for b in range(B):
        st = CO.states_from_tok(want[0][b], ty[b] if tx[b] else 0)
        for x in range(L):
            ys = np.nonzero(st == 2 * x + 1)[0]
            d = len(ys)
            if d == 0:
                assert start[b, x] == end[b, x] and score[b, x] == 0 and logp[b, x] == 0
                continue
            assert (start[b, x], end[b, x]) == (ys[0], ys[-1] + 1) and d == ys[-1] + 1 - ys[0]
            m = p32[b, ys].astype(np.float64).mean()
            assert abs(score[b, x] - m) <= (d + 1) * 2.0 ** -24 * m, (b, x, d, score[b, x], m)
            s = fs[b, ys].astype(np.float64)
            assert abs(logp[b, x] - s.sum()) <= (d - 1) * 2.0 ** -24 * np.abs(s).sum(), (b, x, d, logp[b, x], s.sum())
    same = ctc_token_spans(res)
    assert all(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(same, (start, end, score, logp)))


def test_consumers_take_the_outputs_as_they_are(dev):
    B, L, T, V, blank, C = 4, 65, 140, 32, 0, 3
    e, tg, tx, ty = make_case(B, L, T, V, blank)
    T = e.shape[1]
    lp = torch.log_softmax(torch.from_numpy(e), 2).to(dev)
    d_tg, d_tx, d_ty = torch.from_numpy(tg).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    res = ctc_forced_align(lp, d_tg, d_ty, d_tx, blank)
    assert (res.tok <= -2).any()
    # the binarization loss counts the token frames only: value[b,x,y] = log_probs[b,y,targets[b,x]]
    value = lp.gather(2, d_tg[:, None, :].expand(B, T, L)).transpose(1, 2).contiguous()
    _, count = objective.bin_loss(value, res.tok, d_ty)
    assert torch.equal(count, res.durations.sum(1).to(torch.int32))
    assert torch.isfinite(objective.binarization_loss(value, res.tok, d_ty))
    # the regulator expands text encodings interleaved with a blank embedding
    h = torch.zeros(B, C, 2 * L + 1, device=dev)
    h[:, 0, 0::2] = 1.0
    h[:, 1, :] = torch.arange(2 * L + 1, device=dev, dtype=torch.float32)
    out, rtok = objective.regulate(h, res.state_durations, T)
    frames = torch.arange(T, device=dev)[None, :] < d_ty[:, None]
    assert torch.equal(out[:, 0] == 1.0, (res.tok <= -2) & frames)
    state = torch.where(res.tok >= 0, 2 * res.tok + 1, 2 * (-2 - res.tok))
    assert torch.equal(out[:, 1][frames], state[frames].float())
    assert torch.equal(rtok[frames], state[frames].to(rtok.dtype))
