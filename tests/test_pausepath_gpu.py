"""align_with_pauses() / aligner_pausepath on the GPU against the numpy oracle (tests/pausepath_oracle.py).

tok, durations, pauses, state_durations and score must equal the oracle bit for bit: both perform the same fp32 adds
and the same strict compares.  Shapes sit at the edges of the kernel's structure: the wave boundary (64 rows), the row
groups of a thread (256 rows each, 1 / 2 / 4 groups), the 32-frame decision tile, the largest text, and one shape
whose decision words do not fit LDS (the workspace walk)."""
import functools

import numpy as np
import pytest
import torch

import pausepath_oracle as PO
from aligner_amd import _lib, align, align_with_pauses
from aligner_amd import objective
from aligner_amd.softattn import pitched_logp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


EDGE_SHAPES = [(1, 1), (5, 5), (63, 70), (64, 70), (65, 70), (20, 31), (20, 32), (20, 33), (20, 65), (256, 300), (257, 300),
               (300, 330), (1024, 1030)]
BIG_LDS = [(4, Tx, Ty) for Tx, Ty in EDGE_SHAPES]
ALL_SHAPES = BIG_LDS + [(2, 600, 1500)]            # the last one: decision words in the workspace, walked by windows


@functools.lru_cache(maxsize=None)
def make_case(B, Tx, Ty, seed=0):
    """Gaussian scores times 2 (with pause = 0.5 about half the frames become pauses), ragged lengths, the first
    utterance at full size.  Cached and shared: a test that changes a case copies it first."""
    rng = np.random.default_rng(1000 * Tx + Ty + seed)
    value = (2.0 * rng.standard_normal((B, Tx, Ty))).astype(np.float32)
    ty = rng.integers(max(1, Ty // 2), Ty + 1, B).astype(np.int32)
    tx = np.array([rng.integers(1, min(Tx, t) + 1) for t in ty], np.int32)
    tx[0], ty[0] = min(Tx, Ty), Ty
    if B > 1:
        tx[1], ty[1] = min(Tx, int(ty[1])), ty[1]                      # every row in use, fewer frames
    pz = rng.standard_normal((B, Ty)).astype(np.float32)
    return value, tx, ty, pz


def gap_masks(kind, B, Tx, tx, seed=0):
    if kind == "none":
        return None
    gm = np.zeros((B, Tx + 1), np.uint8)
    rng = np.random.default_rng(seed + Tx)
    for b in range(B):
        if kind == "words":                                           # every 3rd to 5th gap
            g = 0
            while g <= tx[b]:
                gm[b, g] = 1
                g += int(rng.integers(3, 6))
        elif kind == "ends":
            gm[b, 0] = 1
            gm[b, max(int(tx[b]), 0)] = 1
    return gm                                                         # "zero": all disallowed


def run(dev, value_t, tx, ty, pause, gm, **kw):
    res = align_with_pauses(value_t, torch.from_numpy(np.asarray(tx)).to(dev), torch.from_numpy(np.asarray(ty)).to(dev),
                            pause=torch.from_numpy(pause).to(dev) if isinstance(pause, np.ndarray) else pause,
                            gap_mask=None if gm is None else torch.from_numpy(gm).to(dev),
                            want_state_durations=True, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def check(got, want, tx, ty, gm=None, what=""):
    for name, g, w in zip(("tok", "durations", "pauses", "state_durations"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differs from the oracle"
    assert got[4].dtype == np.float32 and np.array_equal(got[4], want[4], equal_nan=True), f"{what}: score {got[4]} vs {want[4]}"
    B, Tx = got[1].shape
    Ty = got[0].shape[1]
    for b in range(B):
        if PO.feasible(tx[b], ty[b], Tx, Ty):
            assert PO.is_legal(got[0][b], tx[b], ty[b], None if gm is None else gm[b]), f"{what}: utterance {b} is not a legal path"
            assert got[1][b].sum() + got[2][b].sum() == ty[b] and (got[1][b, :tx[b]] >= 1).all()


@pytest.mark.parametrize("pause_kind", ["half", "minus_one", "tensor"])
@pytest.mark.parametrize("B,Tx,Ty", ALL_SHAPES)
def test_edge_shapes_equal_the_oracle(dev, B, Tx, Ty, pause_kind):
    value, tx, ty, pz = make_case(B, Tx, Ty)
    pause = {"half": 0.5, "minus_one": -1.0, "tensor": pz}[pause_kind]
    want = PO.pause_align(value, tx, ty, pause)
    got = run(dev, torch.from_numpy(value).to(dev), tx, ty, pause, None)
    check(got, want, tx, ty, what=f"[{B},{Tx},{Ty}] {pause_kind}")
    if pause_kind == "half" and (Tx, Ty) == (20, 65):
        frac = (got[0] <= -2).sum() / ty.sum()
        assert 0.2 < frac < 0.8, f"pause frames {frac:.2f}: the case does not exercise the pause states"


@pytest.mark.parametrize("kind", ["zero", "words", "ends"])
@pytest.mark.parametrize("B,Tx,Ty", [(4, 5, 5), (4, 65, 70), (4, 20, 65), (4, 257, 300), (2, 600, 1500)])
def test_gap_masks(dev, B, Tx, Ty, kind):
    value, tx, ty, _ = make_case(B, Tx, Ty)
    gm = gap_masks(kind, B, Tx, tx)
    want = PO.pause_align(value, tx, ty, 0.5, gm)
    got = run(dev, torch.from_numpy(value).to(dev), tx, ty, 0.5, gm)
    check(got, want, tx, ty, gm, what=f"[{B},{Tx},{Ty}] mask {kind}")
    # bool and integer masks mean the same
    for cast in (torch.bool, torch.int64):
        res = align_with_pauses(torch.from_numpy(value).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev), 0.5,
                                torch.from_numpy(gm).to(dev).to(cast))
        assert np.array_equal(res.tok.cpu().numpy(), want[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_scores_are_upcast_in_the_loader(dev, dtype):
    value, tx, ty, pz = make_case(4, 65, 70)
    v16 = torch.from_numpy(value).to(dtype)
    want = PO.pause_align(v16.float().numpy(), tx, ty, pz)
    got = run(dev, v16.to(dev), tx, ty, pz, None)
    check(got, want, tx, ty, what=str(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Tx,Ty", [(4, 65, 70), (3, 20, 37), (2, 257, 300)])
def test_pitched_rows_and_unaligned_mel_axis(dev, B, Tx, Ty, dtype):
    """A pitched_logp() view is read in place (the padding holds NaN: never read into a result); Ty = 37 gives rows that
    are not 16-byte aligned."""
    value, tx, ty, _ = make_case(B, Tx, Ty)
    v = torch.from_numpy(value).to(dtype)
    want = PO.pause_align(v.float().numpy(), tx, ty, 0.5)
    got = run(dev, v.to(dev), tx, ty, 0.5, None)
    check(got, want, tx, ty, what="contiguous")
    lp = pitched_logp(B, Tx, Ty, dev, dtype)
    lp._base.fill_(float("nan"))
    lp.copy_(v)
    assert not lp.is_contiguous()
    got = run(dev, lp, tx, ty, 0.5, None)
    check(got, want, tx, ty, what="pitched")


@pytest.mark.parametrize("B,Tx,Ty", [(8, 200, 1000)] + BIG_LDS)
def test_without_gaps_it_is_the_pinned_search(dev, B, Tx, Ty):
    """Every gap disallowed: tok and durations equal align()'s, which is pinned to the reference search."""
    value, tx, ty, _ = make_case(B, Tx, Ty)
    v = torch.from_numpy(value).to(dev)
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    ref = align(v, d_tx, d_ty, want_path=False, want_tok=True)
    res = align_with_pauses(v, d_tx, d_ty, pause=5.0, gap_mask=torch.zeros(B, Tx + 1, dtype=torch.uint8, device=dev))
    assert torch.equal(res.tok, ref.tok) and torch.equal(res.durations, ref.durations)
    assert not res.pauses.any()


@pytest.mark.parametrize("B,Tx,Ty", [(4, 5, 5), (4, 20, 65), (4, 65, 70), (4, 257, 300)])
@pytest.mark.parametrize("levels,pause", [(2, 0.0), (3, 1.0), (2, 1.0)])
def test_ties_keep_the_earlier_candidate(dev, B, Tx, Ty, levels, pause):
    """Small-integer scores and an integer pause: the running sums are exact and equal sums are everywhere, for token and
    pause states alike, so every decision is made by the order stay / advance / skip and the strict compare."""
    rng = np.random.default_rng(Tx + Ty + levels)
    _, tx, ty, _ = make_case(B, Tx, Ty)
    value = rng.integers(0, levels, (B, Tx, Ty)).astype(np.float32)
    pz = rng.integers(0, 2, (B, Ty)).astype(np.float32)
    for pa, gm in ((pause, None), (pz, None), (pause, gap_masks("words", B, Tx, tx))):
        want = PO.pause_align(value, tx, ty, pa, gm)
        got = run(dev, torch.from_numpy(value).to(dev), tx, ty, pa, gm)
        check(got, want, tx, ty, gm, what=f"ties [{B},{Tx},{Ty}]")


def test_infeasible_utterances_do_not_disturb_the_others(dev):
    Tx, Ty = 70, 90
    B = 9
    rng = np.random.default_rng(5)
    value = (2.0 * rng.standard_normal((B, Tx, Ty))).astype(np.float32)
    tx = np.array([0, 5, 9, 7, Tx + 1, 3, -1, Tx, 66], np.int32)
    ty = np.array([10, 0, 6, 12, Ty, Ty + 1, 5, Ty, 80], np.int32)
    want = PO.pause_align(value, tx, ty, 0.5)
    got = run(dev, torch.from_numpy(value).to(dev), tx, ty, 0.5, None)
    check(got, want, tx, ty, what="mixed batch")
    for b in (0, 1, 2, 4, 5, 6):
        assert (got[0][b] == -1).all() and not got[1][b].any() and not got[2][b].any() and not got[3][b].any()
        assert got[4][b] == -np.inf
    for b in (3, 7, 8):
        assert np.isfinite(got[4][b]) and got[1][b].sum() + got[2][b].sum() == ty[b]


@pytest.mark.parametrize("case", ["inf_rows", "inf_pause", "nan_cell", "all"])
def test_unusual_scores_equal_the_oracle_and_stay_legal(dev, case):
    B, Tx, Ty = 4, 65, 70
    value, tx, ty, pz = make_case(B, Tx, Ty)
    value, pz = value.copy(), pz.copy()
    pause = pz
    if case in ("inf_rows", "all"):
        for b in range(B):
            value[b, tx[b]:] = -np.inf                 # soft_attention's padding rows
        value[0, 7] = -np.inf                          # and a text row inside the utterance
    if case in ("inf_pause", "all"):
        pause = -np.inf if case == "inf_pause" else pz
        pz[:, 10:20] = -np.inf
    if case in ("nan_cell", "all"):
        value[0, 30, 33] = np.nan
        value[2, 0, 0] = np.nan
    want = PO.pause_align(value, tx, ty, pause)
    got = run(dev, torch.from_numpy(value).to(dev), tx, ty, pause, None)
    check(got, want, tx, ty, what=case)


def test_score_is_the_left_to_right_sum_along_tok(dev):
    B, Tx, Ty = 8, 200, 1000
    value, tx, ty, pz = make_case(B, Tx, Ty)
    got = run(dev, torch.from_numpy(value).to(dev), tx, ty, pz, None)
    tok = got[0]
    assert ((tok <= -2).sum(1) > 0).all()
    sc = np.where(tok >= 0, np.take_along_axis(value, np.clip(tok, 0, Tx - 1)[:, None, :], 1)[:, 0, :], pz)
    acc = sc[:, 0].copy()
    for y in range(1, Ty):
        acc = np.where(y < ty, (acc + sc[:, y]).astype(np.float32), acc)
    assert np.array_equal(acc, got[4])
    want = PO.pause_align(value, tx, ty, pz)
    check(got, want, tx, ty, what="[8,200,1000]")


def test_viterbi_score_is_below_the_ctc_log_likelihood(dev):
    """Scores normalised as the CTC form of forward_sum() normalises them (a blank row at blank_logprob in front of the
    text rows, every frame renormalised over blank + text), the blank as the pause: the best path is one term of the
    sum, so score <= -loss, as it stands (the other terms are many nats here: rounding cannot turn it round)."""
    B, Tx, Ty, blank = 4, 40, 120, -1.0
    value, tx, ty, _ = make_case(B, Tx, Ty)
    logp = torch.log_softmax(torch.from_numpy(value), 1)
    norm = torch.full((B, Tx + 1, Ty), -float("inf"))
    for b in range(B):
        norm[b, :tx[b] + 1] = torch.log_softmax(torch.cat([torch.full((1, Ty), blank), logp[b, :tx[b]]], 0).double(), 0).float()
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    loss, _ = objective.forward_sum(logp.to(dev), d_tx, d_ty, want_grad=False, blank_logprob=blank)
    res = align_with_pauses(norm[:, 1:].contiguous().to(dev), d_tx, d_ty, pause=norm[:, 0].contiguous().to(dev))
    score, ll = res.score.cpu().numpy().astype(np.float64), -loss.cpu().numpy().astype(np.float64)
    assert np.isfinite(score).all() and np.isfinite(ll).all()
    assert (score <= ll).all(), (score, ll)
    assert (score > ll - 0.5 * ty * np.log(2.0 * tx + 1)).all()       # ... and not absurdly far below it


def test_consumers_take_the_outputs_as_they_are(dev):
    B, Tx, Ty, C = 4, 65, 70, 3
    value, tx, ty, _ = make_case(B, Tx, Ty)
    logp = torch.log_softmax(torch.from_numpy(value), 1).to(dev)
    d_tx, d_ty = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    res = align_with_pauses(logp, d_tx, d_ty, pause=-4.0, want_state_durations=True)
    assert (res.tok <= -2).any()
    # the binarization loss counts the token frames only
    _, count = objective.bin_loss(logp, res.tok, d_ty)
    assert torch.equal(count, res.durations.sum(1).to(torch.int32))
    loss = objective.binarization_loss(logp, res.tok, d_ty)
    assert torch.isfinite(loss)
    # the regulator expands text encodings interleaved with a pause embedding
    h = torch.zeros(B, C, 2 * Tx + 1, device=dev)
    h[:, 0, 0::2] = 1.0                                              # channel 0 marks the pause embedding
    h[:, 1, :] = torch.arange(2 * Tx + 1, device=dev, dtype=torch.float32)
    out, rtok = objective.regulate(h, res.state_durations, Ty)
    frames = torch.arange(Ty, device=dev)[None, :] < d_ty[:, None]
    assert torch.equal(out[:, 0] == 1.0, (res.tok <= -2) & frames)
    state = torch.where(res.tok >= 0, 2 * res.tok + 1, 2 * (-2 - res.tok))
    assert torch.equal(out[:, 1][frames], state[frames].float())
    assert torch.equal(rtok[frames], state[frames].to(rtok.dtype))


BAND, CANARY = 4096, 0xA5


class Fenced:
    """nbytes of device memory with a canary band before and after it (as tests/test_guard_bands.py)."""

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


@pytest.mark.parametrize("B,Tx,Ty", [(3, 1, 1), (3, 7, 13), (4, 65, 70), (2, 257, 300), (2, 600, 1500)])
def test_writes_stay_inside_their_buffers(dev, B, Tx, Ty):
    lib = _lib.load()
    value, tx, ty, pz = make_case(B, Tx, Ty)
    tx, ty = tx.copy(), ty.copy()
    tx[-1] = 0                                                        # one utterance without a path
    v = torch.from_numpy(value).to(dev)
    d_tx, d_ty, d_pz = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev), torch.from_numpy(pz).to(dev)
    wsb = lib.aligner_pausepath_workspace_bytes(B, Tx, Ty)
    assert (wsb > 0) == (Tx == 600)
    ws = Fenced(wsb, dev)
    tok, dur, pauses = Fenced(B * Ty * 4, dev), Fenced(B * Tx * 4, dev), Fenced(B * (Tx + 1) * 4, dev)
    sdur, score = Fenced(B * (2 * Tx + 1) * 4, dev), Fenced(B * 4, dev)
    _lib.check(lib.aligner_pausepath(v.data_ptr(), _lib.DT_F32, Ty, d_pz.data_ptr(), 0.0, None, d_tx.data_ptr(), d_ty.data_ptr(),
                                     tok.ptr, dur.ptr, pauses.ptr, sdur.ptr, score.ptr, ws.ptr if wsb else None, wsb, B, Tx, Ty,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, f in (("workspace", ws), ("tok", tok), ("durations", dur), ("pauses", pauses), ("state_durations", sdur),
                    ("score", score)):
        assert f.intact(), f"{name}: the kernel wrote outside its buffer"
    want = PO.pause_align(value, tx, ty, pz)
    got = (tok.view(torch.int32, (B, Ty)), dur.view(torch.int32, (B, Tx)), pauses.view(torch.int32, (B, Tx + 1)),
           sdur.view(torch.int32, (B, 2 * Tx + 1)), score.view(torch.float32, (B,)))
    check(tuple(t.cpu().numpy() for t in got), want, tx, ty, what="fenced")
    # a too small workspace is refused, not overrun
    if wsb:
        rc = lib.aligner_pausepath(v.data_ptr(), _lib.DT_F32, Ty, None, -1.0, None, d_tx.data_ptr(), d_ty.data_ptr(), tok.ptr,
                                   None, None, None, None, ws.ptr, wsb - 4, B, Tx, Ty, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.ENOSPC


def test_single_outputs_and_empty_batches(dev):
    value, tx, ty, _ = make_case(4, 20, 33)
    v, d_tx, d_ty = torch.from_numpy(value).to(dev), torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    want = PO.pause_align(value, tx, ty, 0.5)
    flags = ("want_tok", "want_durations", "want_pauses", "want_state_durations", "want_score")
    for i, name in enumerate(flags):
        res = align_with_pauses(v, d_tx, d_ty, 0.5, **{f: f == name for f in flags})
        assert [t is not None for t in res] == [f == name for f in flags]
        assert np.array_equal(res[i].cpu().numpy(), want[i])
    with pytest.raises(ValueError):
        align_with_pauses(v, d_tx, d_ty, 0.5, **{f: False for f in flags})
    res = align_with_pauses(v[:0], d_tx[:0], d_ty[:0], 0.5, want_state_durations=True)
    assert [tuple(t.shape) for t in res] == [(0, 33), (0, 20), (0, 21), (0, 41), (0,)]
    res = align_with_pauses(v[:, :0], d_tx * 0, d_ty, 0.5, want_state_durations=True)         # no token: no path
    assert (res.tok == -1).all() and (res.score == -float("inf")).all() and tuple(res.pauses.shape) == (4, 1)
    assert not res.pauses.any() and not res.state_durations.any()
    with pytest.raises(ValueError):
        align_with_pauses(torch.zeros(1, 1025, 1030, device=dev), d_tx[:1], d_ty[:1])
