"""CTC forced alignment, the parts that need no GPU: the numpy oracle (tests/ctcalign_oracle.py) against brute-force
enumeration of every legal path, against pausepath_oracle where the labels are pairwise distinct, on tight shapes with
a single legal path; the C ABI's argument checks; the Python entry point's argument checks."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ctcalign_oracle as CO
import pausepath_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_MAX, T_MAX = 4, 7


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("V", [2, 3, 4])
def test_oracle_equals_brute_force(V, quantised):
    """Every shape t_x <= 4, t_y <= 7 (0 included), every blank id; labels drawn from the V entries, so repeats are
    common at V = 2.  Half-quantised scores force ties: the oracle's path is then one of the maximisers."""
    n = n_rep = n_inf = n_tied = 0
    for blank in range(V):
        for t_x, t_y in itertools.product(range(0, L_MAX + 1), range(0, T_MAX + 1)):
            rng = np.random.default_rng(10000 * V + 1000 * blank + 10 * t_x + t_y + (5 if quantised else 0))
            e = rng.standard_normal((T_MAX, V)).astype(np.float32)
            if quantised:
                e = (np.round(2.0 * e) / 2.0).astype(np.float32)
            tg = rng.integers(0, V, L_MAX)
            res = CO.ctc_align_one(e, tg, t_x, t_y, blank)
            best, arg = CO.brute_force(e[:t_y], tg[:t_x], t_y, blank)
            n += 1
            if best is None:                                   # "no path" exactly where the enumeration is empty
                n_inf += 1
                assert len(res.states) == 0 and res.score == -np.inf and (res.tok == -1).all() and (res.labels == -1).all()
                assert not res.durations.any() and not res.pauses.any() and not res.state_durations.any() and not res.frame_scores.any()
                assert not CO.feasible(tg, t_x, t_y, L_MAX, T_MAX, V)
                continue
            assert CO.feasible(tg, t_x, t_y, L_MAX, T_MAX, V)
            assert res.score == best, (V, blank, t_x, t_y)
            assert tuple(res.states) in arg, (V, blank, t_x, t_y)
            n_tied += len(arg) > 1
            n_rep += bool((tg[1:t_x] == tg[:t_x - 1]).any())
            assert CO.is_legal(res.tok, tg, t_x, t_y)
            assert res.durations.sum() + res.pauses.sum() == t_y and (res.durations[:t_x] >= 1).all()
            assert np.array_equal(res.state_durations[1::2], res.durations) and np.array_equal(res.state_durations[0::2], res.pauses)
            assert CO.path_score(e, tg[:t_x], res.states, blank) == res.score
            lab_of = np.where(res.tok[:t_y] >= 0, tg[np.clip(res.tok[:t_y], 0, L_MAX - 1)], blank)
            assert np.array_equal(res.labels[:t_y], lab_of) and np.array_equal(res.frame_scores[:t_y], e[np.arange(t_y), lab_of])
    assert n == V * (L_MAX + 1) * (T_MAX + 1) and n_inf > n // 4 and n_rep >= 8
    assert n_tied >= 8 if quantised else True


def test_oracle_equals_pausepath_oracle_on_distinct_labels():
    """Pairwise distinct labels: no skip is forbidden, the bands are the pause search's, and the search is
    pause_align_one on the gathered scores with the blank column as the pause row -- states and score, bit for bit."""
    rng = np.random.default_rng(3)
    for it in range(60):
        V = 9
        L = int(rng.integers(1, 8))
        T = int(rng.integers(L, 24))
        blank = int(rng.integers(0, V))
        e = rng.standard_normal((T, V)).astype(np.float32)
        if it % 3 == 0:
            e = np.round(e).astype(np.float32)
        tg = rng.permutation(V)[:L]
        t_x = int(rng.integers(1, L + 1))
        t_y = int(rng.integers(t_x, T + 1))
        got = CO.ctc_align_one(e, tg, t_x, t_y, blank)
        want = PO.pause_align_one(np.ascontiguousarray(e[:, tg].T), t_x, t_y, pause=e[:, blank])
        assert np.array_equal(got.states, want.states) and got.score.tobytes() == want.score.tobytes()
        for name in ("tok", "durations", "pauses", "state_durations"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name


@pytest.mark.parametrize("scores", ["random", "nan", "minus_inf", "mixed"])
def test_tight_shapes_have_one_path_whatever_the_scores(scores):
    """t_y == t_x + Rt: every token takes one frame and a blank frame stands between equal labels, nothing else."""
    rng = np.random.default_rng(11)
    for t_x in range(1, 9):
        V = 3
        tg = rng.integers(0, V, t_x)
        r, R = CO.repeats(tg)
        t_y = t_x + int(R[-1])
        e = rng.standard_normal((t_y + 2, V)).astype(np.float32)
        if scores == "nan":
            e[:] = np.nan
        elif scores == "minus_inf":
            e[:] = -np.inf
        elif scores == "mixed":
            e[::2] = np.nan
            e[1::3, 0] = -np.inf
        want = []
        for x in range(t_x):
            if r[x]:
                want.append(2 * x)
            want.append(2 * x + 1)
        res = CO.ctc_align_one(e, tg, t_x, t_y, blank=1)
        assert res.states.tolist() == want and CO.is_legal(res.tok, tg, t_x, t_y)
        assert (res.durations[:t_x] == 1).all() and np.array_equal(res.pauses[:t_x], r) and res.pauses[t_x] == 0
        # one frame fewer: no path
        short = CO.ctc_align_one(e, tg, t_x, t_y - 1, blank=1)
        assert len(short.states) == 0 and short.score == -np.inf


def test_oracle_no_path_cases_and_blank_as_a_label():
    rng = np.random.default_rng(5)
    e = rng.standard_normal((9, 4)).astype(np.float32)
    tg = np.array([1, 2, 2, 3, 0], np.int64)
    assert len(CO.ctc_align_one(e, tg, 4, 5, 0).states) == 5           # 4 labels + 1 repeat
    for t_x, t_y in [(0, 5), (3, 0), (4, 4), (6, 9), (3, 10), (-1, 4)]:
        r = CO.ctc_align_one(e, tg, t_x, t_y, 0)
        assert (r.tok == -1).all() and (r.labels == -1).all() and not r.frame_scores.any() and r.score == -np.inf
    for bad in (4, -1, 1 << 20):
        t = tg.copy()
        t[1] = bad
        assert CO.ctc_align_one(e, t, 3, 9, 0).score == -np.inf
        assert np.isfinite(CO.ctc_align_one(e, t, 1, 9, 0).score)      # (a bad label past t_x is never looked at)
    # a label equal to the blank id is an ordinary token that scores the blank column
    r = CO.ctc_align_one(e, tg, 5, 9, 0)
    assert CO.is_legal(r.tok, tg, 5, 9) and (r.labels[r.tok == 4] == 0).all() and (r.tok == 4).sum() >= 1


def _declared_symbols():
    with open(os.path.join(ROOT, "include", "aligner_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(aligner_[a-z0-9_]+)\s*\(", text))


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared_symbols()
    for name in ("aligner_ctc_align", "aligner_ctc_align_workspace_bytes"):
        assert name in names and hasattr(raw, name) and name in _lib.SIGNATURES
    assert names == set(_lib.SIGNATURES)
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    # decision words in LDS: no workspace; beyond it, three words per row and 32-frame tile; 0 for an unsupported shape
    assert lib.aligner_ctc_align_workspace_bytes(1, 1025, 2000) == 0
    assert lib.aligner_ctc_align_workspace_bytes(64, 200, 1000) == 0
    assert lib.aligner_ctc_align_workspace_bytes(2, 600, 1500) == 2 * 47 * 3 * 601 * 4 > 0
    assert lib.aligner_ctc_align_workspace_bytes(1, 0, 5) == 0

    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data

    def call(lp=p, dtype=_lib.DT_F32, stride_b=64, stride_t=8, V=8, blank=0, targets=p, tx=p, ty=p, tok=p, B=1, L=4, T=8):
        return lib.aligner_ctc_align(lp, dtype, stride_b, stride_t, V, blank, targets, tx, ty, tok, None, None, None, None,
                                     None, None, None, 0, B, L, T, None)
    # validated before any HIP call: none of these looks for a device
    assert call(lp=None) == _lib.EINVAL and b"null" in lib.aligner_last_error()
    assert call(targets=None) == _lib.EINVAL and call(tx=None) == _lib.EINVAL and call(ty=None) == _lib.EINVAL
    assert call(tok=None) == _lib.EINVAL and b"no output" in lib.aligner_last_error()
    assert call(V=0, blank=0, stride_t=8) == _lib.EINVAL and b"V=0" in lib.aligner_last_error()
    assert call(blank=8) == _lib.EINVAL and b"blank=8" in lib.aligner_last_error()
    assert call(blank=-1) == _lib.EINVAL and b"blank=-1" in lib.aligner_last_error()
    assert call(stride_t=7) == _lib.EINVAL and b"stride_t=7" in lib.aligner_last_error()
    for dt in (_lib.DT_F64, _lib.DT_I32, 99):
        assert call(dtype=dt) == _lib.EINVAL and b"dtype" in lib.aligner_last_error()
    assert call(L=1025, T=2000) == _lib.EDOM and b"L=1025" in lib.aligner_last_error()
    assert call(B=65536) == _lib.EDOM and b"B=65536" in lib.aligner_last_error()
    assert call(stride_t=1 << 29, T=8) == _lib.EDOM and str(7 * (1 << 29) + 8).encode() in lib.aligner_last_error()
    assert call(B=60000, L=1024, T=400000, stride_t=8) == _lib.EDOM and b"decision words" in lib.aligner_last_error()
    # an empty batch is nothing to do
    assert call(B=0) == 0


def test_python_argument_checks_come_before_the_library(monkeypatch):
    import aligner_amd
    from aligner_amd import _lib, ctcalign
    assert callable(aligner_amd.ctc_forced_align) and callable(aligner_amd.ctc_token_spans)
    assert {"ctc_forced_align", "ctc_token_spans", "CtcAlignment"} <= set(aligner_amd.__all__)
    assert aligner_amd.CtcAlignment._fields == ("tok", "labels", "frame_scores", "durations", "pauses", "state_durations", "score")

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    lp = torch.zeros(2, 5, 4)
    tg = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        ctcalign.ctc_forced_align(lp, tg)
    with pytest.raises(ValueError, match=r"\[B, T, V\]"):
        ctcalign.ctc_forced_align(lp[0], tg)
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        ctcalign.ctc_forced_align(lp, tg[0])
    with pytest.raises(ValueError, match="integer"):
        ctcalign.ctc_forced_align(lp, tg.float())
    for blank in (4, -1):
        with pytest.raises(ValueError, match="blank"):
            ctcalign.ctc_forced_align(lp, tg, blank=blank)
    import inspect
    assert "oracle" not in inspect.getsource(ctcalign)
