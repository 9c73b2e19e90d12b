"""Pause-aware hard search, the parts that need no GPU: the numpy oracle (tests/pausepath_oracle.py) against brute-force
enumeration and against the pinned search with every gap disallowed, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest

import pausepath_oracle as PO
from oracle import maxpath_oracle


def _case(t_x, t_y, seed):
    rng = np.random.default_rng(seed)
    return (2.0 * rng.standard_normal((t_x, t_y))).astype(np.float32)


@pytest.mark.parametrize("shift", [0.0, -1.0, -2.0])
@pytest.mark.parametrize("masked", [False, True])
def test_oracle_equals_brute_force(masked, shift):
    n = 0
    for t_x in range(1, 4):
        for t_y in range(t_x, 7):
            rng = np.random.default_rng(100 * t_x + t_y + (1000 if masked else 0))
            value = _case(t_x, t_y, 7 * t_x + t_y)
            pause = (rng.standard_normal(t_y) + shift).astype(np.float32)
            gm = rng.integers(0, 2, t_x + 1).astype(np.uint8) if masked else None
            res = PO.pause_align_one(value, t_x, t_y, pause, gm)
            best, arg = PO.brute_force(value, t_x, t_y, pause, gm)
            assert res.score == best, (t_x, t_y)
            assert len(arg) == 1 and tuple(res.states) == arg[0], (t_x, t_y)     # (continuous scores: no ties)
            assert PO.is_legal(res.tok, t_x, t_y, gm)
            assert res.durations.sum() + res.pauses.sum() == t_y and (res.durations >= 1).all()
            assert np.array_equal(res.state_durations[1::2], res.durations) and np.array_equal(res.state_durations[0::2], res.pauses)
            assert PO.path_score(value, res.states, pause) == res.score
            n += 1
    assert n == 15


@pytest.mark.parametrize("masked", [False, True])
def test_oracle_ties_keep_the_earlier_candidate(masked):
    """Integer scores and an integer pause: many paths share the best score.  The oracle's path is one of them, and it is
    the one the candidate order picks -- a frame-by-frame restatement of "stay, else advance, else skip; a later one only
    if strictly greater", written as a scalar loop, finds the same states."""
    n_tied = 0
    for t_x in range(1, 4):
        for t_y in range(t_x, 7):
            rng = np.random.default_rng(10 * t_x + t_y + (100 if masked else 0))
            value = rng.integers(0, 2, (t_x, t_y)).astype(np.float32)
            pause = rng.integers(0, 2, t_y).astype(np.float32)
            gm = rng.integers(0, 2, t_x + 1).astype(np.uint8) if masked else None
            res = PO.pause_align_one(value, t_x, t_y, pause, gm)
            best, arg = PO.brute_force(value, t_x, t_y, pause, gm)
            assert res.score == best and tuple(res.states) in arg
            n_tied += len(arg) > 1
            assert tuple(res.states) == _scalar_dp(value, t_x, t_y, pause, gm)
    assert n_tied >= 8


def _scalar_dp(value, t_x, t_y, pause, gm):
    S = 2 * t_x + 1

    def exists(s, y):
        g = s >> 1
        if s & 1:
            return g <= y and t_y - 1 - y >= t_x - 1 - g
        return g <= y and t_y - 1 - y >= t_x - g and (gm is None or gm[g] != 0)

    def score(s, y):
        return np.float32(value[s >> 1, y]) if s & 1 else np.float32(pause[y])
    Q = {s: score(s, 0) for s in (0, 1) if exists(s, 0)}
    back = []
    for y in range(1, t_y):
        Qn, bk = {}, {}
        for s in range(S):
            if not exists(s, y):
                continue
            pick = None
            for d in ((0, 1, 2) if s & 1 else (0, 1)):
                c = s - d
                if c >= 0 and c in Q and (pick is None or Q[c] > Q[s - pick]):
                    pick = d
            Qn[s], bk[s] = np.float32(Q[s - pick] + score(s, y)), pick
        Q = Qn
        back.append(bk)
    s = 2 * t_x - 1
    if 2 * t_x in Q and Q[2 * t_x] > Q[s]:
        s = 2 * t_x
    states = [s]
    for bk in reversed(back):
        s -= bk[s]
        states.append(s)
    return tuple(reversed(states))


def test_oracle_padding_scalar_pause_and_infeasible():
    value = _case(6, 12, 3)
    res = PO.pause_align_one(value, 4, 9, 0.5)
    assert PO.is_legal(res.tok, 4, 9) and (res.tok[9:] == -1).all() and (res.durations[4:] == 0).all() and (res.pauses[5:] == 0).all()
    assert (res.pauses > 0).any()
    for t_x, t_y in [(0, 5), (3, 0), (5, 4), (7, 9), (3, 13), (-1, 4)]:
        r = PO.pause_align_one(value, t_x, t_y, 0.5)
        assert (r.tok == -1).all() and not r.durations.any() and not r.pauses.any() and not r.state_durations.any()
        assert r.score == -np.inf


@pytest.mark.parametrize("t_x,t_y", [(1, 1), (5, 5), (7, 33), (30, 31), (64, 65), (65, 200)])
def test_oracle_without_gaps_is_the_pinned_search(t_x, t_y):
    value = _case(t_x, t_y, t_x * 1000 + t_y)
    res = PO.pause_align_one(value, t_x, t_y, 5.0, np.zeros(t_x + 1, np.uint8))
    tok, _ = maxpath_oracle.column_sweep(value, t_x, t_y)
    assert np.array_equal(res.tok, tok)
    assert not res.pauses.any() and np.array_equal(res.durations, np.bincount(tok, minlength=t_x))


def test_oracle_unusual_scores_give_a_legal_path():
    value = _case(5, 14, 1)
    value[1] = -np.inf
    value[3, 7] = np.nan
    for pause in (-1.0, -np.inf, np.nan):
        res = PO.pause_align_one(value, 5, 14, pause)
        assert PO.is_legal(res.tok, 5, 14)


def test_abi_symbols_and_argument_checks(built_lib):
    from aligner_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("aligner_pausepath", "aligner_pausepath_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = built_lib
    assert lib.aligner_abi_version() == 5
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def call(ld=8, Tx=4, Ty=8, tok=p, value=p, tx=p):
        return lib.aligner_pausepath(value, _lib.DT_F32, ld, None, -1.0, None, tx, p, tok, None, None, None, None,
                                     None, 0, 1, Tx, Ty, None)
    # validated before any HIP call: none of these looks for a device
    assert call(tok=None) == _lib.EINVAL and b"no output" in lib.aligner_last_error()
    assert call(ld=7) == _lib.EINVAL and b"ld_value" in lib.aligner_last_error()
    assert call(value=None) == _lib.EINVAL and call(tx=None) == _lib.EINVAL
    assert lib.aligner_pausepath_workspace_bytes(1, 1025, 2000) == 0
    assert call(ld=2000, Tx=1025, Ty=2000) == _lib.EDOM
    # decision words in LDS: no workspace; beyond it, three words per row and 32-frame tile
    assert lib.aligner_pausepath_workspace_bytes(64, 200, 1000) == 0
    assert lib.aligner_pausepath_workspace_bytes(2, 600, 1500) == 2 * 47 * 3 * 601 * 4
    assert lib.aligner_pausepath_workspace_bytes(1, 0, 5) == 0


def test_python_entry_point_is_exported_and_does_not_import_the_oracle():
    import aligner_amd
    assert callable(aligner_amd.align_with_pauses) and "align_with_pauses" in aligner_amd.__all__
    assert aligner_amd.PauseAlignment._fields == ("tok", "durations", "pauses", "state_durations", "score")
    import inspect
    from aligner_amd import pausepath
    assert "oracle" not in inspect.getsource(pausepath).replace("pausepath_oracle", "")
