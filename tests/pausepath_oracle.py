"""Float32 numpy restatement of the pause-aware hard search (aligner_pausepath, include/aligner_amd.h), and a
brute-force enumerator for tiny shapes.  The spec is build-defined (the reference snapshot holds no code for it).

States of an utterance: s = 0 .. 2 t_x; s = 2g is the pause in gap g (the place before token g; gap 0 leads, gap t_x
trails) and scores pause[y], s = 2x+1 is token x and scores value[x, y].  Every token takes at least one frame, a pause
zero or more; a gap whose mask is 0 holds no pause.

Band: token x exists at frame y iff x <= y and t_y-1-y >= t_x-1-x; pause g iff g <= y, t_y-1-y >= t_x-g and its gap
is allowed.  Q[s,0] = score(s,0) for the states 0 and 1 that exist; for y > 0, Q[s,y] = Q[pred,y-1] + score(s,y) (one
fp32 add) where pred is chosen among the candidates that EXIST at y-1, in the order stay s, advance s-1, and for
token states skip s-2: the first present one is taken and a later one replaces it only if its Q is strictly greater
(ties keep the earlier, a NaN never replaces anything).  The path ends in state 2 t_x - 1 unless the trailing pause
2 t_x exists at t_y-1 and is strictly greater; the backtrack follows the recorded choices.

One Python step per frame, vectorised over the states, so [200, 1000] takes well under a second.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np


class PauseResult(NamedTuple):
    tok: np.ndarray               # [Ty] int32: x, -2-g on a pause frame of gap g, -1 for y >= t_y
    durations: np.ndarray         # [Tx] int32
    pauses: np.ndarray            # [Tx+1] int32
    state_durations: np.ndarray   # [2 Tx + 1] int32
    score: np.float32
    states: np.ndarray            # [t_y] int32 state per frame (empty when infeasible)


def feasible(t_x: int, t_y: int, Tx: int, Ty: int) -> bool:
    return 1 <= t_x <= t_y and t_x <= Tx and t_y <= Ty


def _pause_row(pause, t_y: int) -> np.ndarray:
    if np.ndim(pause) == 0:
        return np.full(t_y, np.float32(pause), np.float32)
    return np.asarray(pause, np.float32)[:t_y]


def _outputs(states: np.ndarray, score, Tx: int, Ty: int) -> PauseResult:
    tok = np.full(Ty, -1, np.int32)
    sd = np.zeros(2 * Tx + 1, np.int32)
    if len(states):
        tok[:len(states)] = np.where(states & 1, states >> 1, -2 - (states >> 1))
        np.add.at(sd, states, 1)
    return PauseResult(tok, sd[1::2].copy(), sd[0::2].copy(), sd, np.float32(score), states.astype(np.int32))


def pause_align_one(value: np.ndarray, t_x: int, t_y: int, pause=-1.0, gap_mask: Optional[np.ndarray] = None) -> PauseResult:
    """One utterance: value [Tx,Ty] (any float dtype numpy holds; up-cast to fp32), pause a float or [Ty], gap_mask [Tx+1]."""
    Tx, Ty = value.shape
    t_x, t_y = int(t_x), int(t_y)
    if not feasible(t_x, t_y, Tx, Ty):
        return _outputs(np.zeros(0, np.int64), -np.inf, Tx, Ty)
    val = np.asarray(value, np.float32)
    pz = _pause_row(pause, t_y)
    S = 2 * t_x + 1
    s = np.arange(S)
    is_tok = (s & 1) == 1
    idx = s >> 1                                            # token x / gap g
    lo = idx                                                # first frame of the band
    hi = np.where(is_tok, t_y - t_x + idx, t_y - 1 - t_x + idx)
    allowed = np.ones(S, bool)
    if gap_mask is not None:
        allowed[0::2] = np.asarray(gap_mask)[:t_x + 1] != 0

    def exists(y):
        return allowed & (lo <= y) & (y <= hi)

    def scores(y):
        sc = np.empty(S, np.float32)
        sc[0::2] = pz[y]
        sc[1::2] = val[:t_x, y]
        return sc

    Q = np.zeros(S, np.float32)
    e = exists(0)
    assert not e[2:].any()
    Q[e] = scores(0)[e]
    dec = np.zeros((t_y, S), np.int8)
    with np.errstate(all="ignore"):
        for y in range(1, t_y):
            e_prev, e = e, exists(y)
            best = Q.copy()
            have = e_prev.copy()
            d = np.zeros(S, np.int8)
            # advance s-1
            c = np.empty(S, np.float32); c[1:] = Q[:-1]; c[0] = 0
            pres = np.zeros(S, bool); pres[1:] = e_prev[:-1]
            take = pres & (~have | (c > best))
            best = np.where(take, c, best); d[take] = 1; have |= pres
            # skip s-2: token -> token over an empty gap
            c = np.empty(S, np.float32); c[2:] = Q[:-2]; c[:2] = 0
            pres = np.zeros(S, bool); pres[2:] = e_prev[:-2]; pres &= is_tok
            take = pres & (~have | (c > best))
            best = np.where(take, c, best); d[take] = 2; have |= pres
            assert have[e].all(), "an in-band cell without a present candidate"
            Q = np.where(e, (best + scores(y)).astype(np.float32), np.float32(0))
            dec[y] = d
    end = 2 * t_x - 1
    if e[2 * t_x] and Q[2 * t_x] > Q[end]:
        end = 2 * t_x
    states = np.zeros(t_y, np.int64)
    cur = end
    for y in range(t_y - 1, -1, -1):
        states[y] = cur
        cur -= int(dec[y, cur])
    return _outputs(states, Q[end], Tx, Ty)


def pause_align(value, t_xs, t_ys, pause=-1.0, gap_mask=None):
    """A batch: value [B,Tx,Ty], pause a float or [B,Ty], gap_mask None or [B,Tx+1].  Returns the stacked outputs
    (tok, durations, pauses, state_durations, score) as numpy arrays."""
    res = [pause_align_one(value[b], t_xs[b], t_ys[b], pause if np.ndim(pause) == 0 else np.asarray(pause)[b],
                           None if gap_mask is None else np.asarray(gap_mask)[b]) for b in range(len(value))]
    return (np.stack([r.tok for r in res]), np.stack([r.durations for r in res]), np.stack([r.pauses for r in res]),
            np.stack([r.state_durations for r in res]), np.array([r.score for r in res], np.float32))


def path_score(value: np.ndarray, states: np.ndarray, pause) -> np.float32:
    """fp32 left-to-right sum of the scores along a path of states."""
    pz = _pause_row(pause, len(states))
    acc = None
    with np.errstate(all="ignore"):
        for y, st in enumerate(states):
            sc = np.float32(value[st >> 1, y]) if st & 1 else pz[y]
            acc = sc if acc is None else np.float32(acc + sc)
    return acc


def states_from_tok(tok: np.ndarray, t_y: int) -> np.ndarray:
    t = np.asarray(tok[:t_y]).astype(np.int64)
    return np.where(t >= 0, 2 * t + 1, 2 * (-2 - t))


def is_legal(tok: np.ndarray, t_x: int, t_y: int, gap_mask=None) -> bool:
    """Monotone over the CTC topology, starts in state 0 or 1, ends in 2 t_x - 1 or 2 t_x, every token present, pauses
    only in allowed gaps, -1 exactly on the frames past t_y."""
    if (np.asarray(tok[t_y:]) != -1).any() or (np.asarray(tok[:t_y]) == -1).any():
        return False
    st = states_from_tok(tok, t_y)
    if st[0] not in (0, 1) or st[-1] not in (2 * t_x - 1, 2 * t_x) or st.min() < 0 or st.max() > 2 * t_x:
        return False
    step = np.diff(st)
    if ((step < 0) | (step > 2)).any() or ((step == 2) & ((st[:-1] & 1) == 0)).any():
        return False
    if len(set(st[(st & 1) == 1].tolist())) != t_x:
        return False
    if gap_mask is not None and (np.asarray(gap_mask)[st[(st & 1) == 0] >> 1] == 0).any():
        return False
    return True


def brute_force(value: np.ndarray, t_x: int, t_y: int, pause=-1.0, gap_mask=None):
    """Every legal path of a tiny utterance: (best fp32 left-to-right score, list of the state sequences reaching it)."""
    val = np.asarray(value, np.float32)
    S = 2 * t_x + 1
    ok = np.ones(S, bool)
    if gap_mask is not None:
        ok[0::2] = np.asarray(gap_mask)[:t_x + 1] != 0
    best, arg = None, []

    def extend(seq):
        nonlocal best, arg
        if len(seq) == t_y:
            if seq[-1] in (2 * t_x - 1, 2 * t_x):
                sc = path_score(val, np.array(seq), pause)
                if best is None or sc > best:
                    best, arg = sc, [tuple(seq)]
                elif sc == best:
                    arg.append(tuple(seq))
            return
        a = seq[-1]
        for c in (a, a + 1, a + 2):
            if c < S and ok[c] and (c != a + 2 or a & 1):
                extend(seq + [c])

    for first in (0, 1):
        if ok[first]:
            extend([first])
    return best, arg
