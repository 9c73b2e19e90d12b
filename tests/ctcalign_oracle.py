"""Float32 numpy restatement of CTC forced alignment (aligner_ctc_align, include/aligner_amd.h), and a brute-force
enumerator for tiny shapes.  The spec is build-defined; in the style of pausepath_oracle.py, whose search this is with
two changes: scores come from emissions e[y, v] through the labels, and between two equal labels the blank is mandatory.

States of an utterance: s = 0 .. 2 t_x; s = 2g is the blank in gap g (the place before token g; gap 0 leads, gap t_x
trails) and scores e[y, blank], s = 2x+1 is token x and scores e[y, lab[x]].  Moves: stay, advance s-1 -> s, and skip
s-2 -> s only into a token x >= 1 with lab[x] != lab[x-1].  Every token takes at least one frame, a blank zero or more.

Band: with r[x] = 1 if x >= 1 and lab[x] == lab[x-1] else 0, R[x] = r[0] + .. + r[x], Rt = R[t_x-1]:
token x exists at y iff x + R[x] <= y and t_y-1-y >= (t_x-1-x) + (Rt - R[x]); blank g iff g + (R[g-1] if g >= 1 else 0)
<= y and t_y-1-y >= (t_x-g) + (Rt - R[g] if g < t_x else 0).  Q[s,0] = score(s,0) for the states 0 and 1 that exist; for
y > 0, Q[s,y] = Q[pred,y-1] + score(s,y) (one fp32 add) with pred among the candidates that EXIST at y-1 in the order
stay, advance, skip: the first present one is taken and a later one replaces it only if strictly greater (ties keep the
earlier, a NaN never replaces anything).  The path ends in 2 t_x - 1 unless the trailing blank exists at t_y-1 and is
strictly greater.  No path: t_x < 1, t_y < 1, t_x + Rt > t_y, a length outside [0,L] / [0,T], a label outside [0,V).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class CtcResult(NamedTuple):
    tok: np.ndarray               # [T] int32: x, -2-g on a blank frame of gap g, -1 for y >= t_y
    labels: np.ndarray            # [T] int32: lab[x] / blank, -1 for y >= t_y
    frame_scores: np.ndarray      # [T] fp32: e[y, labels[y]], 0 for y >= t_y
    durations: np.ndarray         # [L] int32
    pauses: np.ndarray            # [L+1] int32
    state_durations: np.ndarray   # [2 L + 1] int32
    score: np.float32
    states: np.ndarray            # [t_y] int32 state per frame (empty when infeasible)


def repeats(lab: np.ndarray):
    """(r, R): r[x] = 1 where lab[x] == lab[x-1], and its inclusive prefix sum."""
    lab = np.asarray(lab)
    r = np.zeros(len(lab), np.int64)
    r[1:] = lab[1:] == lab[:-1]
    return r, np.cumsum(r)


def feasible(lab_row: np.ndarray, t_x: int, t_y: int, L: int, T: int, V: int) -> bool:
    """lab_row: the utterance's whole target row [L] (only [:t_x] is looked at)."""
    t_x, t_y = int(t_x), int(t_y)
    if not (1 <= t_x <= L and 1 <= t_y <= T):
        return False
    lab = np.asarray(lab_row)[:t_x]
    if ((lab < 0) | (lab >= V)).any():
        return False
    return t_x + int(repeats(lab)[1][-1]) <= t_y


def _outputs(states, score, e, lab, blank, L, T) -> CtcResult:
    tok = np.full(T, -1, np.int32)
    labels = np.full(T, -1, np.int32)
    fs = np.zeros(T, np.float32)
    sd = np.zeros(2 * L + 1, np.int32)
    n = len(states)
    if n:
        tok[:n] = np.where(states & 1, states >> 1, -2 - (states >> 1))
        labels[:n] = np.where(states & 1, lab[np.minimum(states >> 1, len(lab) - 1)], blank)
        fs[:n] = e[np.arange(n), labels[:n]]
        np.add.at(sd, states, 1)
    return CtcResult(tok, labels, fs, sd[1::2].copy(), sd[0::2].copy(), sd, np.float32(score), states.astype(np.int32))


def ctc_align_one(e: np.ndarray, targets: np.ndarray, t_x: int, t_y: int, blank: int = 0) -> CtcResult:
    """One utterance: e [T,V] (any float dtype numpy holds; up-cast to fp32), targets [L] integers."""
    T, V = e.shape
    L = len(targets)
    t_x, t_y = int(t_x), int(t_y)
    if not feasible(targets, t_x, t_y, L, T, V):
        return _outputs(np.zeros(0, np.int64), -np.inf, None, None, blank, L, T)
    e = np.asarray(e, np.float32)
    lab = np.asarray(targets)[:t_x].astype(np.int64)
    r, R = repeats(lab)
    Rt = int(R[-1])
    S = 2 * t_x + 1
    s = np.arange(S)
    is_tok = (s & 1) == 1
    x = np.arange(t_x)
    g = np.arange(t_x + 1)
    lo = np.empty(S, np.int64)
    hi = np.empty(S, np.int64)
    lo[1::2] = x + R
    hi[1::2] = t_y - 1 - (t_x - 1 - x) - (Rt - R)
    Rbefore = np.concatenate([[0], R])                      # R[g-1], 0 for g = 0
    Rat = np.concatenate([R, [Rt]])                         # R[g], Rt for g = t_x
    lo[0::2] = g + Rbefore
    hi[0::2] = t_y - 1 - (t_x - g) - (Rt - Rat)
    skip_ok = np.zeros(S, bool)
    skip_ok[1::2] = (x >= 1) & (r == 0)

    def exists(y):
        return (lo <= y) & (y <= hi)

    def scores(y):
        sc = np.empty(S, np.float32)
        sc[0::2] = e[y, blank]
        sc[1::2] = e[y, lab]
        return sc

    Q = np.zeros(S, np.float32)
    ex = exists(0)
    assert not ex[2:].any()
    Q[ex] = scores(0)[ex]
    dec = np.zeros((t_y, S), np.int8)
    with np.errstate(all="ignore"):
        for y in range(1, t_y):
            e_prev, ex = ex, exists(y)
            best = Q.copy()
            have = e_prev.copy()
            d = np.zeros(S, np.int8)
            # advance s-1
            c = np.empty(S, np.float32); c[1:] = Q[:-1]; c[0] = 0
            pres = np.zeros(S, bool); pres[1:] = e_prev[:-1]
            take = pres & (~have | (c > best))
            best = np.where(take, c, best); d[take] = 1; have |= pres
            # skip s-2: token -> token over an empty gap, unless the two labels are equal
            c = np.empty(S, np.float32); c[2:] = Q[:-2]; c[:2] = 0
            pres = np.zeros(S, bool); pres[2:] = e_prev[:-2]; pres &= skip_ok
            take = pres & (~have | (c > best))
            best = np.where(take, c, best); d[take] = 2; have |= pres
            assert have[ex].all(), "an in-band cell without a present candidate"
            Q = np.where(ex, (best + scores(y)).astype(np.float32), np.float32(0))
            dec[y] = d
    end = 2 * t_x - 1
    assert ex[end]
    if ex[2 * t_x] and Q[2 * t_x] > Q[end]:
        end = 2 * t_x
    states = np.zeros(t_y, np.int64)
    cur = end
    for y in range(t_y - 1, -1, -1):
        states[y] = cur
        cur -= int(dec[y, cur])
    return _outputs(states, Q[end], e, lab, blank, L, T)


def ctc_align(log_probs, targets, t_ys, t_xs, blank: int = 0):
    """A batch: log_probs [B,T,V], targets [B,L], input lengths t_ys and target lengths t_xs [B].  Returns the stacked
    outputs (tok, labels, frame_scores, durations, pauses, state_durations, score) as numpy arrays."""
    res = [ctc_align_one(log_probs[b], targets[b], t_xs[b], t_ys[b], blank) for b in range(len(log_probs))]
    return (np.stack([r.tok for r in res]), np.stack([r.labels for r in res]), np.stack([r.frame_scores for r in res]),
            np.stack([r.durations for r in res]), np.stack([r.pauses for r in res]),
            np.stack([r.state_durations for r in res]), np.array([r.score for r in res], np.float32))


def state_scores(e: np.ndarray, lab: np.ndarray, states: np.ndarray, blank: int) -> np.ndarray:
    st = np.asarray(states)
    col = np.where(st & 1, np.asarray(lab)[np.minimum(st >> 1, len(lab) - 1)], blank)
    return np.asarray(e, np.float32)[np.arange(len(st)), col]


def path_score(e: np.ndarray, lab: np.ndarray, states: np.ndarray, blank: int) -> np.float32:
    """fp32 left-to-right sum of the emissions along a path of states."""
    acc = None
    with np.errstate(all="ignore"):
        for sc in state_scores(e, lab, states, blank):
            acc = sc if acc is None else np.float32(acc + sc)
    return acc


def states_from_tok(tok: np.ndarray, t_y: int) -> np.ndarray:
    t = np.asarray(tok[:t_y]).astype(np.int64)
    return np.where(t >= 0, 2 * t + 1, 2 * (-2 - t))


def is_legal_states(st: np.ndarray, lab: np.ndarray) -> bool:
    t_x = len(lab)
    st = np.asarray(st).astype(np.int64)
    if len(st) == 0 or st[0] not in (0, 1) or st[-1] not in (2 * t_x - 1, 2 * t_x) or st.min() < 0 or st.max() > 2 * t_x:
        return False
    step = np.diff(st)
    if ((step < 0) | (step > 2)).any():
        return False
    sk = np.nonzero(step == 2)[0]
    if ((st[sk] & 1) == 0).any():                                    # a skip leaves a token ...
        return False
    xs = st[sk + 1] >> 1                                             # ... and enters token x with lab[x] != lab[x-1]
    if (np.asarray(lab)[xs] == np.asarray(lab)[xs - 1]).any():
        return False
    return len(set(st[(st & 1) == 1].tolist())) == t_x


def is_legal(tok: np.ndarray, lab: np.ndarray, t_x: int, t_y: int) -> bool:
    """Monotone over the CTC topology with the repeat rule (no skip between equal labels), starts in state 0 or 1, ends
    in 2 t_x - 1 or 2 t_x, every token present, -1 exactly on the frames past t_y."""
    if (np.asarray(tok[t_y:]) != -1).any() or (np.asarray(tok[:t_y]) == -1).any():
        return False
    return is_legal_states(states_from_tok(tok, t_y), np.asarray(lab)[:t_x])


def brute_force(e: np.ndarray, lab: np.ndarray, t_y: int, blank: int = 0):
    """Every legal path of a tiny utterance (lab: its t_x labels): (best fp32 left-to-right score, list of the state
    sequences reaching it); (None, []) when there is no legal path."""
    e = np.asarray(e, np.float32)
    lab = np.asarray(lab)
    t_x = len(lab)
    S = 2 * t_x + 1
    best, arg = None, []
    if t_x < 1 or t_y < 1:
        return best, arg

    def extend(seq):
        nonlocal best, arg
        if len(seq) == t_y:
            if seq[-1] in (2 * t_x - 1, 2 * t_x):
                sc = path_score(e, lab, np.array(seq), blank)
                if best is None or sc > best:
                    best, arg = sc, [tuple(seq)]
                elif sc == best:
                    arg.append(tuple(seq))
            return
        a = seq[-1]
        for c in (a, a + 1, a + 2):
            if c >= S:
                continue
            if c == a + 2 and (not (a & 1) or lab[c >> 1] == lab[(c >> 1) - 1]):
                continue
            extend(seq + [c])

    for first in (0, 1):
        extend([first])
    return best, arg
