"""An independent restatement of forced alignment (include/basic_pitch_amd_align.h) and the cases both align test files use.
The restatement is numpy in int64: the quantised maps times the 0 / 1 matrices of the states give the gains, the recurrence
runs over all states at once with "unreachable" a boolean beside the number, and the backtrace follows the stored decisions
(none of the library's code).  `best_by_enumeration` is a second yardstick: EVERY monotone path of a small problem, its total
summed cell by cell, the winner picked by the header's tie rule.  The maps, the state lists and the planted problems come from
seeded generators."""
import itertools

import numpy as np

PITCHES = 88
FREE = 2**31 - 1
STATE = np.dtype([("active", np.uint64, (2,)), ("begins", np.uint64, (2,)), ("earliest", np.int32), ("latest", np.int32)])
DEFAULT = dict(threshold_q=307, onset_weight=2)
F = np.float32


def quantise(x):
    x = np.asarray(x, np.float32)
    return np.floor(np.minimum(np.maximum(x, F(0.0)), F(1.0)) * F(1024.0) + F(0.5)).astype(np.int64)


def make_states(active, begins=None, earliest=None, latest=None):
    """STATE records from lists of pitch sets (indices 0 ... 87)."""
    n = len(active)
    st = np.zeros(n, STATE)
    st["latest"] = FREE
    for j in range(n):
        for field, sets in (("active", active), ("begins", begins)):
            for p in (sets[j] if sets is not None else ()):
                st[field][j, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    if earliest is not None:
        st["earliest"] = earliest
    if latest is not None:
        st["latest"] = latest
    return st


def rolls(states):
    """(S, 88) 0 / 1 matrices of active and begins."""
    out = []
    for field in ("active", "begins"):
        m = np.zeros((len(states), PITCHES), np.int64)
        for p in range(PITCHES):
            m[:, p] = (states[field][:, p >> 6] >> np.uint64(p & 63)) & np.uint64(1)
        out.append(m)
    return out


def gains(note, onset, states, threshold_q=307, onset_weight=2):
    act, beg = rolls(states)
    g = quantise(note).reshape(-1, PITCHES) @ act.T - threshold_q * act.sum(axis=1)[None, :]
    b = onset_weight * (quantise(onset).reshape(-1, PITCHES) @ beg.T)
    return g, b


def restate(note, onset, states, **fields):
    """(first_frame int32 per state, total, status)."""
    p = dict(DEFAULT, **fields)
    note, onset = np.asarray(note, np.float32).reshape(-1, PITCHES), np.asarray(onset, np.float32).reshape(-1, PITCHES)
    rows, S = len(note), len(states)
    ff = np.full(S, -1, np.int32)
    if np.isnan(note).any() or np.isnan(onset).any():
        return ff, 0, 1
    if S == 0:
        return ff, 0, 0
    if S > rows:
        return ff, 0, 2
    g, b = gains(note, onset, states, **p)
    early, late = states["earliest"].astype(np.int64), states["latest"].astype(np.int64)
    D, ok = np.zeros(S, np.int64), np.zeros(S, bool)
    D[0], ok[0] = g[0, 0] + b[0, 0], early[0] <= 0
    entered = np.zeros((rows, S), bool)
    for t in range(1, rows):
        stay = D + g[t]
        enter = np.concatenate([[0], D[:-1]]) + g[t] + b[t]
        can = np.concatenate([[False], ok[:-1]]) & (early <= t) & (t <= late)
        take = can & (~ok | (enter > stay))
        D, ok = np.where(take, enter, stay), ok | can
        entered[t] = take
    if not ok[S - 1]:
        return ff, 0, 2
    j = S - 1
    for t in range(rows - 1, 0, -1):
        if j > 0 and entered[t, j]:
            ff[j] = t
            j -= 1
    assert j == 0
    ff[0] = 0
    return ff, int(D[S - 1]), 0


def best_by_enumeration(note, onset, states, **fields):
    """Every monotone path of a small problem: (first_frame, total, status) of the best one under the header's tie rule —
    the smallest first_frame[S - 1], then the smallest first_frame[S - 2], and so on.  No recurrence: sums over cells."""
    p = dict(DEFAULT, **fields)
    note = np.asarray(note, np.float32).reshape(-1, PITCHES)
    rows, S = len(note), len(states)
    g, b = gains(note, onset, states, **p)
    best = None
    for inner in itertools.combinations(range(1, rows), S - 1):
        f = (0,) + inner
        if states["earliest"][0] > 0 or any(not (states["earliest"][j] <= f[j] <= states["latest"][j]) for j in range(1, S)):
            continue
        ends = f[1:] + (rows,)
        total = sum(int(g[f[j]:ends[j], j].sum()) + int(b[f[j], j]) for j in range(S))
        key = (-total,) + tuple(reversed(f))
        if best is None or key < best[0]:
            best = (key, f, total)
    if best is None:
        return np.full(S, -1, np.int32), 0, 2
    return np.array(best[1], np.int32), best[2], 0


# ---- generators
def random_maps(rng, rows, kind="thousand"):
    """(note, onset): `eighths` — multiples of 1/8, so that ties are frequent; `thousand` — a thousand levels, some of them
    outside 0 ... 1 so that the clamp is used."""
    if kind == "eighths":
        draw = lambda: (rng.integers(0, 9, (rows, PITCHES)) / 8.0).astype(np.float32)  # noqa: E731
    else:
        draw = lambda: (rng.integers(-50, 1051, (rows, PITCHES)) / 1000.0).astype(np.float32)  # noqa: E731
    return draw(), draw()


def random_states(rng, S, rows=None, windows=False, most=4):
    """S states of up to `most` pitches with begins a random subset; windows: some states held to a window around the frame a
    uniform spread would give them (feasible for rows >= S, though not always wide enough to be slack)."""
    active, begins = [], []
    for _ in range(S):
        a = sorted(rng.choice(PITCHES, int(rng.integers(0, most + 1)), replace=False).tolist())
        active.append(a)
        begins.append([p for p in a if rng.integers(0, 2)])
    st = make_states(active, begins)
    if windows and rows is not None and rows >= S:
        for j in range(1, S):
            if rng.integers(0, 3) == 0:
                mid = j * rows // S
                st["earliest"][j] = max(0, mid - int(rng.integers(0, 6)))
                st["latest"][j] = min(rows - 1, mid + int(rng.integers(0, 6)))
    return st


def planted(seed, max_states=69, max_rows=470):
    """A planted problem: (note, onset, states, first_frame).  A random state list — notes start, end and repeat on the same
    pitch; adjacent states differ in their set or carry a `begins` — and random cut points; the note map is 0.8 on the state's
    active pitches and 0.1 elsewhere, the onset map 0.8 on `begins` at the entry frame and 0.1 elsewhere, uniform noise of
    +-0.05 on every cell."""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, max_states + 1))
    rows = int(rng.integers(S, max(S, max_rows) + 1))
    sounding, active, begins = set(), [], []
    for _ in range(S):
        while True:
            now, beg = set(sounding), set()
            for p in list(now):
                r = rng.integers(0, 6)
                if r == 0:
                    now.discard(p)      # the note ends
                elif r == 1:
                    beg.add(p)          # it is struck again
            for p in rng.choice(PITCHES, int(rng.integers(0, 3)), replace=False).tolist():
                if p not in now:
                    now.add(p)
                    beg.add(p)          # a note starts
            if not active or now != sounding or beg:
                break
        sounding = now
        active.append(sorted(now))
        begins.append(sorted(beg))
    f = np.concatenate([[0], np.sort(rng.choice(np.arange(1, rows), S - 1, replace=False))]).astype(np.int32) if S > 1 else np.zeros(1, np.int32)
    note = np.full((rows, PITCHES), 0.1)
    onset = np.full((rows, PITCHES), 0.1)
    ends = np.concatenate([f[1:], [rows]])
    for j in range(S):
        note[f[j]:ends[j], active[j]] = 0.8
        onset[f[j], begins[j]] = 0.8
    note += rng.uniform(-0.05, 0.05, note.shape)
    onset += rng.uniform(-0.05, 0.05, onset.shape)
    return note.astype(np.float32), onset.astype(np.float32), make_states(active, begins), f


def stack(segs):
    """[(note, onset, states)] -> (row_offsets, note, onset, state_offsets, states)."""
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in segs])]).astype(np.int64)
    s_offs = np.concatenate([[0], np.cumsum([len(s[2]) for s in segs])]).astype(np.int64)
    cat = lambda k, width: np.ascontiguousarray(np.concatenate([np.asarray(s[k], np.float32).reshape(-1, width) for s in segs]))  # noqa: E731
    states = np.ascontiguousarray(np.concatenate([s[2] for s in segs]), STATE)
    return offs, cat(0, PITCHES), cat(1, PITCHES), s_offs, states
