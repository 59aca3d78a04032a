"""An independent restatement of the melody decode (include/basic_pitch_amd_melody.h) and the cases both melody test files
use.  The restatement is numpy in float32, one operation at a time: a loop over frames and, inside it, a loop over the
candidates IN THE HEADER'S ORDER, each taken where it is strictly greater than all before it (the targets side by side in an
array; none of the library's code).  The refinement is numpy float64 as the header writes it.  `best_total_by_enumeration` is
a second yardstick: every path of a small quantised problem, in exact arithmetic.  The case maps come from seeded
generators."""
import itertools

import numpy as np

BINS = 264
POINT = np.dtype([("bin", np.int32), ("salience", np.float32), ("pitch_midi", np.float64)])
DEFAULT = dict(threshold=0.3, jump_penalty=0.05, voicing_penalty=0.5, max_jump=4, min_bin=0, max_bin=263)
QUANTISED = dict(threshold=0.5, jump_penalty=0.125, voicing_penalty=0.25)
# the sets of the byte comparisons and of the scored sweep: the defaults, max_jump 0 / 1 / 16, a one-bin band, bands that
# touch bins 0 and 263, and the quantised map's own
SETS = (
    dict(),
    dict(max_jump=0, threshold=0.65),
    dict(max_jump=1, threshold=0.5),
    dict(max_jump=16, jump_penalty=0.01, threshold=0.6),
    dict(min_bin=100, max_bin=100, threshold=0.5, voicing_penalty=0.25),
    dict(min_bin=0, max_bin=40, threshold=0.85, voicing_penalty=0.125),
    dict(min_bin=200, max_bin=263, threshold=0.85, voicing_penalty=0.125),
    dict(QUANTISED),
)
F = np.float32
ROWS = (0, 1, 2, 65, 173, 433)


def params(**fields):
    return dict(DEFAULT, **fields)


def in_range(contour):
    c = np.asarray(contour, np.float32)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(c) <= F(65536.0)).all())


def restate_path(contour, tie="low", **fields):
    """(states per row with -1 for U, status).  tie "low": the header's rule.  "high": the opposite — a candidate replaces an
    equal one before it, so ties go to the highest bin and to U first."""
    p = params(**fields)
    c = np.asarray(contour, np.float32).reshape(-1, BINS)
    rows = len(c)
    path = np.full(rows, -1, np.int64)
    if not in_range(c):
        return path, 1
    if rows == 0:
        return path, 0
    thr, jp, vp = F(p["threshold"]), F(p["jump_penalty"]), F(p["voicing_penalty"])
    lo, hi, J = int(p["min_bin"]), int(p["max_bin"]), int(p["max_jump"])
    n = hi - lo + 1
    beats = (lambda a, b: a > b) if tie == "low" else (lambda a, b: a >= b)
    pen = [jp * F(d) for d in range(J + 1)]
    own = np.arange(n)
    D, Du = c[0, lo:hi + 1].copy(), thr
    pred = np.zeros((rows, n + 1), np.int64)  # the state before: 0 ... n - 1 a band bin, n the unvoiced state
    for t in range(1, rows):
        P, Pu = D - Du, Du - Du
        best, arg = np.full(n, -np.inf, np.float32), np.zeros(n, np.int64)
        for d in range(-J, J + 1):
            src = own + d
            ok = (src >= 0) & (src < n)
            cand = np.full(n, -np.inf, np.float32)
            cand[ok] = P[src[ok]] - pen[abs(d)]
            take = ok & beats(cand, best)
            best[take], arg[take] = cand[take], src[take]
        cand_u = Pu - vp
        take = beats(cand_u, best)
        best[take], arg[take] = cand_u, n
        to_u = P - vp
        a = int(np.argmax(to_u)) if tie == "low" else n - 1 - int(np.argmax(to_u[::-1]))
        best_u = to_u[a]
        if beats(Pu, best_u):
            best_u, a = Pu, n
        pred[t, :n], pred[t, n] = arg, a
        D, Du = c[t, lo:hi + 1] + best, thr + best_u
        assert D.dtype == np.float32 and Du.dtype == np.float32
    state = int(np.argmax(D)) if tie == "low" else n - 1 - int(np.argmax(D[::-1]))
    if beats(Du, D[state]):
        state = n
    for t in range(rows - 1, -1, -1):
        path[t] = -1 if state == n else lo + state
        state = int(pred[t, state])
    return path, 0


def records(contour, path):
    """The POINT records of a path (bins, -1 unvoiced) on its map: the cell, and the parabola where the cell is a strict
    local maximum of its row."""
    c = np.asarray(contour, np.float32).reshape(-1, BINS)
    out = np.zeros(len(path), POINT)
    out["bin"] = -1
    for t in np.flatnonzero(np.asarray(path) >= 0):
        b = int(path[t])
        delta = 0.0
        if 1 <= b <= BINS - 2 and c[t, b] > c[t, b - 1] and c[t, b] > c[t, b + 1]:
            l, m, r = (np.float64(c[t, b + k]) for k in (-1, 0, 1))
            delta = 0.5 * (l - r) / ((l - 2.0 * m) + r)
        out[t] = (b, c[t, b], 21.0 + (np.float64(b) + delta) / 3.0)
    return out


def restate(contour, **fields):
    """(POINT record per row, status)."""
    path, status = restate_path(contour, **fields)
    return records(contour, path), status


def path_total(contour, path, **fields):
    """The total of a path in float64: emissions minus penalties; None when it makes a jump above max_jump.  Exact when the
    cells and the parameters are multiples of 1/8."""
    p = params(**fields)
    c = np.asarray(contour, np.float64).reshape(-1, BINS)
    total = 0.0
    for t, s in enumerate(path):
        total += p["threshold"] if s < 0 else c[t, s]
        if t == 0:
            continue
        q = path[t - 1]
        if (s < 0) != (q < 0):
            total -= p["voicing_penalty"]
        elif s >= 0:
            if abs(s - q) > p["max_jump"]:
                return None
            total -= p["jump_penalty"] * abs(s - q)
    return total


def best_total_by_enumeration(contour, **fields):
    """The largest total over ALL paths of a small problem (a band of at most 4 bins, at most 5 rows)."""
    p = params(**fields)
    rows = len(contour)
    states = list(range(p["min_bin"], p["max_bin"] + 1)) + [-1]
    assert len(states) <= 5 and rows <= 5
    totals = [path_total(contour, path, **fields) for path in itertools.product(states, repeat=rows)]
    return max(t for t in totals if t is not None)


def restate_counts(points, ref_pitch, pitch_tolerance_cents=50.0, strict=0, **_):
    """(n_frames, ref_voiced, est_voiced, both_voiced, pitch_ok, chroma_ok) in numpy float64."""
    ref = np.asarray(ref_pitch, np.float64)
    rv, ev = ref != 0.0, points["bin"] >= 0
    both = rv & ev
    d = 100.0 * (ref[both] - points["pitch_midi"][both])
    cmp = (lambda x: x < pitch_tolerance_cents) if strict else (lambda x: x <= pitch_tolerance_cents)
    chroma = np.abs(d - 1200.0 * np.floor(d / 1200.0 + 0.5))
    return (len(ref), int(rv.sum()), int(ev.sum()), int(both.sum()), int(cmp(np.abs(d)).sum()), int(cmp(chroma).sum()))


# ---- the case maps
def glide(rng, rows, max_jump=4):
    """A gated voice whose centre moves by a uniform step of -(max_jump + 2) ... max_jump + 2 bins per row (reflected into bins
    30 ... 230), a weaker steady distractor, low noise."""
    b = np.arange(BINS, dtype=np.float64)[None, :]
    c = rng.uniform(0.0, 0.05, (rows, BINS))
    steps = rng.integers(-(max_jump + 2), max_jump + 3, rows)
    centre = np.zeros(rows)
    at = float(rng.integers(60, 200))
    for t in range(rows):
        at += steps[t]
        if at < 30 or at > 230:
            at -= 2 * steps[t]
        centre[t] = at
    gate = (np.arange(rows) // 24 + int(rng.integers(0, 2))) % 3 != 0  # two stretches on, one off
    c += (0.85 * gate)[:, None] * np.exp(-0.5 * ((b - centre[:, None]) / 1.2) ** 2)
    c += 0.25 * np.exp(-0.5 * ((b - float(rng.integers(40, 220))) / 1.5) ** 2)
    return c.astype(np.float32)


def noise(rng, rows):
    return rng.uniform(0.0, 1.0, (rows, BINS)).astype(np.float32)


def quantised(rng, rows):
    """Cells k / 8, k = 0 ... 8: with QUANTISED every sum is exact and ties are everywhere."""
    return (rng.integers(0, 9, (rows, BINS)) / 8.0).astype(np.float32)


def case_maps(rows, seed=0):
    """[(name, map)] of the three kinds at `rows` rows."""
    rng = np.random.default_rng(1000 * seed + rows)
    return [("glide", glide(rng, rows)), ("noise", noise(rng, rows)), ("quantised", quantised(rng, rows))]


def with_cell(contour, value, row, bin_):
    c = np.array(contour, np.float32, copy=True)
    c[row, bin_] = value
    return c


def stack(segs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    return offs, np.ascontiguousarray(np.concatenate(segs) if segs else np.zeros((0, BINS), np.float32), np.float32)


def ref_for(rng, points):
    """A reference track that makes every count non-trivial against a segment's own records: mostly the estimate's pitch,
    stretches of it 12 and 24 semitones off, half a semitone off (exactly at the default tolerance), a quarter tone more, with
    voicing flipped on some frames."""
    n = len(points)
    ref = np.where(points["bin"] >= 0, points["pitch_midi"], 0.0).astype(np.float64)
    kind = rng.integers(0, 10, n)
    voiced = ref > 0
    ref[voiced & (kind == 1)] += 12.0
    ref[voiced & (kind == 2)] += 24.0
    ref[voiced & (kind == 3)] += 0.5
    ref[voiced & (kind == 4)] += 0.75
    ref[voiced & (kind == 5)] = 0.0
    ref[~voiced & (kind == 6)] = 60.0
    return ref
