"""Tempo and beats, restated (include/basic_pitch_amd_beat.h): an independent numpy int64 statement of the header's
definition, written from the header and not from csrc/beat_host.cpp, the enumeration of every beat sequence of small
problems, the seeded maps and parameter sets the CPU and GPU tests share, and the job of many segments of the GPU test."""
import itertools

import numpy as np

PITCHES = 88
MAX_LAG = 256
F = np.float32
SUMMARY = np.dtype([("status", np.int32), ("period", np.int32), ("n_beats", np.int64), ("score", np.int64), ("period_refined", np.float64)])
DEFAULT = dict(threshold_q=307, min_pitch=0, max_pitch=87, lag_min=21, lag_max=172, tightness=4)


def prior_table(start_bpm=120.0, sd_octaves=1.0):
    """The header's formula in numpy float64: entry L is rint(1024 * exp(-0.5 * (log2(L / L0) / sd)^2)), entry 0 is 0."""
    L0 = 60.0 * 22050.0 / 256.0 / start_bpm
    lags = np.arange(1, MAX_LAG + 1, dtype=np.float64)
    return np.concatenate([[0], np.rint(1024.0 * np.exp(-0.5 * (np.log2(lags / L0) / sd_octaves) ** 2))]).astype(np.int32)


FLAT = np.concatenate([[0], np.full(MAX_LAG, 1024)]).astype(np.int32)
# the parameter sets of the CPU and the GPU tests (fields on top of the defaults; "prior" absent: the default table)
PARAM_SETS = {
    "default": dict(),
    "narrow_band": dict(min_pitch=30, max_pitch=50, lag_min=30, lag_max=60, threshold_q=200),
    "tightness_0": dict(tightness=0),
    "tightness_1024": dict(tightness=1024),
    "one_lag": dict(lag_min=43, lag_max=43),
    "lag_max_256": dict(lag_max=MAX_LAG),
    "flat_prior": dict(prior=FLAT, threshold_q=0),
}


def full(fields):
    """A parameter set spelled out: the defaults, the fields on top, the table."""
    p = dict(DEFAULT, **{k: v for k, v in fields.items() if k != "prior"})
    p["prior"] = np.asarray(fields.get("prior", prior_table()), np.int64)
    return p


def quantise(x):
    """q(x) in float32, as the header writes it."""
    x = np.asarray(x, F)
    return np.floor(np.minimum(np.maximum(x, F(0.0)), F(1.0)) * F(1024.0) + F(0.5)).astype(np.int64)


def strength(onset, p):
    band = quantise(onset[:, p["min_pitch"] : p["max_pitch"] + 1]) - p["threshold_q"]
    return np.maximum(band, 0).sum(axis=1).astype(np.int64)


def none(status):
    return np.array([(status, 0, 0, 0, 0.0)], SUMMARY)


def tempo(o, p):
    """(P, S as an int64 array indexed by lag with zeros outside the admissible lags, the last admissible lag), or None."""
    rows = len(o)
    if rows - 1 < p["lag_min"]:
        return None
    last = min(p["lag_max"], rows - 1)
    S = np.zeros(last + 2, np.int64)
    for L in range(p["lag_min"], last + 1):
        S[L] = int(np.dot(o[: rows - L], o[L:])) * int(p["prior"][L])
    P = p["lag_min"] + int(np.argmax(S[p["lag_min"] : last + 1]))  # (argmax: the first maximum)
    return (P, S, last) if S[P] > 0 else None


def penalties(o, P, p):
    m = int((o * o).sum()) // int(o.sum())
    dmin, dmax = max(1, P // 2), 2 * P
    return dmin, dmax, {d: p["tightness"] * m * (d - P) ** 2 // (P * P) for d in range(dmin, dmax + 1)}


def restate(onset, **fields):
    """The header, step by step: (the summary as an array of one SUMMARY record, the beats as a list)."""
    p = full(fields)
    onset = np.asarray(onset, F).reshape(-1, PITCHES)
    rows = len(onset)
    if np.isnan(onset).any():
        return none(1), []
    o = strength(onset, p) if rows else np.zeros(0, np.int64)
    found = tempo(o, p)
    if found is None:
        return none(2), []
    P, S, last = found
    dmin, dmax, pen = penalties(o, P, p)
    pen_of = np.array([pen[d] for d in range(dmin, dmax + 1)], np.int64)
    C = np.zeros(rows, np.int64)
    back = np.zeros(rows, np.int64)
    for t in range(rows):
        best, src = 0, 0
        hi = min(dmax, t)
        if hi >= dmin:
            cand = C[t - hi : t - dmin + 1][::-1] - pen_of[: hi - dmin + 1]  # d = dmin ... hi
            k = int(np.argmax(cand))
            if cand[k] > 0:
                best, src = int(cand[k]), dmin + k
        C[t], back[t] = o[t] + best, src
    first = max(0, rows - P)
    t = first + int(np.argmax(C[first:]))
    beats = [t]
    while back[t]:
        t -= int(back[t])
        beats.append(t)
    refined = np.float64(P)
    if p["lag_min"] < P < last:
        l, c, r = np.float64(S[P - 1]), np.float64(S[P]), np.float64(S[P + 1])
        if c > l and c > r:
            refined = np.float64(P) + np.float64(0.5) * (l - r) / ((l - np.float64(2.0) * c) + r)
    return np.array([(0, P, len(beats), S[P], refined)], SUMMARY), beats[::-1]


def best_by_enumeration(onset, **fields):
    """Every ascending beat sequence of a small problem whose gaps lie in dmin ... dmax and whose last beat lies in the ending
    window: (the maximum of sum o[beats] - sum pen[gaps], the sequence the tie rule singles out, how many sequences share the
    maximum); None without a pulse.  The rule: the earliest maximal ending; then, read backwards, stopping is preferred to any
    further beat, and a later previous beat to an earlier one."""
    p = full(fields)
    onset = np.asarray(onset, F).reshape(-1, PITCHES)
    rows = len(onset)
    o = strength(onset, p)
    found = tempo(o, p)
    if found is None:
        return None
    P = found[0]
    dmin, dmax, pen = penalties(o, P, p)
    scored = []
    for n in range(1, rows + 1):
        for seq in itertools.combinations(range(rows), n):
            gaps = [b - a for a, b in zip(seq, seq[1:])]
            if seq[-1] >= max(0, rows - P) and all(dmin <= g <= dmax for g in gaps):
                scored.append((int(o[list(seq)].sum()) - sum(pen[g] for g in gaps), seq))
    top = max(v for v, _ in scored)
    ties = [seq for v, seq in scored if v == top]
    end = min(seq[-1] for seq in ties)
    # backwards from the ending: a sequence that has stopped beats one that goes on, a later beat beats an earlier one
    key = lambda seq: tuple(seq[::-1][1:]) + (rows,)  # noqa: E731
    chosen = max((seq for seq in ties if seq[-1] == end), key=key)
    return top, list(chosen), len(ties)


# ---- seeded maps
def noise(rng, rows):
    """A thousand levels, some beyond 0 ... 1."""
    return (rng.integers(-50, 1051, (rows, PITCHES)) / 1000.0).astype(F)


def pulses(rng, rows, period=None, floor=0.2):
    """A pulse train on a few pitches over a floor of low noise."""
    period = int(period or rng.integers(24, 90))
    m = (rng.uniform(0.0, floor, (rows, PITCHES)) if floor else np.zeros((rows, PITCHES))).astype(F)
    for t in range(int(rng.integers(0, period)) if floor else 0, rows, period):
        m[t, rng.choice(PITCHES, 4, replace=False)] = rng.uniform(0.6, 1.0, 4).astype(F)
    return m


def eighths(rng, rows, pitches=3):
    """Zero but for a few pitches in eighths: strengths of few values, so S, the candidates and the ending all tie."""
    m = np.zeros((rows, PITCHES), F)
    cols = rng.choice(PITCHES, pitches, replace=False)
    m[:, cols] = (rng.integers(0, 9, (rows, pitches)) * (rng.random((rows, pitches)) < 0.3) / 8.0).astype(F)
    return m


def silence(rng, rows):
    return np.zeros((rows, PITCHES), F)


def infinities(rng, rows):
    m = noise(rng, rows) * F(0.5)
    at = rng.integers(0, rows, 12)
    m[at, rng.integers(0, PITCHES, 12)] = np.where(rng.random(12) < 0.5, np.inf, -np.inf).astype(F)
    return m


KINDS = {"noise": noise, "pulses": pulses, "eighths": eighths, "silence": silence, "infinities": infinities}


def planted(seed):
    """Strictly periodic beats under the conditions the definition recovers exactly with the default parameters: period
    35 ... 60 in 300 ... 700 rows, three pitches of 0.6 ... 1.0 on each beat, uniform noise below 0.25 everywhere else, rows / 40
    single distractors of 0.7 strictly between the first and the last planted beat.  (onset, period, beats)."""
    rng = np.random.default_rng(1000 + seed)
    period, rows = int(rng.integers(35, 61)), int(rng.integers(300, 701))
    beats = np.arange(int(rng.integers(0, period)), rows, period)
    m = rng.uniform(0.0, 0.25, (rows, PITCHES)).astype(F)
    for t in beats:
        m[t, rng.choice(PITCHES, 3, replace=False)] = rng.uniform(0.6, 1.0, 3).astype(F)
    free = np.setdiff1d(np.arange(beats[0] + 1, beats[-1]), beats)
    for t in rng.choice(free, rows // 40, replace=False):
        m[t, rng.integers(0, PITCHES)] = F(0.7)
    return m, period, beats.tolist()


def job_segments(fields, ring, tile):
    """The segments of the GPU test's job under one parameter set, each (name, onset): the smallest lengths at which the kernels
    can go wrong.  `ring`: the path kernel's LDS ring, `tile`: a row tile of the tempo kernel."""
    p = full(fields)
    lag_min = p["lag_min"]
    rng = np.random.default_rng(77)
    train = np.zeros((2 * lag_min + 1, PITCHES), F)
    train[::lag_min] = F(0.9)  # three pulses at period lag_min: the shortest block of the path kernel
    slow = np.zeros((1100, PITCHES), F)
    slow[40::MAX_LAG, 20:60] = F(1.0)  # period 256: with lag_max = 256 the widest candidate set
    segs = [("no rows", silence(rng, 0)), ("one row", noise(rng, 1)), ("lag_min rows", noise(rng, lag_min)),
            ("lag_min + 1 rows", noise(rng, lag_min + 1)), ("period lag_min", train), ("period 256", slow)]
    for rows in (ring - 1, ring, ring + 1):
        segs.append((f"ring {rows}", pulses(rng, rows)))
    for rows in (tile - 1, tile, tile + 1):
        segs.append((f"tile {rows}", noise(rng, rows)))
    for kind, make in KINDS.items():
        segs.append((f"433 {kind}", make(rng, 433)))
    segs.append(("433 eighths, one pitch", eighths(rng, 433, 1)))
    segs.append(("2049 rows", pulses(rng, 2049, 47)))
    return segs
