"""Chords and key, restated (include/basic_pitch_amd_chord.h): an independent numpy int64 statement of the header's definition,
written from the header and not from csrc/chord_host.cpp, the enumeration of every state sequence of small problems, the
seeded maps, tables and parameter sets the CPU and GPU tests share, and the job of many segments of the GPU test."""
import itertools

import numpy as np

PITCHES = 88
CLASSES = 12
MAX_STATES = 64
F = np.float32
SUMMARY = np.dtype([("status", np.int32), ("key", np.int32), ("n_units", np.int32), ("n_changes", np.int32), ("score", np.int64),
                    ("key_score", np.int64)])
NOTE_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
TONES = {"maj": (0, 4, 7), "min": (0, 3, 7), "dim": (0, 3, 6), "aug": (0, 4, 8), "7": (0, 4, 7, 10), "maj7": (0, 4, 7, 11), "min7": (0, 3, 7, 10)}
VOCABULARIES = {"majmin": ("maj", "min"), "triads": ("maj", "min", "dim", "aug"), "sevenths": ("maj", "min", "7", "maj7", "min7")}
KK = np.array([[6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88],
               [6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17]])


def templates(vocabulary="majmin"):
    """(n_states, bias[64], weights[64][12], names) of a vocabulary, from the header's sentence: N with weights 0 and bias 12,
    then quality-major, root ascending from C, a chord of n tones 12 - n on its tones and -n elsewhere."""
    bias, weights, names = np.zeros(MAX_STATES, np.int64), np.zeros((MAX_STATES, CLASSES), np.int64), ["N"]
    bias[0] = 12
    for quality in VOCABULARIES[vocabulary]:
        for root in range(12):
            tones = [(root + t) % 12 for t in TONES[quality]]
            s = len(names)
            weights[s] = -len(tones)
            weights[s, tones] = 12 - len(tones)
            names.append(f"{NOTE_NAMES[root]}:{quality}")
    return len(names), bias, weights, names


def key_profiles():
    """The header's sentence in numpy float64: mean removed, unit norm x 1024, rint."""
    centred = KK - KK.mean(axis=1, keepdims=True)
    return np.rint(1024.0 * centred / np.sqrt((centred ** 2).sum(axis=1, keepdims=True))).astype(np.int64)


def random_table(seed, n_states):
    """A signed table of n_states states and random profiles, every entry in -1024 ... 1024 (the bounds themselves among them)."""
    rng = np.random.default_rng(seed)
    bias, weights = np.zeros(MAX_STATES, np.int64), np.zeros((MAX_STATES, CLASSES), np.int64)
    bias[:n_states] = rng.integers(-1024, 1025, n_states)
    weights[:n_states] = rng.integers(-1024, 1025, (n_states, CLASSES))
    weights[0, 0], weights[n_states - 1, 11], bias[0] = 1024, -1024, -1024
    return dict(n_states=n_states, bias=bias, weights=weights, key_profile=rng.integers(-1024, 1025, (2, CLASSES)))


DEFAULT = dict(threshold_q=307, min_pitch=0, max_pitch=87, switch_penalty=128)
# the parameter sets of the CPU and the GPU tests (fields on top of the defaults; "vocabulary" or a table of one's own)
PARAM_SETS = {
    "default": dict(),                                   # 25 states
    "threshold_0": dict(threshold_q=0),
    "threshold_1024": dict(threshold_q=1024),            # nothing is above it
    "penalty_0": dict(switch_penalty=0),
    "penalty_1024": dict(switch_penalty=1024),
    "one_state": random_table(1, 1),
    "two_states": random_table(2, 2),
    "triads": dict(vocabulary="triads"),                 # 49 states
    "sevenths": dict(vocabulary="sevenths", switch_penalty=16),  # 61 states
    "random_64": dict(random_table(64, 64), switch_penalty=300, threshold_q=200),
    "one_pitch": dict(min_pitch=45, max_pitch=45, threshold_q=100, switch_penalty=3),
}


def full(fields):
    """A parameter set spelled out: the defaults, the table, the profiles, the fields on top."""
    n, bias, weights, _ = templates(fields.get("vocabulary", "majmin"))
    p = dict(DEFAULT, n_states=n, bias=bias, weights=weights, key_profile=key_profiles())
    p.update({k: v for k, v in fields.items() if k != "vocabulary"})
    for k in ("bias", "weights", "key_profile"):
        p[k] = np.asarray(p[k], np.int64)
    return p


def quantise(x):
    """q(x) in float32, as basic_pitch_amd_align.h writes it."""
    x = np.asarray(x, F)
    return np.floor(np.minimum(np.maximum(x, F(0.0)), F(1.0)) * F(1024.0) + F(0.5)).astype(np.int64)


def chroma(note, p):
    above = np.maximum(quantise(note) - p["threshold_q"], 0)
    above[:, : p["min_pitch"]] = 0
    above[:, p["max_pitch"] + 1 :] = 0
    classes = (np.arange(PITCHES) + 9) % 12
    return np.stack([above[:, classes == k].sum(axis=1) for k in range(CLASSES)], axis=1).astype(np.int64)


def none(status, rows):
    return np.array([(status, -1, 0, 0, 0, 0)], SUMMARY), np.zeros(rows, np.uint8)


def unit_edges(rows, bounds):
    """The first frames of the units and the end of the last one."""
    bounds = [int(b) for b in (bounds if bounds is not None else [])]
    return np.array([0] + bounds + [rows], np.int64) if bounds else np.arange(rows + 1, dtype=np.int64)


def emissions(note, bounds, p):
    """(e[u][s], pen[u], edges, m, c) of a segment in which something sounds, or None."""
    c = chroma(note, p)
    if c.sum() == 0:
        return None
    m = int((c * c).sum()) // int(c.sum())
    edges = unit_edges(len(note), bounds)
    lens = np.diff(edges)
    cu = np.add.reduceat(c, edges[:-1], axis=0)
    n = p["n_states"]
    e = lens[:, None] * p["bias"][None, :n] * m + cu @ p["weights"][:n].T
    return e.astype(np.int64), (lens * p["switch_penalty"] * m).astype(np.int64), edges, m, c


def restate(note, bounds=None, **fields):
    """The header, step by step: (the summary as an array of one SUMMARY record, the labels as one uint8 per row)."""
    p = full(fields)
    note = np.asarray(note, F).reshape(-1, PITCHES)
    rows = len(note)
    if np.isnan(note).any():
        return none(1, rows)
    found = emissions(note, bounds, p) if rows else None
    if found is None:
        return none(2, rows)
    e, pen, edges, m, c = found
    total = c.sum(axis=0)
    K = np.array([sum(int(p["key_profile"][j // 12][(k - j % 12 + 12) % 12]) * int(total[k]) for k in range(CLASSES)) for j in range(24)], np.int64)
    key = int(np.argmax(K))  # (argmax: the first maximum)
    n_units, n = e.shape
    own = np.arange(n)
    back = np.zeros((n_units, n), np.int64)
    back[0] = own
    D = e[0].copy()
    for u in range(1, n_units):
        a = int(np.argmax(D))
        over = D[a] - pen[u]
        move = over > D
        back[u] = np.where(move, a, own)
        D = e[u] + np.where(move, over, D)
    s = int(np.argmax(D))
    score = int(D[s])
    states = np.zeros(n_units, np.int64)
    for u in range(n_units - 1, -1, -1):
        states[u] = s
        s = int(back[u][s])
    labels = np.repeat(states, np.diff(edges)).astype(np.uint8)
    changes = int((np.diff(states) != 0).sum())
    return np.array([(0, key, n_units, changes, score, K[key])], SUMMARY), labels


def best_by_enumeration(note, bounds=None, **fields):
    """Every state sequence of a small problem: (the maximum of sum e[u][s_u] - sum of pen[u] over the units whose state
    differs from the one before, the sequences that reach it); None where nothing sounds."""
    p = full(fields)
    note = np.asarray(note, F).reshape(-1, PITCHES)
    found = emissions(note, bounds, p)
    if found is None:
        return None
    e, pen = found[0], found[1]
    n_units, n = e.shape
    scored = []
    for seq in itertools.product(range(n), repeat=n_units):
        v = sum(int(e[u][s]) for u, s in enumerate(seq)) - sum(int(pen[u]) for u in range(1, n_units) if seq[u] != seq[u - 1])
        scored.append((v, seq))
    top = max(v for v, _ in scored)
    return top, [list(seq) for v, seq in scored if v == top]


# ---- seeded maps
def noise(rng, rows):
    """A thousand levels, some beyond 0 ... 1."""
    return (rng.integers(-50, 1051, (rows, PITCHES)) / 1000.0).astype(F)


def plateaux(rng, rows):
    """Eighths on whole stretches of rows, the same value in every pitch of a class and often in several classes: chromas of
    few values, so states tie in D, D[a] - pen ties with D[s], and the last state ties."""
    m = np.zeros((rows, PITCHES), F)
    classes = (np.arange(PITCHES) + 9) % 12
    t = 0
    while t < rows:
        n = int(rng.integers(1, 12))
        level = rng.integers(3, 9, CLASSES) / 8.0 * (rng.random(CLASSES) < 0.4)
        if rng.random() < 0.3:
            level[:] = level.max()  # every class alike: every chord state ties
        m[t : t + n] = level[classes].astype(F)
        t += n
    return m


def triads(rng, rows, run=None):
    """Runs of clean triads of random levels with silence between some, over a floor of low noise."""
    m = rng.uniform(0.0, 0.2, (rows, PITCHES)).astype(F)
    classes = (np.arange(PITCHES) + 9) % 12
    t = 0
    while t < rows:
        n = int(run or rng.integers(1, 40))
        if rng.random() < 0.75:
            root, third = int(rng.integers(0, 12)), int(rng.choice([3, 4]))
            tones = np.isin(classes, [(root + d) % 12 for d in (0, third, 7)]) & (np.arange(PITCHES) >= 27) & (np.arange(PITCHES) < 63)
            m[t : t + n, tones] = F(rng.uniform(0.5, 1.0))
        t += n
    return m


def silence(rng, rows):
    return np.zeros((rows, PITCHES), F)


def under(rng, rows):
    """Everything under the default threshold."""
    return rng.uniform(0.0, 0.29, (rows, PITCHES)).astype(F)


def infinities(rng, rows):
    m = noise(rng, rows) * F(0.5)
    n = min(12, rows)
    m[rng.integers(0, rows, n), rng.integers(0, PITCHES, n)] = np.where(rng.random(n) < 0.5, np.inf, -np.inf).astype(F)
    return m


def major_minor_tie(root, rows):
    """Root, both thirds and the fifth at one level in one octave: the root's major and minor triads tie in every D."""
    m = np.zeros((rows, PITCHES), F)
    m[:, [39 + root, 42 + root, 43 + root, 46 + root]] = F(0.75)  # pitch p has class (p + 9) % 12: 39 is a C
    return m


KINDS = {"noise": noise, "plateaux": plateaux, "triads": triads, "silence": silence, "under": under, "infinities": infinities}


def irregular(rng, rows):
    """Boundaries at irregular gaps, strictly ascending inside 0 < B < rows (none for rows < 2)."""
    if rows < 2:
        return []
    picks = rng.random(rows - 1) < 0.15
    return (np.flatnonzero(picks) + 1).tolist()


# ---- planted chords and keys
def planted(seed, run):
    """Clean triads of the majmin table in runs of `run` frames, silence of `run` frames between some: every sounding pitch at
    one level, each tone in `octaves` octaves.  The first three runs are a chord, silence, the same chord, then a chord that
    shares two tones with it: the patterns that need the longest runs.  (note, the planted state of every row)"""
    rng = np.random.default_rng(2000 + seed)
    level, octaves = F(rng.uniform(0.5, 1.0)), int(rng.integers(1, 4))
    first = int(rng.integers(1, 25))
    root, minor = (first - 1) % 12, first > 12
    related = 1 + 12 + (root + 9) % 12 if not minor else 1 + (root + 3) % 12  # C:maj -> A:min, A:min -> C:maj
    states = [first, 0, first, related]
    while len(states) < 12:
        s = int(rng.integers(0, 25))
        if s != states[-1]:
            states.append(s)
    _, _, weights, _ = templates("majmin")
    classes = (np.arange(PITCHES) + 9) % 12
    rows = []
    for s in states:
        row = np.zeros(PITCHES, F)
        if s:
            tones = np.flatnonzero(weights[s] > 0)
            row[np.isin(classes, tones) & (np.arange(PITCHES) >= 27) & (np.arange(PITCHES) < 27 + 12 * octaves)] = level
        rows += [row] * run
    return np.array(rows, F), np.repeat(states, run).astype(np.uint8)


def planted_scale(key):
    """A scale with its tonic triad dwelt on: the tonic 4 frames, third and fifth 3, the other degrees 1, at 0.8, one octave.
    key 0 ... 11 major, 12 ... 23 (natural) minor."""
    tonic, minor = key % 12, key >= 12
    degrees = (0, 2, 3, 5, 7, 8, 10) if minor else (0, 2, 4, 5, 7, 9, 11)
    rows = []
    for d in degrees:
        row = np.zeros(PITCHES, F)
        row[36 + ((tonic + d) % 12 + 3) % 12] = F(0.8)  # pitch p has class (p + 9) % 12
        rows += [row] * (4 if d == 0 else (3 if d in (3, 4, 7) else 1))
    return np.array(rows, F)


# ---- the job of the GPU test
def job_segments(chroma_rows, trace_tile):
    """The segments of the GPU test's job, each (name, note): the smallest lengths at which the kernels can go wrong.
    chroma_rows: the rows of a block of the chroma kernel; trace_tile: the records of a tile of the backtrace."""
    rng = np.random.default_rng(78)
    segs = [("no rows", silence(rng, 0))]
    for rows in (1, 2, 63, 64, 65, chroma_rows - 1, chroma_rows, chroma_rows + 1):
        segs.append((f"{rows} noise", noise(rng, rows)))
    for rows in (trace_tile - 1, trace_tile, trace_tile + 1):
        segs.append((f"{rows} triads", triads(rng, rows, 25)))
    for kind, make in KINDS.items():
        segs.append((f"150 {kind}", make(rng, 150)))
    # C, D#, E and G at one level: C:maj (state 1) and C:min (state 13) tie in every D and the first maximum is C:maj; one D#
    # cell raised and C:min is ahead at the end
    tie = major_minor_tie(0, 97)
    raised = tie.copy()
    raised[40, 42] = F(1.0)
    segs += [("97 plateaux", plateaux(rng, 97)), ("97 tie", tie), ("97 tie, one cell raised", raised), ("2049 triads", triads(rng, 2049, 30))]
    return segs


BOUND_MODES = ("none", "every", "one", "spans", "mixed")


def job_bounds(mode, maps, chroma_rows):
    """Per segment its boundaries under one mode (None: the call gets no boundaries at all).  every: all of 1 ... rows - 1;
    one: the middle; spans: units of one frame beside a unit of 2 * chroma_rows + 5 frames, which spans two blocks of the chroma
    kernel whatever its start, then irregular ones; mixed: every other segment irregular, the others none."""
    if mode == "none":
        return None
    rng = np.random.default_rng(79)
    out = []
    for i, m in enumerate(maps):
        rows = len(m)
        if mode == "every":
            b = list(range(1, rows))
        elif mode == "one":
            b = [rows // 2] if rows >= 2 else []
        elif mode == "spans":
            wide = 2 * chroma_rows + 5
            b = [1, 2, 3, 3 + wide, 4 + wide, 5 + wide] + [5 + wide + x for x in irregular(rng, rows - 5 - wide)] if rows > wide + 6 else irregular(rng, rows)
        else:
            b = irregular(rng, rows) if i % 2 else []
        out.append(b)
    return out
