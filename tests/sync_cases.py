"""What the sync tests share (include/basic_pitch_amd_sync.h): an independent restatement of the header's definition in numpy
int64 and Python integers — chroma, units, the ceiling root by math.isqrt, the full D and predecessor matrices, the backtrace —,
the enumeration of ALL monotone paths of small problems, and the generators of maps: seeded levels ("thousand": a thousand
levels; "eighths": eighths on stretches, whose coarse values force ties), planted warps of one-hot units, chord maps, and the
stacking of segments into a job.  No test here; tests/test_sync_cpu.py and tests/test_gpu_sync.py import it."""
import math

import numpy as np

SUMMARY = np.dtype([("status", np.int32), ("units_a", np.int32), ("units_b", np.int32), ("n_path", np.int32),
                    ("path_first", np.int64), ("total", np.int64)])
DEFAULTS = dict(threshold_q=307, min_pitch=0, max_pitch=87, hop=4, band=0)
MAX_GAIN = 255 * 255


def quantise(x):
    """q(x) of basic_pitch_amd_align.h in float32: floor(clamp(x, 0, 1) * 1024 + 0.5)."""
    x = np.asarray(x, np.float32)
    clamped = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
    return np.floor(clamped * np.float32(1024) + np.float32(0.5)).astype(np.int64)


def ceil_root(s):
    """The smallest r with r * r >= s."""
    r = math.isqrt(int(s))
    return r if r * r == s else r + 1


def features(note, threshold_q=307, min_pitch=0, max_pitch=87, hop=4, **_):
    """(U, 12) int64 features of a (rows, 88) map without a NaN."""
    note = np.asarray(note, np.float32).reshape(-1, 88)
    rows = len(note)
    above = np.maximum(quantise(note) - threshold_q, 0)
    above[:, :min_pitch] = 0
    above[:, max_pitch + 1:] = 0
    chroma = np.zeros((rows, 12), np.int64)
    for p in range(88):
        chroma[:, (p + 9) % 12] += above[:, p]
    assert chroma.max(initial=0) <= 2 ** 13
    U = -(-rows // hop)
    x = np.zeros((U, 12), np.int64)
    for u in range(U):
        cu = chroma[u * hop:(u + 1) * hop].sum(axis=0)
        s = int((cu * cu).sum())
        if s:
            x[u] = 255 * cu // ceil_root(s)
    return x


def gains(xa, xb):
    return xa @ xb.T


def admissible(N, M, band):
    i, j = np.arange(N, dtype=np.int64)[:, None], np.arange(M, dtype=np.int64)[None, :]
    if band == 0:
        return np.ones((N, M), bool)
    return np.abs(i * (M - 1) - j * (N - 1)) <= band * max(N - 1, M - 1)


def warp(g, ok):
    """The header's recurrence on an (N, M) gain matrix under the admissible mask: (D with None where unreachable as a list of
    lists, the predecessor codes, the path in ascending order or None, the total)."""
    N, M = g.shape
    D = [[None] * M for _ in range(N)]
    came = [[0] * M for _ in range(N)]
    for i in range(N):
        for j in range(M):
            if not ok[i, j]:
                continue
            if i == 0 and j == 0:
                D[0][0] = 2 * int(g[0, 0])
                continue
            best = None
            for code, (pi, pj, w) in enumerate(((i - 1, j - 1, 2), (i - 1, j, 1), (i, j - 1, 1))):
                if pi < 0 or pj < 0 or D[pi][pj] is None:
                    continue
                value = D[pi][pj] + w * int(g[i, j])
                if best is None or value > best:  # a later candidate wins only when strictly greater
                    best, came[i][j] = value, code
            D[i][j] = best
    if D[N - 1][M - 1] is None:
        return D, came, None, 0
    i, j, path = N - 1, M - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        code = came[i][j]
        i, j = (i - 1 if code != 2 else i), (j - 1 if code != 1 else j)
    return D, came, path[::-1], D[N - 1][M - 1]


def restate(note_a, note_b, **fields):
    """(the SUMMARY record as an array of one, the pair's region of path as (N + M - 1, 2) int32) as bp_sync_rows gives them."""
    p = dict(DEFAULTS, **fields)
    a, b = np.asarray(note_a, np.float32).reshape(-1, 88), np.asarray(note_b, np.float32).reshape(-1, 88)
    N, M = -(-len(a) // p["hop"]), -(-len(b) // p["hop"])
    room = N + M - 1 if N and M else 0
    summary = np.zeros(1, SUMMARY)
    summary["units_a"], summary["units_b"] = N, M
    region = np.full((room, 2), -1, np.int32)
    if np.isnan(a).any() or np.isnan(b).any():
        summary["status"] = 1
        return summary, region
    if not room:
        summary["status"] = 2
        return summary, region
    g = gains(features(a, **p), features(b, **p))
    assert 0 <= g.min() and g.max() <= MAX_GAIN
    _, _, path, total = warp(g, admissible(N, M, p["band"]))
    if path is None:
        summary["status"] = 2
        return summary, region
    assert max(N, M) <= len(path) <= room and total <= (N + M) * MAX_GAIN
    region[:len(path)] = np.array(path, np.int32)
    summary["n_path"], summary["total"] = len(path), total
    return summary, region


def all_paths(N, M):
    """Every monotone path from (0, 0) to (N-1, M-1) by steps (1, 1), (1, 0), (0, 1), each a list of cells."""
    out = []

    def walk(path):
        i, j = path[-1]
        if (i, j) == (N - 1, M - 1):
            out.append(list(path))
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < M:
                path.append((i + di, j + dj))
                walk(path)
                path.pop()

    walk([(0, 0)])
    return out


def path_total(g, path):
    """The first cell and every cell entered diagonally count twice, the others once."""
    total = 2 * int(g[0, 0])
    for (pi, pj), (i, j) in zip(path, path[1:]):
        total += (2 if (i - pi, j - pj) == (1, 1) else 1) * int(g[i, j])
    return total


def selected_by_ties(best_paths):
    """Of the optimal paths the one the tie order selects, read from the end: at every cell, back along what is already chosen,
    diagonal before (i-1, j) before (i, j-1)."""
    left = [list(reversed(p)) for p in best_paths]
    k = 0
    while len(left) > 1:
        k += 1
        cell = left[0][k - 1]
        for step in ((1, 1), (1, 0), (0, 1)):
            keep = [p for p in left if (cell[0] - p[k][0], cell[1] - p[k][1]) == step]
            if keep:
                left = keep
                break
    return list(reversed(left[0]))


# ---- generators
def thousand(rng, rows):
    """A thousand levels, some below 0 and above 1."""
    return (rng.integers(-50, 1051, (rows, 88)) / 1000.0).astype(np.float32)


def eighths(rng, rows, stretch=5):
    """Eighths on stretches of a few rows and pitches: coarse values, so that sums tie."""
    base = rng.integers(0, 9, (-(-rows // stretch), 22))
    return (np.repeat(np.repeat(base, stretch, axis=0)[:rows], 4, axis=1) / 8.0).astype(np.float32)


def sparse(rng, rows):
    """A few sounding pitches a row, silence elsewhere; some rows silent."""
    note = np.zeros((rows, 88), np.float32)
    for t in range(rows):
        if rng.integers(0, 5):
            note[t, rng.integers(0, 88, 3)] = rng.choice([0.5, 0.75, 1.0])
    return note


KINDS = {"thousand": thousand, "eighths": eighths, "sparse": sparse}


def random_maps(seed, rows_a, rows_b, kind):
    rng = np.random.default_rng(seed)
    return KINDS[kind](rng, rows_a), KINDS[kind](rng, rows_b)


def one_hot_units(classes, hop):
    """A map whose unit u sounds one pitch of class classes[u] at level 1, `hop` rows a unit."""
    note = np.zeros((len(classes) * hop, 88), np.float32)
    for u, k in enumerate(classes):
        note[u * hop:(u + 1) * hop, 39 + int(k)] = 1.0  # pitch 39 is a C
    return note


def planted_warp(seed, N, M, hop=4):
    """(a, b, w): a has N one-hot units whose class differs from its neighbours', b = a's units [w] for a non-decreasing w of
    M >= N entries from 0 to N - 1 with steps of 0 or 1."""
    assert M >= N
    rng = np.random.default_rng(seed)
    classes = [int(rng.integers(0, 12))]
    while len(classes) < N:
        k = int(rng.integers(0, 12))
        if k != classes[-1]:
            classes.append(k)
    steps = np.zeros(M - 1, np.int64)
    steps[rng.permutation(M - 1)[:N - 1]] = 1
    w = np.concatenate([[0], np.cumsum(steps)])
    assert w[-1] == N - 1
    return one_hot_units(classes, hop), one_hot_units([classes[i] for i in w], hop), w


def chord_map(seed, units, hop=4):
    """Triads at one level in runs of a few units, every unit a chord of three classes: all units have the same self-gain."""
    rng = np.random.default_rng(seed)
    note = np.zeros((units * hop, 88), np.float32)
    u = 0
    while u < units:
        root, minor, run = int(rng.integers(0, 12)), int(rng.integers(0, 2)), int(rng.integers(2, 6))
        for tone in (0, 3 if minor else 4, 7):
            note[u * hop:(u + run) * hop, 27 + (root + tone) % 12] = 1.0
        u += run
    return note


def stack(maps):
    """(row offsets as int64, the maps one after the other as one C-contiguous float32 array)."""
    offs = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    note = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1, 88) for m in maps]), np.float32)
    return offs, note
