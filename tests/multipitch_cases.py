"""An independent restatement of multi-pitch estimates (include/basic_pitch_amd_multipitch.h) and the cases both multipitch
test files use: scipy.signal.argrelmax for the peaks, numpy float64 for the refinement exactly as the header writes it, and
frame_score_cases' roll of the refs with scipy's maximum bipartite matching per frame for the counts, the peaks' pitches being
the estimate side.  The case maps come from seeded generators; the crafted rows are named."""
import numpy as np
from scipy.signal import argrelmax

import frame_score_cases as FC
import score_cases as SC

BINS = 264
POINT = np.dtype([("frame", np.int32), ("salience", np.float32), ("pitch_midi", np.float64)])
DEFAULT = dict(threshold=0.3, min_bin=1, max_bin=262)
BANDS = ((1, 262), (1, 1), (262, 262), (100, 100), (37, 201), (2, 261))


def params(**fields):
    return dict(DEFAULT, **fields)


def finite(contour):
    return bool(np.isfinite(np.asarray(contour, np.float32)).all())


def restate_points(contour, threshold=0.3, min_bin=1, max_bin=262, **_):
    """(POINT records ordered by frame, then bin; status; delta per point)."""
    c = np.asarray(contour, np.float32).reshape(-1, BINS)
    if not finite(c):
        return np.zeros(0, POINT), 1, np.zeros(0)
    t, b = argrelmax(c, axis=1) if len(c) else (np.zeros(0, np.int64), np.zeros(0, np.int64))  # strict on both sides, never an edge bin
    keep = (b >= min_bin) & (b <= max_bin) & (c[t, b] >= np.float32(threshold))
    t, b = t[keep], b[keep]
    order = np.lexsort((b, t))
    t, b = t[order], b[order]
    left, mid, right = (c[t, b + d].astype(np.float64) for d in (-1, 0, 1))
    delta = 0.5 * (left - right) / ((left - 2.0 * mid) + right)
    out = np.zeros(len(t), POINT)
    out["frame"], out["salience"], out["pitch_midi"] = t, c[t, b], 21.0 + (b.astype(np.float64) + delta) / 3.0
    return out, 0, delta


def restate_counts(points, ref, n_frames, pitch_tolerance_cents=50.0, strict=0, **_):
    """(n_frames, ref_frames, est_frames, true_pos, e_sub), (e_miss, e_fa): per frame the refs sounding there against the
    distinct pitches of the points on it, a maximum bipartite matching of the hit matrix."""
    ref = SC.notes(ref)
    ref_on = FC.roll(ref, n_frames)
    s = np.zeros(6, np.int64)
    inside = points[(points["frame"] >= 0) & (points["frame"] < n_frames)]
    for fr in range(n_frames):
        est_side = np.unique(inside["pitch_midi"][inside["frame"] == fr])
        ref_side = ref[ref_on[:, fr], 2]
        g = FC.hit_matrix(ref_side, est_side, pitch_tolerance_cents=pitch_tolerance_cents, strict=strict)
        n_ref, n_est = len(ref_side), len(est_side)
        tp = SC.matching_size(g) if g.any() else 0
        s += (n_ref, n_est, tp, min(n_ref, n_est) - tp, max(0, n_ref - n_est), max(0, n_est - n_ref))
    return (n_frames, int(s[0]), int(s[1]), int(s[2]), int(s[3])), (int(s[4]), int(s[5]))


# ---- the case maps
def bumps(rng, rows, n_voices=3):
    """Smooth bumps plus low noise: a few peaks per row.  Every voice a Gaussian of 2 - 4 bins' width that drifts slowly."""
    b = np.arange(BINS, dtype=np.float64)[None, :]
    c = rng.uniform(0.0, 0.02, (rows, BINS))
    for _ in range(n_voices):
        centre = rng.uniform(20, 240) + np.cumsum(rng.normal(0, 0.15, rows))
        width = rng.uniform(2.0, 4.0)
        c += rng.uniform(0.4, 0.9) * np.exp(-0.5 * ((b - centre[:, None]) / width) ** 2)
    return c.astype(np.float32)


def dense(rng, rows):
    """Uniform noise: about a third of the bins are peaks."""
    return rng.uniform(0.0, 1.0, (rows, BINS)).astype(np.float32)


def _below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def crafted(threshold=0.3):
    """The named rows, one segment of them: {name: row index}, the map (finite)."""
    thr = np.float32(threshold)
    rows, names = [], {}

    def add(name, row):
        names[name] = len(rows)
        rows.append(np.asarray(row, np.float32))

    alt = np.zeros(BINS, np.float32)
    alt[1:262:2] = 0.8  # bins 1, 3, ..., 261
    add("alternating_131", alt)
    flat = np.zeros(BINS, np.float32)
    flat[50:52] = 0.7   # a plateau of two
    flat[90:93] = 0.7   # a plateau of three
    add("plateaus", flat)
    ends = np.zeros(BINS, np.float32)
    ends[1], ends[262] = 0.9, 0.6
    add("peaks_at_1_and_262", ends)
    edges = np.zeros(BINS, np.float32)
    edges[0], edges[263] = 5.0, 7.0  # large cells at the edge bins: never peaks (and bins 1, 262 are below them)
    add("edge_cells", edges)
    at = np.zeros(BINS, np.float32)
    at[40], at[80] = thr, _below(thr)
    add("threshold_exact_and_one_step_below", at)
    skew = np.zeros(BINS, np.float32)
    skew[119], skew[120], skew[121] = 0.001, 0.75, _below(0.75)  # delta near +0.5
    skew[199], skew[200], skew[201] = _below(0.6), 0.6, 0.002    # delta near -0.5
    add("delta_near_half", skew)
    add("all_zero", np.zeros(BINS, np.float32))
    return names, np.stack(rows)


def with_nonfinite(contour, value, row, bin_):
    c = np.array(contour, np.float32, copy=True)
    c[row, bin_] = value
    return c


SEGMENT_ROWS = (0, 1, 2, 63, 64, 65, 142, 173, 433)


def segment_job(seed=0, rows=SEGMENT_ROWS):
    """Segments of the given rows, alternating bumps and dense noise, the crafted rows appended to the segment of 65."""
    rng = np.random.default_rng(seed)
    segs = []
    for i, r in enumerate(rows):
        c = bumps(rng, r) if i % 2 == 0 else dense(rng, r)
        if r == 65:
            crafted_rows = crafted()[1]
            c[: len(crafted_rows)] = crafted_rows
        segs.append(c)
    return segs


def stack(segs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    return offs, np.ascontiguousarray(np.concatenate(segs) if segs else np.zeros((0, BINS), np.float32), np.float32)


def refs_for(rng, contour, params_, n=12):
    """Refs that make the reference non-trivial against a segment's own peaks: some exactly on a peak's pitch over a stretch
    of frames (true positives), some a quarter tone or more off (substitutions), some where nothing is (misses); the rest of
    the peaks are false alarms."""
    rows = len(contour)
    points, status, _ = restate_points(contour, **params_)
    out = []
    for k in range(n):
        f0 = int(rng.integers(0, max(1, rows)))
        f1 = min(rows + 3, f0 + int(rng.integers(1, 40)))
        on = points[points["frame"] == f0]
        if len(on) and k % 3 != 2:
            pitch = float(on["pitch_midi"][int(rng.integers(0, len(on)))]) + (0.0, 0.7)[k % 3]
        else:
            pitch = float(rng.uniform(10.0, 20.0))  # below every bin: hits nothing
        out.append((float(SC.frame_time(f0)), float(SC.frame_time(f1)), pitch))
    return SC.notes(out)
