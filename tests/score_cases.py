"""An independent restatement of note-level scoring (include/basic_pitch_amd_score.h) and the cases both score test files
use: numpy for the three predicates, scipy.sparse.csgraph.maximum_bipartite_matching for the size of a maximum matching.
Notes are rows (start_s, end_s, pitch_midi) of float64 arrays."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

DEFAULTS = dict(onset_tolerance_s=0.05, offset_ratio=0.2, offset_min_tolerance_s=0.05, pitch_tolerance_cents=50.0, strict=0)


def frame_time(fr):
    """model_frames_to_time()[fr], the expression every event's times come from (csrc/note_decode.cpp bp_internal_frame_time)."""
    fr = np.asarray(fr, np.int64)
    window_offset = (256.0 / 22050.0) * (172.0 - (43844.0 / 256.0)) + 0.0018
    return (fr * 256).astype(np.float64) / 22050.0 - window_offset * np.floor(fr.astype(np.float64) / 172.0)


def notes(rows):
    return np.asarray(rows, np.float64).reshape(-1, 3)


def graphs(est, ref, **tolerances):
    """The two hit matrices [ref][est]: onset and pitch; onset, pitch and offset."""
    t = dict(DEFAULTS, **tolerances)
    est, ref = notes(est), notes(ref)
    cmp = np.less if t["strict"] else np.less_equal
    on = cmp(np.round(np.abs(ref[:, None, 0] - est[None, :, 0]), 6), t["onset_tolerance_s"])
    pitch = cmp(100.0 * np.abs(ref[:, None, 2] - est[None, :, 2]), t["pitch_tolerance_cents"])
    tol = np.maximum(t["offset_ratio"] * (ref[:, 1] - ref[:, 0]), t["offset_min_tolerance_s"])
    off = cmp(np.round(np.abs(ref[:, None, 1] - est[None, :, 1]), 6), tol[:, None])
    return on & pitch, on & pitch & off


def matching_size(g):
    if g.size == 0:
        return 0
    return int((maximum_bipartite_matching(csr_matrix(g.astype(np.int8)), perm_type="column") >= 0).sum())


def first_fit(g):
    """What a matcher that never augments finds: every est, in order, takes the first ref it hits that is still free."""
    taken, size = set(), 0
    for e in range(g.shape[1]):
        for r in np.flatnonzero(g[:, e]):
            if r not in taken:
                taken.add(r)
                size += 1
                break
    return size


def restate(est, ref, **tolerances):
    """(n_ref, n_est, matched_onset, matched_offset)"""
    g_on, g_off = graphs(est, ref, **tolerances)
    return len(notes(ref)), len(notes(est)), matching_size(g_on), matching_size(g_off)


def random_case(rng):
    """1 - 11 notes a side on the frame grid: pitches 60 - 61, starts at frames 1 - 129, lengths 3 - 29 frames."""
    def side():
        n = int(rng.integers(1, 12))
        start = rng.integers(1, 130, n)
        end = start + rng.integers(3, 30, n)
        return np.stack([frame_time(start), frame_time(end), rng.integers(60, 62, n).astype(np.float64)], axis=1)

    return side(), side()


# The minimal chain: est 0.04 hits both refs, est -0.04 the ref at 0.00 alone.  A first fit strands the second est when the est
# that hits both comes first in its order of ests and the shared ref first in its order of refs: the four arrangements fail
# the four scan orders, so that none passes by luck.  Maximum 2, first fit 1.
_E, _R = [(0.04, 1.0, 60), (-0.04, 1.0, 60)], [(0.00, 1.0, 60), (0.08, 1.0, 60)]
CHAINS = [(notes(e), notes(r)) for e in (_E, _E[::-1]) for r in (_R, _R[::-1])]


def long_chain(p, decoy_low, start=1.0, end=2.0, k=8):
    """k est notes of equal onset at pitches p ... p + k - 1; refs at p + 0.5 ... p + k - 1.5, each hitting two of them at 50
    cents, and a decoy at p - 0.4 (hitting p alone) or at p + k - 0.6 (hitting p + k - 1 alone): all k match only by a path
    through the whole chain.  Low decoy: ests and refs ascending, the decoy last; high decoy: the mirror, both descending.
    Either way a first fit in index order takes every inner ref from the wrong side and strands the last est."""
    order = range(k) if decoy_low else range(k - 1, -1, -1)
    est = notes([(start, end, p + i) for i in order])
    mid = [(start, end, p + i + 0.5) for i in (range(k - 1) if decoy_low else range(k - 2, -1, -1))]
    return est, notes(mid + [(start, end, p - 0.4 if decoy_low else p + k - 0.6)])
