"""An independent restatement of frame-level scoring (include/basic_pitch_amd_frame_score.h) and the cases both frame-score
test files use: a numpy roll of the refs and events sounding on each frame from score_cases.frame_time, the hit matrix by the
pitch predicate, scipy's maximum bipartite matching per frame, and the sums — misses and false alarms summed per frame
directly, not by the identity.  Notes are rows (start_s, end_s, pitch_midi) of float64 arrays."""
import numpy as np

import score_cases as SC

FIELDS = ("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub")
TOLERANCES = (0.0, 30.0, 50.0, 100.0, 120.0)
N_FRAMES = (150, 172, 173, 344, 345, 360)  # ends before, on and after the time steps at 172 and 344


def roll(rows, n_frames):
    """[note][frame]: the note sounds on the frame, start_s <= time(fr) < end_s."""
    rows = SC.notes(rows)
    t = SC.frame_time(np.arange(n_frames))
    return (rows[:, None, 0] <= t[None, :]) & (t[None, :] < rows[:, None, 1])


def hit_matrix(ref_pitches, est_pitches, pitch_tolerance_cents=50.0, strict=0, **_):
    cmp = np.less if strict else np.less_equal
    return cmp(100.0 * np.abs(np.asarray(ref_pitches, np.float64)[:, None] - np.asarray(est_pitches, np.float64)[None, :]),
               pitch_tolerance_cents)


def per_frame(est, ref, n_frames, **tolerances):
    """Per frame (n_ref, n_est, tp, e_sub, e_miss, e_fa) and the hit matrix [ref][est] of its two sides.  Frames with the same
    notes sounding share one matching."""
    est, ref = SC.notes(est), SC.notes(ref)
    est_on, ref_on = roll(est, n_frames), roll(ref, n_frames)
    seen, out = {}, []
    for fr in range(n_frames):
        key = (est_on[:, fr].tobytes(), ref_on[:, fr].tobytes())
        if key not in seen:
            est_side = np.unique(est[est_on[:, fr], 2])  # the set of distinct pitches
            ref_side = ref[ref_on[:, fr], 2]             # the multiset, as given
            g = hit_matrix(ref_side, est_side, **tolerances)
            n_ref, n_est, tp = len(ref_side), len(est_side), SC.matching_size(g) if g.any() else 0
            seen[key] = ((n_ref, n_est, tp, min(n_ref, n_est) - tp, max(0, n_ref - n_est), max(0, n_est - n_ref)), g)
        out.append(seen[key])
    return out


def restate(est, ref, n_frames, **tolerances):
    """(n_frames, ref_frames, est_frames, true_pos, e_sub), (e_miss, e_fa)"""
    frames = np.array([f for f, _ in per_frame(est, ref, n_frames, **tolerances)], np.int64).reshape(-1, 6)
    s = frames.sum(axis=0)
    return (n_frames, int(s[0]), int(s[1]), int(s[2]), int(s[3])), (int(s[4]), int(s[5]))


def random_case(rng):
    """1 - 11 notes a side on the frame grid: est pitches 58 - 63, ref pitches the same plus one of 0, +-0.3, +-0.5; starts at
    frames 1 - 300, lengths 3 - 60 frames; the segment's frames, the tolerance and the comparison drawn too."""
    def side(moved):
        n = int(rng.integers(1, 12))
        start = rng.integers(1, 301, n)
        end = start + rng.integers(3, 61, n)
        pitch = rng.integers(58, 64, n).astype(np.float64)
        if moved:
            pitch = pitch + rng.choice([0.0, 0.3, -0.3, 0.5, -0.5], n)
        return np.stack([SC.frame_time(start), SC.frame_time(end), pitch], axis=1)

    est, ref = side(False), side(True)
    n_frames = int(rng.choice(N_FRAMES))
    tol = dict(pitch_tolerance_cents=float(rng.choice(TOLERANCES)), strict=int(rng.integers(0, 2)))
    return est, ref, n_frames, tol


def seeded_cases(n=2000, seed=0):
    rng = np.random.default_rng(seed)
    return [random_case(rng) for _ in range(n)]


# The minimal chain of the frame level: ests 60 and 61, refs 60.5 (hits both at exactly 50 cents) and 60.4 (hits 60 alone), all
# over the same frames.  The maximum is 2 on every frame; a first fit that gives 60.5 the est 60 strands 60.4.
CHAIN_ESTS, CHAIN_REFS = [(60.0,), (61.0,)], [(60.5,), (60.4,)]


def chains(start=SC.frame_time(10), end=SC.frame_time(30)):
    """The four orders: (est rows, ref rows)."""
    rows = lambda pitches: SC.notes([(start, end, p[0]) for p in pitches])  # noqa: E731
    return [(rows(e), rows(r)) for e in (CHAIN_ESTS, CHAIN_ESTS[::-1]) for r in (CHAIN_REFS, CHAIN_REFS[::-1])]
