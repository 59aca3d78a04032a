"""The track lengths of tests/track_cases.py, without a device: the library's handle-free geometry gives the reference
windowing's counts at every one of them, the list enters every class of the geometry it claims, and — the condition under
which the bit-for-bit equalities of tests/test_gpu_track_edges.py can fail at all — every planted error of the windowing
changes the result on `track_cases.signal`.

The stand-in for the model (`stand_in`) is a deterministic map of a window to (172, 88): frame f is a sum of |x| over the
frame's hop (256 samples; 512 in the extended geometry) with a fixed weight per position and bin, plus halves and quarters of
the frames one and two to either side.  Position weights, because a plain sum over a frame does not see a shift inside it;
neighbours, because a row of the real model depends on far more than the samples under it (the CQT's kernels are longer than
a frame, the CNN spans seven frames) and the last kept row can end up to one frame before the track does.

Where a planted error can show follows from the geometry alone (track_cases' docstring), not from any code under test:
  * every planted windowing differs from the correct one in the windows themselves, at every length it applies to;
  * in the kept rows it shows only where rows are kept of a window it touches: a wrong lead-in and a stale tail at every
    length with rows (all but 1 and R - 1), a wrong start from window 1 on at every length with more than 142 rows — up to
    n = H + 1 all kept rows are window 0's and window 1 is computed and thrown away, on the device too;
  * a trim one row long or short shows in the shape, at every length with rows."""
import numpy as np
import pytest

import track_cases as TC
from oracle import bp_oracle as O

DEFAULT = (O.AUDIO_N_SAMPLES, O.HOP_SIZE, O.OVERLAP_LEN // 2)
EXTENDED = (O.EXT_AUDIO_N_SAMPLES, 2 * O.HOP_SIZE, O.OVERLAP_LEN)
GEOMETRIES = pytest.mark.parametrize("win,hop,lead", [DEFAULT, EXTENDED], ids=["default", "extended"])


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


def test_geometries_are_the_reference_s_and_its_double():
    assert DEFAULT == (43844, 36164, 3840) and EXTENDED == (87688, 72328, 7680)
    assert TC.lengths(36164, 3840)[:2] == [254, 255] and TC.lengths(72328, 7680)[:2] == [509, 510]
    for win, hop, lead in (DEFAULT, EXTENDED):
        ns = TC.lengths(hop, lead)
        assert len(set(ns)) == len(ns) == 19 and min(ns) == 1
    y = TC.signal(5000, 3)
    assert np.array_equal(y, TC.signal(5000, 3)) and not np.array_equal(y, TC.signal(5000, 4)) and np.abs(y).max() <= 0.8


# ---- counts ------------------------------------------------------------------------------------------------------------------
def oracle_counts(n, win, hop, lead):
    """(windows, rows) of the oracle's windowing and un-overlapping of n samples."""
    wins, n_orig = O.window_track(np.ones(n, np.float32), win=win, hop=hop, lead=lead)
    assert n_orig == n and wins.shape[1] == win
    rows = O.unwrap_output(np.zeros((wins.shape[0], 172, 1), np.float32), n, win=win, hop=hop, lead=lead).shape[0]
    return wins.shape[0], rows


def test_library_counts_equal_the_oracle_windowing(lib):
    win, hop, lead = DEFAULT
    for n in TC.lengths(hop, lead):
        n_win, rows = oracle_counts(n, win, hop, lead)
        assert lib.bp_track_n_windows(n) == n_win, n
        assert lib.bp_track_n_frames(n) == rows, n


@GEOMETRIES
def test_shared_formulas_equal_the_oracle_windowing(win, hop, lead):
    for n in TC.lengths(hop, lead):
        assert (TC.n_windows(n, hop, lead), TC.n_rows(n, hop, lead)) == oracle_counts(n, win, hop, lead), n


# ---- coverage ----------------------------------------------------------------------------------------------------------------
@GEOMETRIES
def test_the_list_enters_every_class_it_claims(win, hop, lead):
    H, L, R = hop, lead, TC.first_row_length(hop)
    ns = TC.lengths(hop, lead)
    count = {n: oracle_counts(n, win, hop, lead) for n in ns}
    assert sorted({c[0] for c in count.values()}) == [1, 2, 3, 4, 5]
    for below, windows in ((H - L, 1), (2 * H - L, 2), (3 * H - L, 3)):
        assert below in ns and below + 1 in ns
        assert count[below][0] == windows and count[below + 1][0] == windows + 1, below
    assert count[R - 1][1] == 0 and count[R][1] == 1
    assert count[1] == (1, 0)
    # the last window of a track is never whole (n <= windows * H - L, and a whole last window needs n >= windows * H + L):
    # every length has a tail of zeros
    for n in ns:
        assert (count[n][0] - 1) * H - L + win > n
    # rows of window 1 are kept from W on, of window 0 alone up to H + 1
    assert [n for n in ns if count[n][0] >= 2 and count[n][1] <= TC.ROWS] == [H - L + 1, H - 1, H, H + 1]
    assert sum(count[n][1] > TC.ROWS for n in ns) == 7


# ---- power -------------------------------------------------------------------------------------------------------------------
def planted_windows(y, win, hop, lead, lead_err=0, start_err=0, tail=None):
    """The windowing written out per sample, with errors to plant.  lead_err: the lead-in is L + lead_err samples; start_err:
    windows 1.. start that many samples late; tail: what lies behind the track's end instead of zeros — "call": what the
    slot held before (the windows `track_cases.dirty` predicts), "window": the samples of the window before it (before
    window 0: the last call's)."""
    n = len(y)
    n_win = TC.n_windows(n, hop, lead)
    stale = TC.dirty_windows(n_win, win)
    out = np.zeros((n_win, win), np.float32)
    for w in range(n_win):
        at = w * hop - (lead + lead_err) + (start_err if w else 0) + np.arange(win)
        inside = (at >= 0) & (at < n)
        out[w, inside] = y[at[inside]]
        behind = at >= n
        if tail == "call":
            out[w, behind] = stale[w, behind]
        elif tail == "window":
            out[w, behind] = (out[w - 1] if w else stale[0])[behind]
    return out


def stand_in(wins):
    """(n, W) -> (n, 172, 88) in float64; see the module's docstring."""
    n, win = wins.shape
    fh = 256 * (win // O.AUDIO_N_SAMPLES)
    x = np.zeros((n, 172 * fh))
    x[:, :win] = np.abs(wins)
    weights = np.random.default_rng(1234).uniform(0.5, 1.5, (fh, 88))
    p = np.zeros((n, 172 + 4, 88))
    p[:, 2:-2] = x.reshape(n, 172, fh) @ weights
    return p[:, 2:-2] + 0.5 * (p[:, 1:-3] + p[:, 3:-1]) + 0.25 * (p[:, :-4] + p[:, 4:])


def rows_of(wins, n, win, hop, lead, trim_err=0):
    maps = stand_in(wins)
    if trim_err == 0:
        return O.unwrap_output(maps, n, win=win, hop=hop, lead=lead)
    flat = maps[:, 15:157].reshape(-1, 88)
    keep = TC.n_rows(n, hop, lead) + trim_err
    assert 0 <= keep <= flat.shape[0]  # a trim that a wrong `left < 142` could produce
    return flat[:keep]


@GEOMETRIES
def test_every_planted_error_of_the_windowing_changes_the_result(win, hop, lead):
    geo = (win, hop, lead)
    tried = {"lead": 0, "start": 0, "tail": 0, "trim": 0}
    for n in TC.lengths(hop, lead):
        y = TC.signal(n, 1, 22050 * (win // O.AUDIO_N_SAMPLES))
        right = planted_windows(y, *geo)
        assert np.array_equal(right, O.window_track(y, win=win, hop=hop, lead=lead)[0]), n
        good = rows_of(right, n, *geo)
        n_win, rows = right.shape[0], good.shape[0]
        assert (n_win, rows) == (TC.n_windows(n, hop, lead), TC.n_rows(n, hop, lead))

        def shows(wins, in_rows, what):
            assert wins.shape == right.shape and not np.array_equal(wins, right), (n, what, "windows")
            got = rows_of(wins, n, *geo)
            assert got.shape == good.shape
            assert np.array_equal(got, good) != in_rows, (n, what, "rows")

        for err in (-1, 1):
            shows(planted_windows(y, *geo, lead_err=err), rows > 0, ("lead-in", err))
            tried["lead"] += 1
            if n_win >= 2:
                shows(planted_windows(y, *geo, start_err=err), rows > TC.ROWS, ("start of windows 1..", err))
                tried["start"] += 1
            if rows > 0:
                assert rows_of(right, n, *geo, trim_err=err).shape != good.shape, (n, "trim", err)
                tried["trim"] += 1
        for tail in ("call", "window"):
            shows(planted_windows(y, *geo, tail=tail), rows > 0, ("stale tail", tail))
            tried["tail"] += 1
    # 19 lengths: all have a lead-in and a tail, 11 two windows or more, 17 rows; two errors of each kind at each
    assert tried == {"lead": 38, "start": 22, "tail": 38, "trim": 34}
