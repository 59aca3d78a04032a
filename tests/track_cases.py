"""What the track tests share (tests/test_track_cases_cpu.py, tests/test_gpu_track_edges.py): the track lengths at which the
windowing's geometry changes, a signal in which no sample is zero, and a call that leaves other data in a handle's buffers.
Nothing here needs a device until `dirty` is called.

The geometry, with H = hop, L = lead-in, W = H + 2 L the window (the reference's inference.py:194-279; 36,164 / 3,840 / 43,844
at 22.05 kHz, doubled for the extended 44.1 kHz handle): a track of n samples has ceil((n + L) / H) windows, window w holds
samples [w H - L, w H - L + W) with zeros outside [0, n), every window gives 142 rows (its frames 15..156) and the first
int(n / H * 142) rows of them are kept."""
import functools

import numpy as np

ROWS = 142  # rows kept of a window's 172 frames


def geometry(m):
    """(window, hop, lead-in) of a handle: the window from the handle, hop and lead-in the reference's times rate / 22050."""
    rate, win = m.sample_rate, m.audio_n_samples
    assert rate % 22050 == 0
    hop, lead = 36164 * rate // 22050, 3840 * rate // 22050
    assert win == hop + 2 * lead
    return win, hop, lead


def n_windows(n, hop, lead):
    return -(-(n + lead) // hop) if n > 0 else 0


def n_rows(n, hop, lead):
    return min(n_windows(n, hop, lead) * ROWS, int(n / hop * ROWS))


def first_row_length(hop):
    """R = ceil(H / 142): the first length that keeps a row."""
    return -(-hop // ROWS)


def lengths(hop, lead):
    """The lengths at which the geometry changes, and one generic length of five windows."""
    H, L, W, R = hop, lead, hop + 2 * lead, first_row_length(hop)
    return [
        R - 1, R,  # no row / the first row
        1,  # the smallest track
        L - 1, L, L + 1,  # the lead-in boundary
        H - L - 1, H - L, H - L + 1,  # one window -> two
        H - 1, H, H + 1,  # one hop
        W,  # one window's length
        2 * H - L, 2 * H - L + 1,  # two windows -> three
        2 * H,  # two hops
        3 * H - L, 3 * H - L + 1,  # three windows -> four
        4 * H + H // 3 + 17,  # five windows, nothing special
    ]


def signal(n, seed=0, rate=22050):
    """n float32 samples of noise in +-0.5 plus a 440 Hz tone of 0.3, none of them zero: a window that is read one sample
    off, or that holds zeros where signal belongs, is another window."""
    rng = np.random.default_rng([seed, n])
    y = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    y += (0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)).astype(np.float32)
    y[y == 0] = np.float32(0.25)
    assert y.dtype == np.float32 and not (y == 0).any()
    return y


@functools.lru_cache(maxsize=8)
def dirty_windows(n_win, win, seed=99):
    """What `dirty` predicts: n_win windows of full-scale noise (read-only: one array per shape)."""
    x = np.random.default_rng(seed).uniform(-1, 1, (n_win, win)).astype(np.float32)
    x.setflags(write=False)
    return x


def dirty(model):
    """Predict `max_windows` windows of full-scale noise: afterwards every slot of the handle's window buffer, of its maps and
    of its staging holds other data than zeros or the next call's."""
    out = model.predict(dirty_windows(model.max_windows, model.audio_n_samples))
    assert out["note"].shape[0] == model.max_windows
