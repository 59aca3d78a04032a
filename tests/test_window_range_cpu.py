"""The window cutting of `inference.predict_window_range` (the window-range fallback of the sharded job) without a GPU: a stub
model that exposes what the function reads of a `Model` — `sample_rate`, `audio_n_samples`, `max_windows`, `resample`,
`predict` — and records what `predict` is given.  The windows must be those of the model's own geometry: window length from
the model, hop 36,164 and lead-in 3,840 samples times rate / 22,050 (87,688 / 72,328 / 7,680 for the extended 44.1 kHz range),
and `assemble_window_ranges` must trim to int(L / hop * 142) rows with that hop.  A model-shaped object that has neither
attribute keeps the reference's geometry."""
import numpy as np
import pytest

import clip_files as CF

WIDTHS = (("note", 88), ("onset", 88), ("contour", 264))


class Stub:
    """`predict` returns maps whose every row holds window number * 172 + frame, so the assembled rows name their source."""

    def __init__(self, rate=None, win=None, max_windows=2):
        if rate is not None:
            self.sample_rate, self.audio_n_samples = rate, win
        self.max_windows = max_windows
        self.seen = []  # the batches predict was given
        self._at = 0

    def resample(self, pcm, sr):
        self.file_rate = sr
        return np.asarray(pcm, np.float32).mean(axis=1, dtype=np.float32)

    def predict(self, x):
        x = np.array(x, np.float32)
        self.seen.append(x)
        rows = (self.first + self._at + np.arange(x.shape[0]))[:, None] * 172 + np.arange(172)[None, :]
        self._at += x.shape[0]
        return {k: np.repeat(rows[:, :, None], w, axis=2).astype(np.float32) for k, w in WIDTHS}


@pytest.mark.parametrize("rate,win,hop,lead", [(44100, 87688, 72328, 7680), (22050, 43844, 36164, 3840), (None, 43844, 36164, 3840)])
@pytest.mark.parametrize("n", [3 * 72328 - 7680 + 1, 2 * 72328 + 555, 5000])
def test_windows_are_cut_with_the_models_own_geometry(tmp_path, rate, win, hop, lead, n):
    from basic_pitch_amd import inference as I
    from basic_pitch_amd.sharding import split_windows

    file_rate = rate or 22050
    x = CF.tones(n, 1, file_rate, 3) * 0.5
    path = CF.write_wav(tmp_path / "x.wav", x, "f32", file_rate)  # float32 samples: the file's values are the track's
    y = x.astype(np.float32)[:, 0]
    padded = np.concatenate([np.zeros(lead, np.float32), y, np.zeros(win + hop, np.float32)])
    n_windows = -(-(n + lead) // hop)
    parts = []
    for piece in range(2):
        m = Stub(rate, win)
        w0, w1 = split_windows(n_windows, 2)[piece]
        m.first = w0
        part = I.predict_window_range(path, m, piece, 2)
        assert m.file_rate == file_rate
        assert part["range"] == (w0, w1) and part["n_windows"] == n_windows and part["original_length"] == n
        assert [b.shape for b in m.seen] == [(min(2, w1 - a), win) for a in range(w0, w1, 2)], (rate, piece)
        got = np.concatenate(m.seen) if m.seen else np.zeros((0, win), np.float32)
        for w in range(w0, w1):
            assert np.array_equal(got[w - w0], padded[w * hop : w * hop + win]), (rate, w)
        for k, width in WIDTHS:
            assert part["rows"][k].shape == ((w1 - w0) * 142, width)
        parts.append(part)
    out, _, _ = I.assemble_window_ranges(parts[::-1], onset_threshold=1e9)  # (the stub's maps are row numbers, not probabilities)
    T = int(n / hop * 142)
    assert T > 0
    want = (np.arange(n_windows)[:, None] * 172 + np.arange(15, 157)[None, :]).reshape(-1)[:T]
    for k, width in WIDTHS:
        assert out[k].shape == (T, width) and np.array_equal(out[k][:, 0], want.astype(np.float32)), (rate, k)


def test_the_geometry_of_a_model_shaped_object():
    from basic_pitch_amd import inference as I

    assert I._window_geometry(object()) == (43844, 36164, 3840)
    assert I._window_geometry(Stub(22050, 43844)) == (43844, 36164, 3840)
    assert I._window_geometry(Stub(44100, 87688)) == (87688, 72328, 7680)
