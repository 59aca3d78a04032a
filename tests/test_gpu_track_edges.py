"""`predict_track` — the root that every other entry point is held to — against the reference's windowing at the lengths where
the geometry changes (tests/track_cases.py), on handles that cut a track into pieces and whose buffers hold other data.

The reference windowing is `oracle.bp_oracle.window_track` / `unwrap_output` (inference.py:194-279) around `predict` of a
separate handle of the same mode with max_windows = 8, the suite's small-batch truth (tests/test_gpu_launch_regimes.py).
Every comparison is of the float32 bit patterns: there is no tolerance.  tests/test_track_cases_cpu.py shows on the same
lengths and signals that an error in the lead-in, in a piece's first sample, in the tail or in the trim changes the result.

Before every call under test `track_cases.dirty` predicts max_windows windows of full-scale noise on the handle.

Tried once on an MI355X against four builds of the library with one such error planted each (none reads or writes out of
bounds): a piece that starts one sample late from window 1 on (`tracks_core`) fails (a) with max_windows 1 and 2 and (b),
and passes where every track is one piece; a lead-in of L + 1, a tail that is left as the buffer held it (`gather_window`)
and a trim one row short when the last kept window is partial (`scatter_window`) each fail all 23 tests of this file."""
import numpy as np
import pytest
import torch

import track_cases as TC
from oracle import bp_oracle as O
from test_gpu_mode_matrix import frames_for, s16

pytestmark = pytest.mark.gpu

MODES = ("default", "bf16_weights", "ext_cqt_44k")
MAPS = ("note", "onset", "contour")
MAX_TRACK_SEGS = 16  # kMaxTrackSegs (csrc/bp_common.h): pieces one windowing / un-overlapping launch describes


class Handles:
    """Handles by (mode, max_windows, role), made when first asked for; and per mode the reference windowing's result for
    `track_cases.signal(n)` and for any other signal the tests name, computed once and read-only from then on."""

    def __init__(self):
        self.made, self.wanted = {}, {}

    def get(self, mode, max_windows, role="tested"):
        from basic_pitch_amd.inference import Model

        key = (mode, max_windows, role)
        if key not in self.made:
            self.made[key] = Model(device=0, max_windows=max_windows, **({} if mode == "default" else {mode: True}))
        return self.made[key]

    def signal(self, mode, n):
        return TC.signal(n, 1, self.get(mode, 8, "reference").sample_rate)

    def reference(self, mode, y, name=None):
        """unwrap_output(ref.predict(window_track(y)), len(y)) with the geometry of the mode's handle."""
        key = (mode, name if name is not None else len(y))
        if key not in self.wanted:
            ref = self.get(mode, 8, "reference")
            win, hop, lead = TC.geometry(ref)
            wins, n = O.window_track(y, win=win, hop=hop, lead=lead)
            assert n == len(y) and 1 <= wins.shape[0] <= 8
            maps = ref.predict(wins)
            out = {k: np.ascontiguousarray(O.unwrap_output(maps[k], n, win=win, hop=hop, lead=lead)) for k in MAPS}
            for v in out.values():
                assert v.shape[0] == 0 or np.ptp(v) > 0  # a map that is constant could hide a misplaced row
                v.setflags(write=False)
            self.wanted[key] = out
        return self.wanted[key]

    def want(self, mode, n):
        """(signal(n), its reference result)"""
        y = self.signal(mode, n)
        return y, self.reference(mode, y)

    def close(self):
        for m in self.made.values():
            m.close()


@pytest.fixture(scope="module")
def handles():
    h = Handles()
    yield h
    h.close()


def host(maps):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in maps.items()}


def same(got, want, what, rows=None):
    got = host(got)
    for k in MAPS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        if rows is not None:
            assert got[k].shape[0] == rows, (what, k, got[k].shape, rows)
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)


def handle_rows(m, n):
    return int(m._lib.bp_handle_track_n_frames(m._handle, n))


# ---- a: one track per call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_windows", [1, 2, 8])
@pytest.mark.parametrize("mode", MODES)
def test_a_track_equals_the_reference_windowing(handles, mode, max_windows):
    """With max_windows 1 and 2 the tracks of three to five windows are cut into pieces that start inside the track
    (`w0 * hop - lead`), with 8 every track is one piece.  The row count is the handle's, which for the extended geometry is
    held to the oracle's windowing here and nowhere else."""
    m = handles.get(mode, max_windows)
    win, hop, lead = TC.geometry(m)
    pieces = 0
    for on_device in (False, True):
        for n in TC.lengths(hop, lead):
            y, want = handles.want(mode, n)
            assert want["note"].shape[0] == TC.n_rows(n, hop, lead)
            TC.dirty(m)
            got = m.predict_track(torch.from_numpy(y).cuda() if on_device else y)
            same(got, want, (mode, max_windows, n, "device" if on_device else "host"), rows=handle_rows(m, n))
            pieces = max(pieces, -(-TC.n_windows(n, hop, lead) // max_windows))
    assert pieces == {1: 5, 2: 3, 8: 1}[max_windows]


# ---- b: many tracks per call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_packed_tracks_equal_the_reference_windowing(handles, mode):
    """All lengths in one `predict_tracks` call, in the list's order and reversed (the pieces of neighbouring tracks share the
    chunks of 8 windows at other cuts), from host and from device memory; then 40 tracks drawn from the list through a
    handle of 64 windows, whose first chunk holds more pieces than one windowing launch describes."""
    m = handles.get(mode, 8)
    win, hop, lead = TC.geometry(m)
    ns = TC.lengths(hop, lead)

    def check(model, order, on_device, what):
        tracks = [handles.signal(mode, n) for n in order]
        TC.dirty(model)
        got = model.predict_tracks([torch.from_numpy(y).cuda() for y in tracks] if on_device else tracks)
        assert len(got) == len(order)
        for n, y, g in zip(order, tracks, got):
            same(g, handles.reference(mode, y), (mode, what, n, "device" if on_device else "host"), rows=handle_rows(model, n))

    for order, what in ((ns, "list order"), (ns[::-1], "reversed")):
        for on_device in (False, True):
            check(m, order, on_device, what)
    big = handles.get(mode, 64)
    drawn = [int(n) for n in np.random.default_rng(17).choice(ns, 40)]
    ends = np.cumsum([TC.n_windows(n, hop, lead) for n in drawn])
    assert int(np.searchsorted(ends, 64)) + 1 > MAX_TRACK_SEGS and ends[-1] > 64  # pieces of the first chunk; a second chunk
    for on_device in (False, True):
        check(big, drawn, on_device, "40 tracks in chunks of 64")


# ---- c: ingest, then the track ----------------------------------------------------------------------------------------------------
# (input rate, mode, the resampling kernel `launch_resample` (csrc/audio_ingest.hip) takes for it).  The kernel follows from
# the filter design, restated in `kernel_reached`: 8 : 1 has 1,541 taps, too many for the tiled kernel's LDS table, but a
# block's 256 outputs still reach fewer than 4,096 inputs; from 16 : 1 on they do not, and the one-thread-per-output kernel runs.
PCM_CASES = (
    (44100, "default", "2 : 1"),
    (11025, "default", "tiled, taps in LDS"),
    (48000, "default", "tiled"),
    (176400, "default", "tiled"),
    (352800, "default", "one thread per output"),
    (44101, "default", "taps in place"),
    (48000, "ext_cqt_44k", "tiled"),
    (352800, "ext_cqt_44k", "tiled"),
    (705600, "ext_cqt_44k", "one thread per output"),
)


def kernel_reached(sr, rate):
    """launch_resample's choice in the product library, from the tap count of the filter design (make_resample_plan,
    csrc/audio_ingest.hip; the same formulas as `audio.soxr_hq_taps`, without making the taps)."""
    from fractions import Fraction

    from basic_pitch_amd import audio as A

    fr = Fraction(rate, sr)
    up, down = fr.numerator, fr.denominator
    db = 20.0 * np.log10(2.0)
    rej, att = 20.0 * db, 21.0 * db
    fp = 1.0 - 0.05 / ((1.6e-6 * rej - 7.5e-4) * rej + 0.646)
    tr_bw = 0.5 * (1.0 - fp) / max(up, down)
    fc = 1.0 / max(up, down) - tr_bw
    realm = np.log2(tr_bw * 0.5 / fc / 0.0005)
    r0, r1 = (int(np.clip(int(realm) + d, 0, 9)) for d in (0, 1))
    b0, b1 = (((c[0] * att + c[1]) * att + c[2]) * att + c[3] for c in (A._BETA_FIT[r0], A._BETA_FIT[r1]))
    beta = b0 + (b1 - b0) * (realm - int(realm))
    n_taps = int(np.ceil((((0.0007528358 - 1.577737e-05 * beta) * beta + 0.6248022) * beta + 0.06186902) / tr_bw + 1))
    n_taps = (n_taps + 2) // 4 * 4 + 1
    if max(up, down) <= 16:
        assert n_taps == len(A.soxr_hq_taps(up, down))
    if n_taps > 1 << 22:
        return "taps in place"
    if (up, down) == (1, 2):
        return "2 : 1"
    span = (255 * down + n_taps - 1) // up + 2
    if span > 4096:
        return "one thread per output"
    return "tiled, taps in LDS" if n_taps <= 1024 else "tiled"


def stereo(frames, sr, seed):
    """Two channels of `track_cases.signal` as 16-bit PCM [frames, 2] and the float32 samples they stand for."""
    pcm = s16(np.stack([TC.signal(frames, seed, sr), TC.signal(frames, seed + 1, sr)], axis=1))
    return pcm, pcm.astype(np.float32) / np.float32(32768)


@pytest.mark.parametrize("sr,mode,kernel", PCM_CASES)
def test_pcm_calls_equal_resample_then_track_at_the_edges(handles, sr, mode, kernel):
    """Input lengths whose resampled length is H - L (one window), H - L + 1 (two) and 2 H + H / 3 (three).  Doubling the
    rate gives even lengths only: from 11,025 Hz the second length is H - L + 2, the first one that has two windows."""
    from basic_pitch_amd import _native

    m = handles.get(mode, 8)
    rate = m.sample_rate
    win, hop, lead = TC.geometry(m)
    assert kernel_reached(sr, rate) == kernel
    resampled = lambda frames: int(m._lib.bp_handle_resampled_length(m._handle, frames, sr))  # noqa: E731
    for target, windows in ((hop - lead, 1), (hop - lead + 1, 2), (2 * hop + hop // 3, 3)):
        frames = frames_for(target, sr, rate)
        if resampled(frames) != target:
            assert 2 * sr == rate and target % 2 == 1
            frames, target = frames + 1, target + 1
        assert resampled(frames) == target and TC.n_windows(target, hop, lead) == windows
        pcm, f32 = stereo(frames, sr, 31)
        what = (sr, mode, target)
        TC.dirty(m)
        y = m.resample(f32, sr)
        assert y.shape == (target,)
        TC.dirty(m)
        track = m.predict_track(y)
        same(track, handles.reference(mode, y, name=what), what + ("track",), rows=handle_rows(m, target))
        TC.dirty(m)
        same(m.predict_pcm(f32, sr), track, what + ("predict_pcm",))
        TC.dirty(m)
        same(m.predict_pcm_raw(pcm, _native.BP_PCM_S16, frames, 2, sr), track, what + ("predict_pcm_raw",))


@pytest.mark.parametrize("mode", ["default", "ext_cqt_44k"])
def test_mono_samples_at_the_model_rate_go_straight_through(handles, mode):
    """bp_infer_pcm of mono float samples at the handle's own rate: from device memory the track is windowed straight from
    the caller's buffer (no downmix, no resampling, no staging copy), from host memory from the ingest's staging."""
    from basic_pitch_amd import _native
    from basic_pitch_amd.inference import _empty_maps

    m = handles.get(mode, 8)
    win, hop, lead = TC.geometry(m)
    for n in (hop - lead + 1, 2 * hop + hop // 3):
        y, want = handles.want(mode, n)
        TC.dirty(m)
        track = m.predict_track(y)
        same(track, want, (mode, n, "track"))
        TC.dirty(m)
        same(m.predict_pcm(y, m.sample_rate), track, (mode, n, "host"))
        x = torch.from_numpy(y).cuda()
        out = _empty_maps((handle_rows(m, n),), x.device)
        TC.dirty(m)
        torch.cuda.synchronize()
        rc = m._lib.bp_infer_pcm(m._handle, x.data_ptr(), n, 1, m.sample_rate, *[out[k].data_ptr() for k in MAPS], _native.BP_MEM_DEVICE)
        _native.check(m._lib, m._handle, rc, "bp_infer_pcm")
        same(out, track, (mode, n, "device"))
