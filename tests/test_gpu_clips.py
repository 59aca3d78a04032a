"""Many clips in one call on the GPU (bp_clips_row_offsets / bp_infer_clips_candidates, include/basic_pitch_amd_clips.h;
Model.transcribe_clips): clip by clip the bytes are those of bp_infer_pcm_raw_candidates on the clip alone with the same
handle, for any grouping of the clips.

The handles have max_windows = 8, so chunks flush inside clips and several clips share a chunk.  A chunk of 8 windows cannot
hold more than kMaxTrackSegs = 16 pieces, so the byte comparison runs once more on a handle of 32 windows, where the 17
adjacent one-window clips share one chunk."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import note_oracle as NO

pytestmark = pytest.mark.gpu

HOP, LEAD = 36164, 3840
# model-rate lengths: 0 rows (no samples; one sample), 1, 2, 3, 141, 142 (twice) and 143 rows; one window - 1, exactly, + 1
# sample (ceil((n + 3840) / 36164) windows); two windows + 1 sample
EDGE = (0, 1, 255, 510, 765, 36163, 36164, 36165, 36419, 32323, 32324, 32325, 2 * HOP - LEAD + 1)
SHORT = tuple(255 + 37 * i for i in range(17))  # 17 adjacent one-window clips of 1 to 3 rows


def _signal(rng, n, rate):
    """Low-level noise with a few sines that start and stop inside the clip (notes to find), float64 in [-1, 1]."""
    t = np.arange(n) / rate
    x = 2e-3 * rng.standard_normal(n)
    for _ in range(3):
        f = 110.0 * 2 ** (rng.integers(0, 40) / 12.0)
        a, b = sorted(rng.uniform(0, max(n, 1) / rate, 2))
        x += rng.uniform(0.1, 0.3) * np.sin(2 * np.pi * f * t) * ((t >= a) & (t < b))
    return x


def _make_clips():
    rng = np.random.default_rng(2024)
    clips, rates = [], []
    a_len = list(EDGE[:6]) + list(SHORT) + list(EDGE[6:])  # 30 clips at 44.1 kHz stereo S16
    assert len(a_len) == 30
    for k, n in enumerate(a_len):
        f = max(0, 2 * n - (k % 2))  # ceil(f / 2) = n either way
        x = np.stack([_signal(rng, f, 44100), _signal(rng, f, 44100)], axis=1) if f else np.zeros((0, 2))
        clips.append(np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16))
        rates.append(44100)
    for n in (0, 255, 36164, 36419, 32325, 2 * HOP - LEAD + 1, 510, 765, 1, 32324):  # 10 at 22.05 kHz mono F32
        clips.append(_signal(rng, n, 22050).astype(np.float32))
        rates.append(22050)
    order = rng.permutation(len(clips))  # the two groups interleaved: the Python layer sorts them out
    keep_short = [i for i in order if not 6 <= i < 23]
    at = len(keep_short) // 2
    order = keep_short[:at] + list(range(6, 23)) + keep_short[at:]  # ... the 17 short ones stay adjacent
    return [clips[i] for i in order], [rates[i] for i in order]


@pytest.fixture(scope="module")
def job():
    return _make_clips()


@pytest.fixture(scope="module")
def nat():
    from basic_pitch_amd import _native

    return _native


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _prm(nat, lib, limits=False, bends=1, onset=None):
    prm = nat.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    prm.include_pitch_bends = bends
    if limits:
        prm.min_freq_hz, prm.max_freq_hz = 100.0, 1500.0
    if onset is not None:
        prm.onset_threshold = onset
    return prm


def _single(m, nat, a, rate, prm):
    """bp_infer_pcm_raw_candidates on one clip alone: (note, bits, bend, status)."""
    from basic_pitch_amd import clips as CL

    T = m._pcm_frames(a.shape[0], rate)
    note, bits, bend = np.full((T, 88), -7, np.float32), np.full((T, 12), 0xAA, np.uint8), np.full((T, 88), 99, np.int8)
    status = C.c_int(-1)
    rc = m._lib.bp_infer_pcm_raw_candidates(m._handle, a.ctypes.data if a.size else None, CL.FORMATS[a.dtype], a.shape[0], a.shape[1],
                                            rate, C.byref(prm), note.ctypes.data, bits.ctypes.data, bend.ctypes.data, C.byref(status))
    nat.check(m._lib, m._handle, rc, "bp_infer_pcm_raw_candidates")
    return note, bits, bend, status.value


def _batched(m, nat, arrays, rate, prm):
    """One bp_infer_clips_candidates call; the outputs pre-filled, so rows the call does not write show."""
    from basic_pitch_amd import clips as CL

    lib = CL.bind(m._lib)
    tab = CL.clip_table(arrays)
    offs = CL.clips_row_offsets(m, arrays, rate)
    T = int(offs[-1])
    note, bits, bend = np.full((T, 88), -7, np.float32), np.full((T, 12), 0xAA, np.uint8), np.full((T, 88), 99, np.int8)
    status = np.full(len(arrays), -1, np.int32)
    rc = lib.bp_infer_clips_candidates(m._handle, len(arrays), tab, rate, nat.BP_MEM_HOST, C.addressof(prm), note.ctypes.data,
                                       bits.ctypes.data, bend.ctypes.data, status.ctypes.data)
    nat.check(lib, m._handle, rc, "bp_infer_clips_candidates")
    return offs, note, bits, bend, status


def _compare_with_single(m, nat, arrays, rate, prm, skip_bits_of=()):
    offs, note, bits, bend, status = _batched(m, nat, arrays, rate, prm)
    for i, a in enumerate(arrays):
        r0, r1 = int(offs[i]), int(offs[i + 1])
        n1, b1, d1, s1 = _single(m, nat, a, rate, prm)
        assert r1 - r0 == n1.shape[0], i
        assert status[i] == s1, (i, a.shape)
        assert note[r0:r1].tobytes() == n1.tobytes(), (i, a.shape)
        if i not in skip_bits_of:
            assert bits[r0:r1].tobytes() == b1.tobytes(), (i, a.shape)
        assert bend[r0:r1].tobytes() == d1.tobytes(), (i, a.shape)  # include_pitch_bends 0: neither call writes it
    return offs, note, bits, bend, status


@pytest.mark.parametrize("max_windows", [8, 32])
def test_the_bytes_of_every_clip_are_those_of_the_single_clip_call(model, nat, job, max_windows):
    from basic_pitch_amd import clips as CL
    from basic_pitch_amd.inference import Model

    m = model if max_windows == 8 else Model(device=0, max_windows=max_windows)
    try:
        arrays, rates = [CL.as_clip(c, i) for i, c in enumerate(job[0])], job[1]
        rows = set()
        for rate in (44100, 22050):
            group = [a for a, r in zip(arrays, rates) if r == rate]
            assert len(group) == (30 if rate == 44100 else 10)
            for limits, bends in ((False, 1), (True, 1), (False, 0), (True, 0)) if max_windows == 8 else ((True, 1),):
                offs, note, _, _, status = _compare_with_single(m, nat, group, rate, _prm(nat, m._lib, limits, bends))
                rows |= set(np.diff(offs).tolist())
                assert not status.any() and np.isfinite(note).all()
        assert {0, 1, 2, 3, 141, 142, 143} <= rows
        # status 1 without a NaN: an onset threshold <= 0, for every clip that has rows, the bytes still the single call's
        group = [a for a, r in zip(arrays, rates) if r == 22050]
        offs, _, _, _, status = _compare_with_single(m, nat, group, 22050, _prm(nat, m._lib, onset=0.0))
        assert np.array_equal(status, (np.diff(offs) > 0).astype(np.int32))
    finally:
        if m is not model:
            m.close()


@pytest.fixture(scope="module")
def ab(nat):
    from basic_pitch_amd import build

    lib = nat.load_library(build.build_library(ab=True))
    lib.bp_ab_clips_candidates_from_maps.restype = C.c_int
    lib.bp_ab_clips_candidates_from_maps.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)] + [C.c_void_p] * 8
    return lib


def _boundary_sets():
    """Two handcrafted jobs of clips' maps: (lengths, note, onset, contour)."""
    rng = np.random.default_rng(11)

    def base(T):
        return (rng.uniform(0, 0.02, (T, 88)).astype(np.float32), rng.uniform(0, 0.02, (T, 88)).astype(np.float32),
                rng.uniform(0, 1, (T, 264)).astype(np.float32))

    # (a) clip 0 ends on its highest onset (bin 10: a peak only if the next clip's first row counted as its neighbour and were
    # lower — bin 11: lower; bin 10: higher, which would make THAT row a peak of clip 1 with clip 0's row as its neighbour);
    # interior peaks in both clips keep the bitmaps from being empty.  One-row and empty clips sit between clips too.
    lens_a = (7, 6, 1, 0, 5)
    n, o, c = base(sum(lens_a))
    o[3, 40], o[6, 10], o[6, 11] = 0.8, 0.9, 0.9
    o[7, 10], o[7, 11], o[8, 10], o[8, 11] = 0.95, 0.6, 0.7, 0.5
    o[10, 50] = 0.85
    o[13, 20] = 0.99  # the one-row clip: no neighbours at all
    o[16, 30] = 0.7
    # a real rise of the note map in every clip of three rows or more (its third row on): the inferred onsets are scaled by it
    # and the noise floor stays far below the threshold
    n[2:7, 40], n[9:13, 50], n[16:19, 30] = 0.6, 0.5, 0.5
    # (b) clip 1 starts loud after a quiet clip 0: rows 0 and 1 of clip 1 would get a frame difference of 0.9 from clip 0's
    # rows and become the largest inferred onsets of the job; clip 1's own rise (rows 4, 5) is smaller.  The clips' maxima differ.
    lens_b = (6, 9, 4)
    n2, o2, c2 = base(sum(lens_b))
    n2[6:15, 33] = 0.9
    n2[10:15, 60] = 0.4
    o2[2, 5], o2[10, 60], o2[17, 70] = 0.9, 0.55, 0.6
    o2[5, 44] = 0.8  # clip 0's last row again: a peak only for a scan that takes clip 1's first row as its neighbour
    n2[3:6, 5] = 0.5
    return (lens_a, n, o, c), (lens_b, n2, o2, c2)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("infer", [1, 0])
def test_no_scan_sees_across_a_clip_boundary(ab, nat, which, infer):
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    lens, note, onset, contour = _boundary_sets()[which]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(offs[-1])
    h = C.c_void_p()
    assert ab.bp_create(blob, len(blob), 0, 0, 8, C.byref(h)) == 0, ab.bp_last_error(None)
    try:
        prm = _prm(nat, ab)
        prm.infer_onsets = infer
        got_note, got_bits, got_bend = np.full((T, 88), -7, np.float32), np.full((T, 12), 0xAA, np.uint8), np.full((T, 88), 99, np.int8)
        status = np.full(len(lens), -1, np.int32)
        rc = ab.bp_ab_clips_candidates_from_maps(h, len(lens), offs.ctypes.data_as(C.POINTER(C.c_int64)), note.ctypes.data,
                                                 onset.ctypes.data, contour.ctypes.data, C.addressof(prm), got_note.ctypes.data,
                                                 got_bits.ctypes.data, got_bend.ctypes.data, status.ctypes.data)
        assert rc == 0, ab.bp_last_error(h)
        assert not status.any()
        marked = 0
        for i in range(len(lens)):
            r0, r1 = int(offs[i]), int(offs[i + 1])
            if r1 == r0:
                continue
            out = {"note": note[r0:r1], "onset": onset[r0:r1], "contour": contour[r0:r1]}
            ref_note, ref_bits, ref_bend = NO.note_candidates(out, prm.onset_threshold, bool(infer), None, None, True)
            assert got_note[r0:r1].tobytes() == ref_note.tobytes(), i
            assert np.array_equal(got_bits[r0:r1], ref_bits), (i, np.argwhere(got_bits[r0:r1] != ref_bits))
            assert np.array_equal(got_bend[r0:r1], ref_bend), i
            marked += int(np.unpackbits(ref_bits).sum())
        assert marked >= 2  # the comparison is not one of empty bitmaps
        whole = NO.note_candidates({"note": note, "onset": onset, "contour": contour}, prm.onset_threshold, bool(infer), None, None, True)[1]
        assert not np.array_equal(whole, got_bits)  # ... and a scan over the whole buffer gives another answer
        if which == 0:
            bit = lambda t, f: (got_bits[t, f >> 3] >> (f & 7)) & 1  # noqa: E731
            assert not bit(6, 10) and not bit(6, 11) and not bit(7, 10) and not bit(7, 11) and not bit(13, 20)
    finally:
        ab.bp_destroy(h)


def test_a_nan_in_one_clip_changes_no_other_clip(model, nat, ab):
    """A NaN sample in the PCM: the clip's status and bytes are whatever the single-clip call gives for it (measured: the CQT's
    maxima drop the NaN, the maps stay finite and the status is 0), every other clip as in a run without it.  The NaN record
    itself — status 1, a zero bitmap, no other clip touched — is reached with a NaN in a clip's MAPS, through the A/B
    library's hook."""
    from basic_pitch_amd import clips as CL

    rng = np.random.default_rng(5)
    lens = (300, 700, 36164 + 500, 255, 9000, 400)  # rows that are no multiple of the bend kernel's 16: blocks straddle clips
    clean = [CL.as_clip(_signal(rng, n, 22050).astype(np.float32), i) for i, n in enumerate(lens)]
    bad = [a.copy() for a in clean]
    bad[2][20000, 0] = np.nan
    prm = _prm(nat, model._lib, limits=True)
    offs0, note0, bits0, bend0, status0 = _batched(model, nat, clean, 22050, prm)
    offs, note, bits, bend, status = _compare_with_single(model, nat, bad, 22050, prm)  # status and bytes of every clip
    assert np.array_equal(offs, offs0) and not status0.any()
    for i in (0, 1, 3, 4, 5):
        a, b = int(offs[i]), int(offs[i + 1])
        assert status[i] == 0
        assert note[a:b].tobytes() == note0[a:b].tobytes() and bits[a:b].tobytes() == bits0[a:b].tobytes(), i
        assert bend[a:b].tobytes() == bend0[a:b].tobytes(), i

    # a NaN in the maps of one clip of three
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    lens, note, onset, contour = _boundary_sets()[1]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(offs[-1])
    h = C.c_void_p()
    assert ab.bp_create(blob, len(blob), 0, 0, 8, C.byref(h)) == 0, ab.bp_last_error(None)
    try:
        prm = _prm(nat, ab)

        def run(n, o, c):
            out = np.full((T, 88), -7, np.float32), np.full((T, 12), 0xAA, np.uint8), np.full((T, 88), 99, np.int8)
            status = np.full(len(lens), -1, np.int32)
            rc = ab.bp_ab_clips_candidates_from_maps(h, len(lens), offs.ctypes.data_as(C.POINTER(C.c_int64)), n.ctypes.data,
                                                     o.ctypes.data, c.ctypes.data, C.addressof(prm), *[x.ctypes.data for x in out],
                                                     status.ctypes.data)
            assert rc == 0, ab.bp_last_error(h)
            return out, status.tolist()

        want, st = run(note, onset, contour)
        assert st == [0, 0, 0]
        for which_map, row in ((0, 8), (1, 6), (1, 14), (2, 9)):  # note, onset (the clip's first and last row), contour
            maps = [note.copy(), onset.copy(), contour.copy()]
            maps[which_map][row, 33] = np.nan
            got, st = run(*maps)
            assert st == ([0, 1, 0] if which_map < 2 else [0, 0, 0]), (which_map, row)  # a contour NaN is no reason to hand over
            for i in (0, 2):
                r0, r1 = int(offs[i]), int(offs[i + 1])
                for g, w in zip(got, want):
                    assert g[r0:r1].tobytes() == w[r0:r1].tobytes(), (which_map, row, i)
            r0, r1 = int(offs[1]), int(offs[2])
            if which_map < 2:
                assert not got[1][r0:r1].any()  # a clip the caller decodes itself gets a zero bitmap
            else:
                assert got[1][r0:r1].tobytes() == want[1][r0:r1].tobytes()
                rest = np.ones((r1 - r0, 88), bool)
                rest[row - r0] = False  # bends are row-local: only the row with the NaN may differ
                assert np.array_equal(got[2][r0:r1][rest], want[2][r0:r1][rest])
            again, st = run(note, onset, contour)  # the records the NaN marked were left initialised
            assert st == [0, 0, 0] and all(g.tobytes() == w.tobytes() for g, w in zip(again, want))
    finally:
        ab.bp_destroy(h)


def _same_events(got, want, where):
    assert len(got) == len(want), where
    for g, w in zip(got, want):
        assert (g[0], g[1], g[2], g[4]) == (w[0], w[1], w[2], w[4]), where
        assert np.float32(g[3]).tobytes() == np.float32(w[3]).tobytes(), where


def _alone(m, clip, rate, **kw):
    from basic_pitch_amd import clips as CL
    from basic_pitch_amd import inference as I

    a = CL.as_clip(clip, 0)
    out = m.predict_pcm_raw(a, CL.FORMATS[a.dtype], a.shape[0], a.shape[1], rate)
    return I._output_to_notes(out, kw.get("onset_threshold", 0.5), kw.get("frame_threshold", 0.3), 127.70, kw.get("minimum_frequency"),
                              kw.get("maximum_frequency"), False, True, 120)


def test_transcribe_clips_returns_the_events_of_predict_per_clip(model, job):
    clips, rates = job
    n_events = 0
    for kw in ({}, {"minimum_frequency": 100.0, "maximum_frequency": 1500.0, "onset_threshold": 0.3}):
        res = model.transcribe_clips(clips, rates, **kw)
        assert len(res) == len(clips)
        for i, (clip, rate) in enumerate(zip(clips, rates)):
            midi, events = res[i]
            _same_events(events, _alone(model, clip, rate, **kw)[1], i)
            assert sum(len(inst.notes) for inst in midi.instruments) == len(events)
            n_events += len(events)
    assert n_events >= 20  # the clips hold notes
    assert model.transcribe_clips([], 44100) == []
    # broken input (a NaN) and an onset threshold of 0 take the host's decoder and still give predict's events
    x = clips[rates.index(22050)].copy()
    long = [c for c, r in zip(clips, rates) if r == 22050 and len(c) > 30000][0].copy()
    long[100] = np.nan
    for kw in ({}, {"onset_threshold": 0.0}):
        res = model.transcribe_clips([long, x, clips[0]], [22050, 22050, rates[0]], **kw)
        for r, (c, rate) in zip(res, ((long, 22050), (x, 22050), (clips[0], rates[0]))):
            _same_events(r[1], _alone(model, c, rate, **kw)[1], kw)


def test_the_call_leaves_the_handle_fit_for_every_other_call(model, nat, job):
    from basic_pitch_amd import clips as CL
    from basic_pitch_amd.inference import Model

    rng = np.random.default_rng(9)
    clips, rates = job
    a441 = [c for c, r in zip(clips, rates) if r == 44100][:8] + [c for c, r in zip(clips, rates) if r == 44100 and len(c) > 60000][:2]
    c48 = [np.clip(np.round(_signal(rng, n, 48000) * 32767), -32768, 32767).astype(np.int16) for n in (700, 48000, 90000)]
    song = np.stack([_signal(rng, 100000, 44100)] * 2, axis=1).astype(np.float32)
    song48 = _signal(rng, 60000, 48000).astype(np.float32)
    with Model(device=0, max_windows=8) as fresh:  # each alone
        want_clips = fresh.transcribe_clips(a441, 44100)
    with Model(device=0, max_windows=8) as fresh:
        want_48 = fresh.transcribe_clips(c48, 48000)
    with Model(device=0, max_windows=8) as fresh:
        want_song, want_song48 = fresh.predict_pcm(song, 44100), fresh.predict_pcm(song48, 48000)
    with Model(device=0, max_windows=8) as fresh, fresh.open_stream(44100, 2) as s:
        want_rows = [s.push(song[:60000]), s.push(song[60000:]), s.finish()]

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _same_events(g[1], w[1], "interleaved")

    with model.open_stream(44100, 2) as s:
        rows = [s.push(song[:60000])]
        same(model.transcribe_clips(a441, 44100), want_clips)
        got48 = model.predict_pcm(song48, 48000)  # replaces the cached 44.1 kHz filter
        same(model.transcribe_clips(a441, 44100), want_clips)  # ... which the call brings back
        same(model.transcribe_clips(c48, 48000), want_48)  # a second rate
        got_song = model.predict_pcm(song, 44100)  # the one-shot path on the filter the batched call cached
        rows.append(s.push(song[60000:]))
        same(model.transcribe_clips(a441 + c48, [44100] * len(a441) + [48000] * 3), want_clips + want_48)
        rows.append(s.finish())
    for k in ("note", "onset", "contour"):
        assert got_song[k].tobytes() == want_song[k].tobytes() and got48[k].tobytes() == want_song48[k].tobytes(), k
        for g, w in zip(rows, want_rows):
            assert g[k].tobytes() == w[k].tobytes(), k
    # the maps of a job of clips do not stay for bp_track_maps; those of a single track still do
    prm = _prm(nat, model._lib)
    one = CL.as_clip([c for c in a441 if len(c) > 60000][0], 0)
    T = _single(model, nat, one, 44100, prm)[0].shape[0]
    maps = [np.empty((T, w), np.float32) for w in (88, 88, 264)]
    assert T > 0 and model._lib.bp_track_maps(model._handle, T, *[a.ctypes.data for a in maps], nat.BP_MEM_HOST) == 0
    offs = _batched(model, nat, [one], 44100, prm)[0]
    assert int(offs[-1]) == T
    assert model._lib.bp_track_maps(model._handle, T, *[a.ctypes.data for a in maps], nat.BP_MEM_HOST) == nat.BP_ERR_INVALID_ARG
    # a ratio whose filter the one-shot path evaluates in the kernel is refused, and nothing of the handle changes
    with pytest.raises(ValueError, match="BP_ERR_UNSUPPORTED"):
        model.transcribe_clips([np.zeros(50000, np.float32)], 44101)
    same(model.transcribe_clips(a441, 44100), want_clips)
