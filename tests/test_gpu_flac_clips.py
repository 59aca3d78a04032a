"""A job of FLAC clips decoded on the device in one call (include/basic_pitch_amd_flac_clips.h; csrc/flac_clips.hip): clip by
clip the host decoder's integers, the rows of bp_infer_flac_candidates on the clip alone and the events
bp_notes_decode_candidates makes of them — for any order of the clips, with a corrupt clip or one left to the host in the
middle — and Model.transcribe_flac_clips against transcribe_clips on the host decoder's arrays."""
import ctypes as C

import numpy as np
import pytest

import flac_streams as FS
import flac_writer as FW

pytestmark = pytest.mark.gpu

RATE = 22050
PITCHES = (48, 52, 55, 60, 64, 67, 72, 57, 62, 65)


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import flac_clips
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        flac_clips.bind(m._lib)
        m._lib.bp_infer_flac_candidates.restype = C.c_int
        m._lib.bp_infer_flac_candidates.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_int)]
        yield m


def _chord(n, ch, bits, seed, rate=RATE, noise=None):
    """Three steady tones (a chord of PITCHES, another per seed) at 0.2 of full scale each plus a little noise, per channel."""
    rng = np.random.default_rng(seed)
    full = (1 << (bits - 1)) - 1
    t = np.arange(n)[:, None] / rate
    x = sum(np.sin(2 * np.pi * 440.0 * 2 ** ((PITCHES[(seed + 3 * k) % len(PITCHES)] - 69) / 12) * t + 0.3 * np.arange(ch)) for k in range(3))
    lim = max(1, full // 256) if noise is None else noise
    return np.clip(0.2 * full * x + rng.integers(-lim, lim + 1, (n, ch)), -full, full).astype(np.int64)


# (what, frames, channels, bits, encoder arguments): neighbours differ in bits AND channels
MATRIX = (
    ("mono 16, 1152", 15000, 1, 16, dict(blocksize=1152)),
    ("stereo 24, 4096", 16000, 2, 24, dict(blocksize=4096)),
    ("mono 8, 192", 5000, 1, 8, dict(blocksize=192)),
    ("stereo 16, 576", 15000, 2, 16, dict(blocksize=576)),
    ("mono 24, 1152", 14000, 1, 24, dict(blocksize=1152)),
    ("stereo 8, 576", 6000, 2, 8, dict(blocksize=576)),
    ("mono 16, one frame", 4096, 1, 16, dict(blocksize=4096)),
    ("stereo 16, variable", 15000, 2, 16, dict(sizes=[1152, 576, 2304])),
    ("mono 24, 192", 5000, 1, 24, dict(blocksize=192)),
    ("stereo 16, short last block", 1152 * 9 + 77, 2, 16, dict(blocksize=1152)),
    ("mono 16, no rows", 100, 1, 16, dict(blocksize=192)),
    ("stereo 16, two scan chunks", 45000, 2, 16, dict(blocksize=4096)),
    ("mono 16, 4096", 14000, 1, 16, dict(blocksize=4096)),
    ("stereo 24, 576", 12000, 2, 24, dict(blocksize=576)),
)


def _layout(lib, blob):
    from basic_pitch_amd import _native

    lay = _native.bp_flac_stream_layout()
    assert lib.bp_flac_layout(bytes(blob), len(blob), C.byref(lay)) == _native.BP_OK
    return lay


def _host_ints(lib, blob):
    """bp_flac_decode's samples as the integers they are made of."""
    from basic_pitch_amd import flac_clips

    pcm, _ = flac_clips.host_decode(lib, blob)
    bits = _layout(lib, blob).bits_per_sample
    return np.round(pcm.astype(np.float64) * (1 << (bits - 1))).astype(np.int32)


def _prm(**kw):
    from basic_pitch_amd import note_creation as NC

    return NC._note_params(0.5, 0.3, 11, True, None, None, True, NC.ENERGY_TOLERANCE, True)


def _records(events, bends, lo, hi):
    return [(e.start_frame, e.end_frame, e.pitch_midi, np.float32(e.amplitude).tobytes(), float(e.start_s), float(e.end_s),
             e.n_bends, e.reserved, tuple(bends[e.bend_offset : e.bend_offset + e.n_bends].tolist())) for e in events[lo:hi]]


def _alone(m, blob, prm):
    """bp_infer_flac_candidates on one clip: (note, bits, bends, status, records of bp_notes_decode_candidates on them)."""
    from basic_pitch_amd import note_creation as NC

    lay = _layout(m._lib, blob)
    T = m._pcm_frames(lay.n_frames, lay.sample_rate)
    note, bits, bend = np.zeros((T, 88), np.float32), np.zeros((T, 12), np.uint8), np.zeros((T, 88), np.int8)
    status = C.c_int(-1)
    rc = m._lib.bp_infer_flac_candidates(m._handle, bytes(blob), len(blob), C.addressof(prm), note.ctypes.data, bits.ctypes.data,
                                         bend.ctypes.data, C.byref(status))
    assert rc == 0, m._lib.bp_last_error(m._handle)
    recs = []
    if T and status.value == 0:
        events, bends, n = NC._grow_and_call(m._lib.bp_notes_decode_candidates,
                                             (note.ctypes.data, bits.ctypes.data, bend.ctypes.data, T, C.byref(prm)), T,
                                             "bp_notes_decode_candidates")
        recs = _records(events, bends, 0, n)
    return note, bits, bend, status.value, recs


@pytest.fixture(scope="module")
def job(model):
    """The clips of MATRIX, built once: blobs, the host decoder's integers, and each clip through the single-file calls."""
    lib = model._lib
    blobs = [FW.encode(_chord(n, ch, bits, i, noise=300 if n == 45000 else None), RATE, bits, **kw)
             for i, (_, n, ch, bits, kw) in enumerate(MATRIX)]
    lays = [_layout(lib, b) for b in blobs]
    # the shapes the batched kernels can go wrong at are really there
    n_frames = [sum(1 for _ in range(0, l.n_frames, l.max_block)) if l.min_block == l.max_block else None for l in lays]
    assert n_frames[6] == 1 and lays[9].n_frames % lays[9].max_block and (lays[7].min_block, lays[7].max_block) == (576, 2304)
    assert sum(f or 7 for f in n_frames) > 64  # more FLAC frames than one decode wave holds
    slots = [(l.n_frames + l.min_block - 1) // l.min_block + 1 for l in lays]
    assert slots[0] + slots[1] + slots[2] < 64  # the first wave serves frames of three streams ...
    assert all((a.bits_per_sample != b.bits_per_sample or a.channels != b.channels) for a, b in zip(lays, lays[1:]))
    assert sum(a.bits_per_sample != b.bits_per_sample and a.channels != b.channels for a, b in zip(lays, lays[1:])) >= 8  # ... of other bits and channels
    assert {l.bits_per_sample for l in lays} == {8, 16, 24} and {l.channels for l in lays} == {1, 2}
    assert {l.max_block for l in lays} >= {192, 576, 1152, 4096}
    big = len(blobs[11]) - lays[11].audio_start
    assert big > 65536 + 4096, big  # a second scan chunk, and (below) a frame across the boundary
    starts = [p for p in range(lays[11].audio_start, len(blobs[11]) - 6) if blobs[11][p] == 0xFF and FS.header_at(blobs[11], p, 16, 2, 4096)]
    edge = lays[11].audio_start + 65536
    assert len(starts) >= 11 and edge not in starts and min(starts) < edge < max(starts)
    prm = _prm()
    return dict(blobs=blobs, lays=lays, ints=[_host_ints(lib, b) for b in blobs], prm=prm, alone=[_alone(model, b, prm) for b in blobs])


def _candidates(m, blobs, prm):
    from basic_pitch_amd import flac_clips

    return flac_clips.infer_flac_clips_candidates(m, blobs, RATE, prm)


def _events(m, blobs, prm):
    from basic_pitch_amd import flac_clips

    events, bends, offs, status = flac_clips.infer_flac_clips_events(m, blobs, RATE, prm)
    assert offs[0] == 0 and (np.diff(offs) >= 0).all()
    all_ev = events[: int(offs[-1])]
    assert [e.bend_offset for e in all_ev] == np.concatenate([[0], np.cumsum([e.n_bends for e in all_ev])])[:-1].astype(int).tolist()
    return [_records(events, bends, int(offs[i]), int(offs[i + 1])) for i in range(len(blobs))], status.tolist()


def test_decode_matrix_in_one_call_and_in_reverse(model, job):
    from basic_pitch_amd import flac_clips

    got, status = flac_clips.decode_device(model, job["blobs"])
    assert status.tolist() == [0] * len(MATRIX)
    for (what, *_), g, w in zip(MATRIX, got, job["ints"]):
        assert g.shape == w.shape and np.array_equal(g, w), what
    rev, status = flac_clips.decode_device(model, job["blobs"][::-1])
    assert status.tolist() == [0] * len(MATRIX)
    for (what, *_), g, w in zip(MATRIX, rev[::-1], got):
        assert g.tobytes() == w.tobytes(), what
    none, status = flac_clips.decode_device(model, [])  # an empty job
    assert none == [] and status.tolist() == []


def _planted_tail(seed, number):
    """Mono 16-bit verbatim frames (the samples ARE the bytes) whose LAST samples spell a CRC-8-valid frame header: the clip's
    last bytes are that header and the frame's CRC-16."""
    rng = np.random.default_rng(seed)
    n = 256 * 6
    pcm = (9000 + 6000 * np.sin(np.arange(n) * 0.05) + rng.integers(0, 2000, n)).astype(np.int64)[:, None]
    pcm[::256] |= 1  # no wasted bits
    h = FS.fake_header(number, bs_code=8, sr_code=0)
    pcm[n - len(h) // 2 :, 0] = np.frombuffer(h, ">i2")
    data = FW.encode(pcm, RATE, 16, blocksize=256, plan=lambda fi: dict(kind="verbatim"))
    assert data[-2 - len(h) : -2] == h and FS.header_at(data, len(data) - 2 - len(h), 16, 1, 256)[:3] == (False, number, 256)
    return data, pcm


def test_a_header_in_a_clips_last_bytes_is_no_frame_of_the_next_clip(model):
    from basic_pitch_amd import flac_clips

    # the planted number is the one the NEXT clip's first frame would be continued by (frame 0 -> 1); the next clip is of the
    # same stream parameters, so the header would pass its scan
    first, pcm_a = _planted_tail(1, 1)
    second, pcm_b = _planted_tail(2, 1)
    got, status = flac_clips.decode_device(model, [first, second, first])
    assert status.tolist() == [0, 0, 0]
    for g, w in zip(got, (pcm_a, pcm_b, pcm_a)):
        assert np.array_equal(g, w) and np.array_equal(g, _host_ints(model._lib, first if w is pcm_a else second))


def test_candidates_are_the_single_file_calls_rows(model, job):
    offs, note, bits, bend, status = _candidates(model, job["blobs"], job["prm"])
    windows = sum(int(model._lib.bp_handle_track_n_windows(model._handle, l.n_frames)) for l in job["lays"])
    assert windows > 8  # more windows than a batch holds: they pack across clips and batches
    assert status.tolist() == [a[3] for a in job["alone"]] == [0] * len(MATRIX)
    for i, (what, *_) in enumerate(MATRIX):
        r0, r1 = int(offs[i]), int(offs[i + 1])
        a = job["alone"][i]
        assert r1 - r0 == a[0].shape[0], what
        assert note[r0:r1].tobytes() == a[0].tobytes() and bits[r0:r1].tobytes() == a[1].tobytes() and bend[r0:r1].tobytes() == a[2].tobytes(), what
    assert offs[11] == offs[10] and offs[-1] > 0  # the clip of 100 frames has no rows
    # the handle's state afterwards is that of bp_infer_clips_candidates: no maps left for bp_track_maps
    z = np.zeros((int(offs[-1]), 440), np.float32)
    assert model._lib.bp_track_maps(model._handle, int(offs[-1]), z.ctypes.data, z.ctypes.data, z.ctypes.data, 0) != 0


def test_events_are_those_of_the_single_file_rows(model, job):
    got, status = _events(model, job["blobs"], job["prm"])
    assert status == [0] * len(MATRIX)
    n_events = sum(len(a[4]) for a in job["alone"])
    print("events of the single-clip route:", [len(a[4]) for a in job["alone"]])
    assert n_events >= 20  # the comparison is not one of empty lists
    for i, (what, *_) in enumerate(MATRIX):
        assert got[i] == job["alone"][i][4], what


def _flip_in_first_payload(lib, blob):
    lay = _layout(lib, blob)
    hdr = FS.header_at(blob, lay.audio_start, lay.bits_per_sample, lay.channels, lay.max_block)
    at = lay.audio_start + hdr[3] + 20
    return blob[:at] + bytes([blob[at] ^ 0x40]) + blob[at + 1 :]


def test_one_bad_clip_in_the_middle_changes_no_other_clip(model, job):
    from basic_pitch_amd import _native, flac_clips

    lib, prm, blobs = model._lib, job["prm"], list(job["blobs"])
    k = 3
    clean_c = _candidates(model, blobs, prm)
    clean_e, _ = _events(model, blobs, prm)
    assert len(clean_e[k]) > 0  # the clip that goes bad holds events
    bad = _flip_in_first_payload(lib, blobs[k])
    with pytest.raises(ValueError):  # ordinary data the decoders are built to reject
        flac_clips.host_decode(lib, bad)
    nototal = FW.encode(_chord(12000, 2, 16, 90), RATE, 16, blocksize=1152, total_in_header=False)
    wide = FW.encode(_chord(20000, 2, 16, 91), RATE, 16, sizes=[16, 4608])
    wlay = _layout(lib, wide)
    assert (wlay.min_block, wlay.max_block) == (16, 4608)
    for what, clip, want in (("a flipped byte", bad, _native.BP_CLIP_FLAC_FAILED), ("no sample count", nototal, _native.BP_CLIP_FLAC_HOST),
                             ("block sizes 16 and 4608", wide, _native.BP_CLIP_FLAC_HOST)):
        mixed = blobs[:k] + [clip] + blobs[k + 1 :]
        offs, note, bits, bend, status = _candidates(model, mixed, prm)
        assert status.tolist() == [0] * k + [want] + [0] * (len(blobs) - k - 1), what
        rows_k = int(offs[k + 1] - offs[k])
        # rows from STREAMINFO for the failed clip; none, and so no device work, for a clip left to the host
        assert rows_k == (clean_c[0][k + 1] - clean_c[0][k] if want == _native.BP_CLIP_FLAC_FAILED else 0), what
        got_e, status_e = _events(model, mixed, prm)
        assert status_e == status.tolist() and got_e[k] == [], what
        for i in range(len(blobs)):
            if i == k:
                continue
            r0, r1, c0, c1 = int(offs[i]), int(offs[i + 1]), int(clean_c[0][i]), int(clean_c[0][i + 1])
            assert r1 - r0 == c1 - c0, (what, i)
            for g, w in zip((note, bits, bend), clean_c[1:4]):
                assert g[r0:r1].tobytes() == w[c0:c1].tobytes(), (what, i)
            assert got_e[i] == clean_e[i], (what, i)
        ints, dstatus = flac_clips.decode_device(model, mixed)
        assert dstatus.tolist() == status.tolist() and ints[k] is None, what
        assert all(np.array_equal(ints[i], job["ints"][i]) for i in range(len(blobs)) if i != k), what


def test_refusals_queue_nothing_and_the_next_call_is_right(model, job):
    from basic_pitch_amd import _native, flac_clips

    lib, h, prm = model._lib, model._handle, job["prm"]
    err = lambda: lib.bp_last_error(h).decode()  # noqa: E731
    blobs = job["blobs"][:4]
    other = FW.encode(_chord(6000, 1, 16, 5, rate=44100), 44100, 16, blocksize=1152)
    mixed = blobs[:2] + [other] + blobs[2:]
    for call in (_candidates, _events):
        with pytest.raises(ValueError, match=r"clip 2: .*44100 Hz"):
            call(model, mixed, prm)
    offs, note, bits, bend, status = _candidates(model, blobs, prm)  # the next valid call
    for i in range(4):
        a = job["alone"][i]
        r0, r1 = int(offs[i]), int(offs[i + 1])
        assert status[i] == 0 and note[r0:r1].tobytes() == a[0].tobytes() and bits[r0:r1].tobytes() == a[1].tobytes() and bend[r0:r1].tobytes() == a[2].tobytes()
    tab, keep = flac_clips.clip_table(blobs)
    st = np.zeros(4, np.int32)
    o = np.zeros(5, np.int64)
    p64 = o.ctypes.data_as(C.POINTER(C.c_int64))
    T = int(offs[-1])
    bad = _native.BP_ERR_INVALID_ARG
    assert lib.bp_flac_clips_row_offsets(h, 4, None, RATE, p64, st.ctypes.data) == bad and "null clips" in err()
    assert lib.bp_flac_clips_row_offsets(h, 4, tab, RATE, p64, None) == bad
    assert lib.bp_flac_clips_row_offsets(h, 4, tab, RATE, None, st.ctypes.data) == bad
    assert lib.bp_infer_flac_clips_candidates(h, 4, None, RATE, C.addressof(prm), note.ctypes.data, bits.ctypes.data, bend.ctypes.data, st.ctypes.data) == bad
    assert lib.bp_infer_flac_clips_candidates(h, 4, tab, RATE, C.addressof(prm), note.ctypes.data, bits.ctypes.data, bend.ctypes.data, None) == bad
    assert lib.bp_infer_flac_clips_candidates(h, 4, tab, RATE, C.addressof(prm), None, bits.ctypes.data, bend.ctypes.data, st.ctypes.data) == bad and T > 0
    assert lib.bp_infer_flac_clips_candidates(h, 4, tab, RATE, C.addressof(prm), note.ctypes.data, None, bend.ctypes.data, st.ctypes.data) == bad
    assert lib.bp_infer_flac_clips_candidates(h, 4, tab, RATE, None, note.ctypes.data, bits.ctypes.data, bend.ctypes.data, st.ctypes.data) == bad
    ev = (_native.bp_note_event * 4096)()
    bd = np.zeros(1 << 18, np.int32)
    assert lib.bp_infer_flac_clips_events(h, 4, None, RATE, C.addressof(prm), C.addressof(ev), 4096, bd.ctypes.data, bd.size, p64, st.ctypes.data) == bad
    assert lib.bp_infer_flac_clips_events(h, 4, tab, RATE, C.addressof(prm), C.addressof(ev), 4096, bd.ctypes.data, bd.size, p64, None) == bad
    assert lib.bp_infer_flac_clips_events(h, 4, tab, RATE, C.addressof(prm), None, 4096, bd.ctypes.data, bd.size, p64, st.ctypes.data) == bad
    assert lib.bp_infer_flac_clips_events(h, 4, tab, RATE, C.addressof(prm), C.addressof(ev), 4096, bd.ctypes.data, bd.size, None, st.ctypes.data) == bad
    pcm = np.zeros(1 << 18, np.int32)
    assert lib.bp_flac_clips_decode_device(h, 4, tab, None, p64, st.ctypes.data) == bad and "clip 0" in err()
    assert lib.bp_flac_clips_decode_device(h, 4, tab, pcm.ctypes.data, None, st.ctypes.data) == bad
    # an empty job is fine and writes offsets[0] = 0
    o[:] = -1
    assert lib.bp_flac_clips_row_offsets(h, 0, None, RATE, p64, None) == 0 and o[0] == 0
    o[:] = -1
    assert lib.bp_infer_flac_clips_events(h, 0, None, RATE, C.addressof(prm), None, 0, None, 0, p64, None) == 0 and o[0] == 0
    assert lib.bp_infer_flac_clips_candidates(h, 0, None, RATE, C.addressof(prm), None, None, None, None) == 0
    # and the call after all of that still gives the right bytes
    got, status = _events(model, blobs, prm)
    assert status == [0] * 4 and all(got[i] == job["alone"][i][4] for i in range(4))


def _same_events(got, want, where):
    assert len(got) == len(want), where
    for g, w in zip(got, want):
        assert (g[0], g[1], g[2], g[4]) == (w[0], w[1], w[2], w[4]), where
        assert np.float32(g[3]).tobytes() == np.float32(w[3]).tobytes(), where


def test_transcribe_flac_clips_is_transcribe_clips_on_the_host_decoders_arrays(model, job):
    from basic_pitch_amd import flac_clips

    lib = model._lib
    mixed = [FW.encode(_chord(n, ch, bits, 20 + i, rate=rate), rate, bits, blocksize=bs)
             for i, (n, ch, bits, rate, bs) in enumerate(((14000, 2, 16, 22050, 1152), (26000, 1, 16, 44100, 4096), (27000, 2, 24, 48000, 1152),
                                                         (13000, 1, 8, 22050, 576), (24000, 2, 16, 44100, 1152)))]
    bad = _flip_in_first_payload(lib, job["blobs"][3])
    nototal = FW.encode(_chord(12000, 2, 16, 90), RATE, 16, blocksize=1152, total_in_header=False)
    blobs = mixed[:2] + [nototal] + mixed[2:] + [bad, b"RIFF" + bytes(100)]
    decodable = [i for i in range(len(blobs)) if i < len(blobs) - 2]
    host = {i: flac_clips.host_decode(lib, blobs[i]) for i in decodable}
    n_events = 0
    for decode in ("host", "device"):
        want = model.transcribe_clips([host[i][0] for i in decodable], [host[i][1] for i in decodable], decode=decode)
        with pytest.raises(ValueError, match=rf"clip {len(blobs) - 2}: "):
            model.transcribe_flac_clips(blobs, decode=decode)
        got = model.transcribe_flac_clips(blobs, decode=decode, errors="return")
        assert len(got) == len(blobs)
        for i, w in zip(decodable, want):
            _same_events(got[i][1], w[1], (decode, i))
            assert got[i][0].to_bytes() == w[0].to_bytes(), (decode, i)
            n_events += len(w[1])
        assert isinstance(got[-2], ValueError) and f"clip {len(blobs) - 2}: " in str(got[-2])  # corrupt: the host decoder names the fault
        assert isinstance(got[-1], ValueError) and f"clip {len(blobs) - 1}: " in str(got[-1])  # not FLAC at all
    assert n_events >= 10
    assert model.transcribe_flac_clips([]) == []
