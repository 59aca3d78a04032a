"""Note events decoded on the device for a job of clips (bp_infer_clips_events / bp_note_events_from_maps,
include/basic_pitch_amd_events.h; csrc/note_track.hip): clip by clip the bytes of the host path — bp_note_candidates or
bp_infer_clips_candidates, then bp_notes_decode_candidates — frames, pitch, the float32 amplitude's bit pattern, times as
float64, bend lists, event order and counts."""
import ctypes as C

import numpy as np
import pytest

import note_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _prm(args):
    from basic_pitch_amd import note_creation as NC

    return NC._note_params(args.get("onset_thresh", 0.5), args.get("frame_thresh", 0.3), args.get("min_note_len", 11),
                           args.get("infer_onsets", True), args.get("max_freq"), args.get("min_freq"),
                           args.get("melodia_trick", True), args.get("energy_tol", NC.ENERGY_TOLERANCE),
                           args.get("include_pitch_bends", True))


def _records(events, bends, lo, hi, with_bends):
    """bp_note_event records lo ... hi - 1 as comparable tuples: frames, pitch, the amplitude's bits, times, bends."""
    return [(e.start_frame, e.end_frame, e.pitch_midi, np.float32(e.amplitude).tobytes(), float(e.start_s), float(e.end_s),
             e.n_bends, e.reserved, tuple(bends[e.bend_offset : e.bend_offset + e.n_bends].tolist()) if with_bends else None)
            for e in events[lo:hi]]


def _host(m, out, prm):
    """The host path on one clip's maps alone: (records, status of bp_note_candidates)."""
    from basic_pitch_amd import note_creation as NC

    note, bits, bend, status = m.note_candidates(out, prm)
    if status:
        return None, status
    T = note.shape[0]
    maps = (note.ctypes.data, bits.ctypes.data, bend.ctypes.data if bend is not None else None, T)
    events, bends, n = NC._grow_and_call(m._lib.bp_notes_decode_candidates, maps + (C.byref(prm),), T, "bp_notes_decode_candidates")
    return _records(events, bends, 0, n, bool(prm.include_pitch_bends)), 0


def _device(m, outs, prm, room=None):
    """One bp_note_events_from_maps call on the maps of `outs`, one after the other: (records per segment, status)."""
    from basic_pitch_amd import _native, events as EV

    cat = {k: np.ascontiguousarray(np.concatenate([np.asarray(o[k], np.float32).reshape(-1, w) for o in outs]))
           for k, w in (("note", 88), ("onset", 88), ("contour", 264))}
    before = {k: v.copy() for k, v in cat.items()}
    offs = np.concatenate([[0], np.cumsum([o["note"].shape[0] for o in outs])]).astype(np.int64)
    events, bends, ev_offs, status = EV.note_events_from_maps(m, offs, cat["note"].ctypes.data, cat["onset"].ctypes.data,
                                                              cat["contour"].ctypes.data, _native.BP_MEM_HOST, prm, room)
    for k in cat:  # the caller's maps are left alone
        assert np.array_equal(cat[k], before[k], equal_nan=True), k
    assert ev_offs[0] == 0 and (np.diff(ev_offs) >= 0).all()
    pb = bool(prm.include_pitch_bends)
    recs = [_records(events, bends, int(ev_offs[i]), int(ev_offs[i + 1]), pb) for i in range(len(outs))]
    # bend_offset runs through the bends of all clips in event order
    all_ev = events[: int(ev_offs[-1])]
    assert [e.bend_offset for e in all_ev] == np.concatenate([[0], np.cumsum([e.n_bends for e in all_ev])])[:-1].astype(int).tolist()
    return recs, status.tolist()


def _same(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (where, k, g, w)


@pytest.fixture(scope="module")
def cases(model):
    """The 16 fixture cases: (name, maps, own arguments), decoded once by the host with their own parameters."""
    out = []
    for name in note_cases.CASES:
        maps, args = note_cases.case_args(name)
        args = {k: v for k, v in args.items() if k not in ("multiple_pitch_bends", "midi_tempo")}
        out.append((name, maps, args, _host(model, maps, _prm(args))))
    return out


def test_the_fixture_cases_one_per_call(model, cases):
    n_events = 0
    for name, maps, args, (want, want_status) in cases:
        got, status = _device(model, [maps], _prm(args))
        assert status == [want_status], name
        if want_status:
            assert got == [[]], name
            continue
        _same(got[0], want, name)
        n_events += len(want)
    assert n_events >= 100  # the comparison is not one of empty lists


def test_the_fixture_cases_as_one_call_of_16_segments(model, cases):
    # one parameter set per call: the cases go together under the default parameters and, a second time, under another set
    for args in ({}, {"onset_thresh": 0.6, "frame_thresh": 0.25, "min_note_len": 5, "infer_onsets": False, "min_freq": 80.0,
                      "max_freq": 1500.0}):
        prm = _prm(args)
        got, status = _device(model, [c[1] for c in cases], prm)
        assert len(got) == 16
        for i, (name, maps, own, own_host) in enumerate(cases):
            want, want_status = own_host if own == args or (not args and own == note_cases._BASE) else _host(model, maps, prm)
            assert status[i] == want_status, name
            _same(got[i], want or [], name)


# ---- handcrafted maps at the smallest shapes where the tracker can go wrong
H = dict(onset_thresh=0.5, frame_thresh=0.3, min_note_len=3, energy_tol=5, infer_onsets=False)


def _blank(rng, T):
    return {"note": rng.uniform(0, 0.02, (T, 88)).astype(np.float32), "onset": np.zeros((T, 88), np.float32),
            "contour": rng.uniform(0, 1, (T, 264)).astype(np.float32)}


def _put(rng, m, t0, t1, f, peak=True, lo=0.5, hi=0.9):
    """A sustained note of t1 - t0 frames at bin f with an onset peak on its first frame."""
    m["note"][t0:t1, f] = rng.uniform(lo, hi, t1 - t0).astype(np.float32)
    if peak:
        m["onset"][t0, f] = 0.9


def _handcrafted():
    rng = np.random.default_rng(77)
    clips = [_blank(rng, T) for T in (0, 1, 2, 3)]
    clips[2]["onset"][0, 5] = 0.9
    clips[3]["onset"][1, 5] = 0.9  # a peak at T - 2 of the shortest clip that can hold one
    clips[3]["note"][1:3, 5] = 0.8
    a = _blank(rng, 60)  # a peak at T - 2; notes of exactly min_note_len and min_note_len + 1 frames; gaps; bins 0 and 87
    _put(rng, a, 58, 60, 10)
    _put(rng, a, 50, 60, 12)  # runs into the last row
    _put(rng, a, 5, 8, 20)    # min_note_len frames: refused by both phases
    _put(rng, a, 5, 9, 24)    # min_note_len + 1
    _put(rng, a, 20, 30, 30), _put(rng, a, 34, 40, 30, peak=False)  # a gap of energy_tol - 1: bridged
    _put(rng, a, 20, 30, 34), _put(rng, a, 35, 41, 34, peak=False)  # a gap of energy_tol: the note ends, melodia finds the rest
    _put(rng, a, 10, 18, 0), _put(rng, a, 30, 44, 87)
    clips.append(a)
    b = _blank(rng, 64)  # two peaks in one frame at adjacent bins: the upper one's zeroing reaches the lower one
    _put(rng, b, 10, 14, 41), _put(rng, b, 10, 25, 40)   # ... for fewer than energy_tol rows: bridged
    _put(rng, b, 30, 40, 61), _put(rng, b, 30, 45, 60)   # ... for more: the lower one ends at its second row
    _put(rng, b, 30, 40, 70), _put(rng, b, 28, 45, 69)   # the lower one starts earlier: shortened to the upper one's start
    clips.append(b)
    c = _blank(rng, 50)  # melodia only: equal maxima in one row and in two rows, walks that reach row 1 and row T - 2
    for f in (50, 60):
        _put(rng, c, 20, 35, f, peak=False, hi=0.8)
        c["note"][27, f] = 0.95
    _put(rng, c, 5, 15, 70, peak=False, hi=0.8), _put(rng, c, 30, 45, 20, peak=False, hi=0.8)
    c["note"][12, 70] = c["note"][40, 20] = 0.93
    _put(rng, c, 0, 12, 5, peak=False), _put(rng, c, 38, 50, 80, peak=False)
    clips.append(c)
    d = _blank(rng, 142)  # every branch of the pairwise sum, in LDS ...
    for k, n in enumerate((7, 8, 127)):
        _put(rng, d, 3 + k, 3 + k + n, 10 + 4 * k)
    _put(rng, d, 20, 60, 70, peak=False)
    clips.append(d)
    e = _blank(rng, 142)
    for k, n in enumerate((128, 129, 131)):
        _put(rng, e, 2 + k, 2 + k + n, 30 + 4 * k)
    clips.append(e)
    g = _blank(rng, 701)  # ... and in the scratch buffer, with the split levels of 290 frames
    for k, n in enumerate((7, 8, 127, 128, 129, 131, 290)):
        _put(rng, g, 5 + 3 * k, 5 + 3 * k + n, 4 + 6 * k)
    _put(rng, g, 300, 699, 60), _put(rng, g, 350, 700, 80, peak=False)
    _put(rng, g, 640, 700, 87), _put(rng, g, 500, 640, 0, peak=False)
    clips.append(g)
    return clips


def test_handcrafted_maps_in_one_segmented_call(model):
    clips = _handcrafted()
    assert [c["note"].shape[0] for c in clips] == [0, 1, 2, 3, 60, 64, 50, 142, 142, 701]
    for extra in ({}, {"include_pitch_bends": False}, {"melodia_trick": False}):
        args = dict(H, **extra)
        prm = _prm(args)
        got, status = _device(model, clips, prm)
        assert status == [0] * len(clips)
        total = onset_phase = 0
        lengths = set()
        for i, c in enumerate(clips):
            if c["note"].shape[0] == 0:
                assert got[i] == []
                continue
            want, st = _host(model, c, prm)
            assert st == 0
            _same(got[i], want, (extra, i))
            total += len(want)
            onset_phase += len(_host(model, c, _prm(dict(args, melodia_trick=False)))[0])
            lengths |= {w[1] - w[0] for w in want}
        # the comparison is not one of empty lists, and both phases gave events
        assert total >= 10 and onset_phase >= 1
        if args.get("melodia_trick", True):
            assert total - onset_phase >= 1
            assert {7, 8, 127, 128, 129, 131, 290} <= lengths, sorted(lengths)


def _fuzz_maps(rng, T, runs):
    out = {"note": rng.random((T, 88), dtype=np.float32) ** 3, "onset": rng.random((T, 88), dtype=np.float32) ** 4,
           "contour": rng.random((T, 264), dtype=np.float32)}
    if runs:  # note-like structure: runs along time
        out["note"] = np.repeat(out["note"][::7], 7, axis=0)[:T].copy()
    return out


@pytest.mark.parametrize("trial", range(6))
def test_seeded_fuzz_packs_of_8_segments(model, trial):
    rng = np.random.default_rng(500 + trial)
    args = dict(onset_thresh=float(rng.choice([0.2, 0.5, 0.9])), frame_thresh=float(rng.choice([0.1, 0.3])),
                infer_onsets=bool(rng.integers(0, 2)), melodia_trick=bool(trial % 2), min_note_len=int(rng.choice([3, 11])),
                include_pitch_bends=bool((trial // 2) % 2), min_freq=float(rng.choice([0, 100.0])) or None,
                max_freq=float(rng.choice([0, 2000.0])) or None)
    segs = [_fuzz_maps(rng, int(rng.integers(3, 700)), k % 3 == 0) for k in range(8)]
    prm = _prm(args)
    got, status = _device(model, segs, prm)
    n = 0
    for i, s in enumerate(segs):
        want, st = _host(model, s, prm)
        assert status[i] == st == 0, (args, i)
        _same(got[i], want, (args, i))
        n += len(want)
    assert n >= 8


def test_a_nan_or_an_overflow_in_one_clip_changes_no_other_clip(model):
    from basic_pitch_amd import events as EV

    rng = np.random.default_rng(9)
    # frame threshold 0: zeroed cells no longer end a scan, every note runs to the clip's end and notes of one pitch overlap
    args = dict(onset_thresh=0.5, frame_thresh=0.0, min_note_len=0, infer_onsets=False, melodia_trick=False)
    prm = _prm(args)
    clean = []
    for T in (40, 142, 450):
        c = _blank(rng, T)
        for k in range(6):
            _put(rng, c, 3 + 5 * k, 10 + 5 * k, 8 + 9 * k)
        clean.append(c)
    dense = _blank(rng, 64)  # a peak on every other frame of every other bin, each note running to the end of the clip
    dense["note"][:] = 1.0
    dense["onset"][1:62:2, ::2] = 0.9
    want = [_host(model, c, prm)[0] for c in clean]
    for c, w in zip(clean, want):  # the clean clips stay under their capacity
        T = c["note"].shape[0]
        assert 0 < len(w) <= EV.events_capacity(T, 0) and sum(r[6] for r in w) <= EV.bends_capacity(T)
    w_dense = _host(model, dense, prm)[0]
    assert sum(r[6] for r in w_dense) > EV.bends_capacity(64) and len(w_dense) <= EV.events_capacity(64, 0)
    got, status = _device(model, [clean[0], dense, clean[1], clean[2]], prm)
    assert status == [0, 2, 0, 0] and got[1] == []
    for g, w in zip((got[0], got[2], got[3]), want):
        _same(g, w, "beside an overflow")
    # the events' own capacity, under min_note_len 11: 88 * ceil(64 / 12) notes of more than 11 frames
    prm11 = _prm(dict(args, min_note_len=11))
    w11 = _host(model, dense, prm11)[0]
    assert len(w11) > EV.events_capacity(64, 11)
    got, status = _device(model, [dense, clean[1]], prm11)
    assert status == [2, 0] and got[0] == []
    _same(got[1], _host(model, clean[1], prm11)[0], "beside an overflow of events")
    # a NaN in the note rows, in the onset rows: status 1 for that clip alone
    for which in ("note", "onset"):
        bad = {k: v.copy() for k, v in clean[1].items()}
        bad[which][70, 33] = np.nan
        assert _host(model, bad, prm)[1] == 1
        got, status = _device(model, [clean[0], bad, clean[2]], prm)
        assert status == [0, 1, 0] and got[1] == []
        _same(got[0], want[0], which), _same(got[2], want[2], which)
    # an onset threshold <= 0 is status 1 for every clip that has rows
    got, status = _device(model, [clean[0], _blank(rng, 0), clean[1]], _prm(dict(args, onset_thresh=0.0)))
    assert status == [1, 0, 1] and got == [[], [], []]


def test_too_small_buffers_name_the_sizes_and_the_repeated_call_succeeds(model):
    from basic_pitch_amd import _native, events as EV

    rng = np.random.default_rng(3)
    segs = [_fuzz_maps(rng, T, True) for T in (100, 300)]
    prm = _prm(dict(min_note_len=11))
    want = [_host(model, s, prm)[0] for s in segs]
    n_ev, n_b = sum(len(w) for w in want), sum(r[6] for w in want for r in w)
    assert n_ev >= 4 and n_b >= 50
    lib = EV.bind(model._lib)
    cat = {k: np.ascontiguousarray(np.concatenate([s[k] for s in segs])) for k in ("note", "onset", "contour")}
    offs = np.array([0, 100, 400], np.int64)

    def call(max_events, max_bends):
        events = (_native.bp_note_event * max(1, max_events))()
        bends = np.zeros(max(1, max_bends), np.int32)
        ev_offs, status = np.full(3, -1, np.int64), np.full(2, -1, np.int32)
        rc = lib.bp_note_events_from_maps(model._handle, 2, offs.ctypes.data_as(C.POINTER(C.c_int64)), cat["note"].ctypes.data,
                                          cat["onset"].ctypes.data, cat["contour"].ctypes.data, _native.BP_MEM_HOST, C.addressof(prm),
                                          C.addressof(events), max_events, bends.ctypes.data, max_bends,
                                          ev_offs.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data)
        return rc, events, bends, ev_offs, status

    for room in ((n_ev - 1, n_b), (n_ev, n_b - 1), (0, 0)):
        rc, _, _, ev_offs, status = call(*room)
        msg = lib.bp_last_error(model._handle).decode()
        assert rc == _native.BP_ERR_INVALID_ARG and f"{n_ev} events and {n_b} bends" in msg, msg
        assert ev_offs.tolist() == [0, len(want[0]), n_ev] and status.tolist() == [0, 0]
    rc, events, bends, ev_offs, status = call(n_ev, n_b)
    assert rc == 0 and ev_offs.tolist() == [0, len(want[0]), n_ev]
    for i in range(2):
        _same(_records(events, bends, int(ev_offs[i]), int(ev_offs[i + 1]), True), want[i], i)


def test_transcribe_clips_on_the_device_returns_the_hosts_events(model):
    from test_gpu_clips import _make_clips

    clips, rates = _make_clips()
    song = clips[[i for i, c in enumerate(clips) if len(c) > 60000][0]]
    rate = rates[[i for i, c in enumerate(clips) if len(c) > 60000][0]]
    before = model.predict_pcm(np.asarray(song, np.float32).reshape(len(song), -1), rate)
    n_events = 0
    for kw in ({}, {"minimum_frequency": 100.0, "maximum_frequency": 1500.0, "onset_threshold": 0.3}):
        host = model.transcribe_clips(clips, rates, **kw)
        dev = model.transcribe_clips(clips, rates, decode="device", **kw)
        assert len(dev) == len(host) == len(clips)
        for i, ((m_h, e_h), (m_d, e_d)) in enumerate(zip(host, dev)):
            assert len(e_h) == len(e_d), i
            for g, w in zip(e_d, e_h):
                assert (g[0], g[1], g[2], g[4]) == (w[0], w[1], w[2], w[4]), i
                assert np.float32(g[3]).tobytes() == np.float32(w[3]).tobytes(), i
            assert sum(len(inst.notes) for inst in m_d.instruments) == sum(len(inst.notes) for inst in m_h.instruments) == len(e_h)
            n_events += len(e_h)
    assert n_events >= 20  # the clips hold notes
    assert model.transcribe_clips([], 44100, decode="device") == []
    # a NaN and an onset threshold of 0 fall back to the host's decoder, as they do with decode="host"
    x = clips[rates.index(22050)].copy()
    long = [c for c, r in zip(clips, rates) if r == 22050 and len(c) > 30000][0].copy()
    long[100] = np.nan
    for kw in ({}, {"onset_threshold": 0.0}):
        host = model.transcribe_clips([long, x], 22050, **kw)
        dev = model.transcribe_clips([long, x], 22050, decode="device", **kw)
        for (_, e_h), (_, e_d) in zip(host, dev):
            assert [(g[0], g[1], g[2], g[4]) for g in e_d] == [(w[0], w[1], w[2], w[4]) for w in e_h]
    # Model.note_events: posteriorgrams the caller holds, as numpy arrays and as device tensors
    import torch

    outs = [note_cases.case_args("clip_default")[0], note_cases.synthetic(300, 21)]
    prm = _prm({})
    want = [_host(model, o, prm)[0] for o in outs]
    for form in (outs, [{k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for k, v in o.items()} for o in outs]):
        res = model.note_events(form, prm)
        assert [s for _, s in res] == [0, 0]
        for (ev, _), w in zip(res, want):
            assert [(e[2], np.float32(e[3]).tobytes(), e[0], e[1], tuple(e[4])) for e in ev] == [(r[2], r[3], r[4], r[5], r[8]) for r in w]
    # afterwards the handle predicts what it predicted before
    after = model.predict_pcm(np.asarray(song, np.float32).reshape(len(song), -1), rate)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_one_job_gives_the_same_events_by_every_route():
    """What the job driver (csrc/clips_api.hip run_clips) holds in one place: a job of three segments of 142, 0 and 284 rows —
    the smallest with an empty segment between two that have rows, on a handle of two windows so that chunks end inside it — as
    44.1 kHz stereo int16 PCM through bp_infer_clips_candidates and bp_infer_clips_events, and as maps through
    bp_note_events_from_maps from host and from device memory.  A job of clips leaves no maps for bp_track_maps (its rows
    are those of the single-clip call, tests/test_gpu_clips.py), so the maps are fetched with it after
    bp_infer_pcm_raw_candidates on each clip alone."""
    import torch

    from basic_pitch_amd import _native, clips as CL, events as EV, note_creation as NC
    from basic_pitch_amd.inference import Model
    from test_gpu_clips import _signal

    rng = np.random.default_rng(31)
    frames = (2 * 36164, 0, 4 * 36164)  # 36164 and 72328 samples at the model's rate: int(n / 36164 * 142) rows
    arrays = [np.clip(np.round(np.stack([_signal(rng, f, 44100)] * 2, axis=1) * 32767), -32768, 32767).astype(np.int16)
              if f else np.zeros((0, 2), np.int16) for f in frames]
    prm = _prm({})
    with Model(device=0, max_windows=2) as m:
        offs, note, bits, bend, st_cand = CL.infer_clips_candidates(m, arrays, 44100, prm)
        assert offs.tolist() == [0, 142, 142, 426]
        by_pcm = EV.infer_clips_events(m, arrays, 44100, prm)
        maps = {k: np.zeros((426, w), np.float32) for k, w in (("note", 88), ("onset", 88), ("contour", 264))}
        for i, a in enumerate(arrays):
            r0, r1 = int(offs[i]), int(offs[i + 1])
            if r1 == r0:
                continue
            status = C.c_int(-1)
            one = [np.empty((r1 - r0, w), t) for w, t in ((88, np.float32), (12, np.uint8), (88, np.int8))]
            rc = m._lib.bp_infer_pcm_raw_candidates(m._handle, a.ctypes.data, CL.FORMATS[a.dtype], a.shape[0], 2, 44100, C.byref(prm),
                                                    one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, C.byref(status))
            _native.check(m._lib, m._handle, rc, "bp_infer_pcm_raw_candidates")
            assert one[0].tobytes() == note[r0:r1].tobytes()  # the job's rows are this call's
            part = {k: np.empty_like(v[r0:r1]) for k, v in maps.items()}
            rc = m._lib.bp_track_maps(m._handle, r1 - r0, part["note"].ctypes.data, part["onset"].ctypes.data,
                                      part["contour"].ctypes.data, _native.BP_MEM_HOST)
            _native.check(m._lib, m._handle, rc, "bp_track_maps")
            for k in maps:
                maps[k][r0:r1] = part[k]
        by_host = EV.note_events_from_maps(m, offs, *[maps[k].ctypes.data for k in ("note", "onset", "contour")], _native.BP_MEM_HOST, prm)
        dev = {k: torch.from_numpy(v).cuda() for k, v in maps.items()}
        torch.cuda.synchronize()
        by_dev = EV.note_events_from_maps(m, offs, *[dev[k].data_ptr() for k in ("note", "onset", "contour")], _native.BP_MEM_DEVICE, prm)
    routes = {"pcm": by_pcm, "host maps": by_host, "device maps": by_dev}
    n_events = 0
    for name, (events, bends, ev_offs, status) in routes.items():
        assert ev_offs.tolist() == by_pcm[2].tolist() and ev_offs[1] == ev_offs[2], name
        assert status.tolist() == st_cand.tolist() == [0, 0, 0], name
        assert _records(events, bends, 0, int(ev_offs[-1]), True) == _records(by_pcm[0], by_pcm[1], 0, int(ev_offs[-1]), True), name
        for i in range(3):
            r0, r1 = int(offs[i]), int(offs[i + 1])
            want = NC.decode_candidates(note[r0:r1], bits[r0:r1], bend[r0:r1], prm) if r1 > r0 else []
            got = EV.clip_events(events, bends, ev_offs, i, True)
            assert len(got) == len(want), (name, i)
            for g, w in zip(got, want):
                assert tuple(g[:3]) == tuple(w[:3]) and np.float32(g[3]).tobytes() == np.float32(w[3]).tobytes(), (name, i, g, w)
                assert list(g[4]) == list(w[4]), (name, i)
            n_events += len(want)
    assert n_events >= 6  # the comparison is not one of empty lists
