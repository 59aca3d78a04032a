"""Tempo and beats on the device (include/basic_pitch_amd_beat.h; csrc/beat.hip): the summaries, beat_offsets and beats of
bp_beats_from_maps are byte for byte those of the host checker bp_beat_rows, segment by segment — one job of many segments at
the lengths where the kernels can go wrong (no row, one row, lag_min and lag_min + 1 rows, the shortest and the widest block of
the path kernel, the LDS ring's length and a row tile of the tempo kernel -+ 1, every kind of map, a long segment) under every
parameter set of tests/beat_cases.py, the onset map in host and in device memory and left untouched —, a segment with a NaN
among neighbours that do not notice, too little room, the refusals, and clips through the model."""
import ctypes as C

import numpy as np
import pytest

import beat_cases as BC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

INV = -1
RING, TILE_ROWS, TILE_LAGS, WAVES, MAX_LAG = 1024, 256, 64, 16, 256  # BP_BEAT_* (compared with the binding's below)


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import beat as BT
    from basic_pitch_amd.inference import Model

    assert (BT.RING, BT.TEMPO_ROWS, BT.TEMPO_LAGS, BT.PATH_WAVES, BT.MAX_LAG) == (RING, TILE_ROWS, TILE_LAGS, WAVES, MAX_LAG)
    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host(maps, prm=None):
    """The host checker on every segment: (summaries, beats of all segments, beat_offsets), the outputs of the device call."""
    from basic_pitch_amd import beat as BT

    got = [BT.beat_rows_raw(m, prm) for m in maps]
    beats = np.concatenate([g[1] for g in got] + [np.zeros(0, np.int32)]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(g[1]) for g in got])]).astype(np.int64)
    return np.concatenate([g[0] for g in got]), beats, offsets


def _device(model, maps, prm=None, where="host"):
    import torch

    from basic_pitch_amd import _native, beat as BT

    offs = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    onset = np.ascontiguousarray(np.concatenate(maps), np.float32)
    if where == "host":
        before = onset.copy()
        got = BT.beats_from_maps(model, offs, onset.ctypes.data, _native.BP_MEM_HOST, prm)
        after = onset
    else:
        before = onset
        dev = torch.from_numpy(onset).cuda()
        torch.cuda.synchronize()
        got = BT.beats_from_maps(model, offs, dev.data_ptr(), _native.BP_MEM_DEVICE, prm)
        after = dev.cpu().numpy()
    assert after.tobytes() == before.tobytes(), "the map is left untouched"
    return got


def _assert_equal(got, want, where):
    for g, w, name in zip(got, want, ("summaries", "beats", "beat_offsets")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (where, name, g[:8], w[:8])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", list(BC.PARAM_SETS))
def test_one_job_of_many_segments_equals_the_checker_byte_for_byte(model, name, where):
    from basic_pitch_amd import beat as BT

    fields = BC.PARAM_SETS[name]
    prm = BT.beat_params(fields)
    segs = BC.job_segments(fields, RING, TILE_ROWS)
    names, maps = [s[0] for s in segs], [s[1] for s in segs]
    assert [len(m) for m in maps[:4]] == [0, 1, prm.lag_min, prm.lag_min + 1] and len(maps[4]) == 2 * prm.lag_min + 1
    assert {RING - 1, RING, RING + 1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 433, 2049} <= {len(m) for m in maps}
    want = _host(maps, prm)
    status = dict(zip(names, want[0]["status"].tolist()))
    period = dict(zip(names, want[0]["period"].tolist()))
    # the inputs do what they are there for (properties of the checker's results, before the device is asked)
    assert status["no rows"] == status["one row"] == status["lag_min rows"] == status["433 silence"] == 2
    assert status["lag_min + 1 rows"] == 0 and period["lag_min + 1 rows"] == prm.lag_min  # one lag only
    assert status["period lag_min"] == 0 and period["period lag_min"] == prm.lag_min      # the shortest block of the path kernel
    if prm.lag_max == MAX_LAG:
        assert period["period 256"] == MAX_LAG  # dmin 128 ... dmax 512: 385 candidates, every lane form
    assert int(want[2][-1]) > 50 and sum(s == 2 for s in status.values()) >= 4, "many beats and some segments without a pulse"
    _assert_equal(_device(model, maps, prm, where), want, (name, where))


def test_a_segment_with_a_nan_has_status_1_and_its_neighbours_do_not_notice(model):
    rng = np.random.default_rng(3)
    maps = [BC.pulses(rng, 300, 40), BC.noise(rng, 130), BC.pulses(rng, 500, 55), BC.noise(rng, 10), BC.eighths(rng, 433)]
    clean = _device(model, maps)
    _assert_equal(clean, _host(maps), "clean")
    for i, (row, pitch) in ((1, (129, 87)), (0, (0, 0)), (3, (4, 40)), (2, (257, 3))):
        bad = [m.copy() for m in maps]
        bad[i][row, pitch] = np.nan
        got = _device(model, bad, None, "device")
        _assert_equal(got, _host(bad), ("a NaN in", i))
        assert got[0][i].tolist() == (1, 0, 0, 0, 0.0) and got[2][i + 1] == got[2][i]
        for j in range(len(maps)):
            if j != i:  # the others: the bytes they have without it
                assert got[0][j].tobytes() == clean[0][j].tobytes()
                assert got[1][got[2][j]:got[2][j + 1]].tobytes() == clean[1][clean[2][j]:clean[2][j + 1]].tobytes()


def test_nothing_to_do_the_refusals_and_too_little_room(model):
    from basic_pitch_amd import _native, beat as BT

    lib = BT.bind(model._lib)
    h = model._handle
    rng = np.random.default_rng(70)
    maps = [BC.pulses(rng, 200, 33), BC.noise(rng, 90)]
    offs = np.array([0, 200, 290], np.int64)
    onset = np.concatenate(maps)
    want = _host(maps)
    p = BT.beat_params()
    cap = BT.beats_capacity(200, 21) + BT.beats_capacity(90, 21)
    assert cap == 20 + 9
    summaries = np.zeros(4, BC.SUMMARY)
    beats = np.full(64, 77, np.int32)
    offsets = np.full(5, 77, np.int64)
    zero = np.zeros(4, np.int64)

    def fresh():
        summaries.view(np.uint8)[:] = 77
        beats[:], offsets[:] = 77, 77

    def call(n=2, offs=offs, onset_p=onset.ctypes.data, kind=_native.BP_MEM_HOST, p=p, summaries_p=summaries.ctypes.data,
             beats_p=beats.ctypes.data, room=cap, offsets_p=_p64(offsets)):
        return lib.bp_beats_from_maps(h, n, _p64(offs), onset_p, kind, C.addressof(p) if p is not None else None, summaries_p, beats_p, room,
                                      offsets_p)

    def refused(rc, *words):
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and "bp_beats_from_maps" in msg and all(w in msg for w in words), (rc, msg)
        assert np.all(summaries.view(np.uint8) == 77) and np.all(beats == 77) and np.all(offsets == 77), "a refused call wrote to its outputs"

    fresh()
    # zero segments; segments without rows: no device work, status 2
    assert call(n=0, offs=zero, onset_p=None, summaries_p=None, beats_p=None, room=0, offsets_p=None) == 0
    assert call(n=3, offs=zero, onset_p=None, beats_p=None, room=0) == 0
    assert summaries[:3].tolist() == [(2, 0, 0, 0, 0.0)] * 3 and offsets[:4].tolist() == [0, 0, 0, 0]
    fresh()
    # the refusals, each before anything is queued or written
    refused(call(n=-1), "negative")
    refused(call(offs=np.array([1, 200, 290], np.int64)), "row_offsets")
    refused(call(offs=np.array([0, 200, 199], np.int64)), "row_offsets")
    refused(call(kind=7), "mem_kind")
    refused(call(onset_p=None), "null input")
    refused(call(summaries_p=None), "summaries")
    refused(call(offsets_p=None), "beat_offsets")
    refused(call(p=None), "params")
    refused(call(room=cap - 1), "room for 28", "29", "nothing has been written")  # one below the capacity
    refused(call(room=-1), "max_beats")
    refused(call(beats_p=None), "without a buffer")
    for field, value, word in (("threshold_q", 1025, "threshold_q"), ("lag_min", 1, "lag_min"), ("lag_max", 257, "lag_max"),
                               ("tightness", 1025, "tightness"), ("max_pitch", 88, "max_pitch"), ("reserved", 1, "reserved"),
                               ("reserved_tail", 1, "reserved")):
        refused(call(p=BT.beat_params(**{field: value})), "params", word)
    table = BC.FLAT.copy()
    table[77] = 1025
    refused(call(p=BT.beat_params(prior=table)), "params", "prior")
    # the bounds, refused from the offsets alone (nothing is read): the segment is named
    big = np.array([0, 10, 10 + BT.MAX_ROWS + 1], np.int64)
    refused(call(offs=big, room=10 ** 6), "segment 1", "BP_BEAT_MAX_ROWS")
    many = np.arange(0, 18 * BT.MAX_ROWS, BT.MAX_ROWS, dtype=np.int64)
    refused(call(n=17, offs=many, room=10 ** 7), "BP_SWEEP_MAX_ROWS")
    # and the handle is usable: the same arguments, unbroken, with exactly the room the bound asks for
    assert call() == 0
    n = int(want[2][-1])
    assert summaries[:2].tobytes() == want[0].tobytes() and offsets[:3].tolist() == want[2].tolist()
    assert beats[:n].tobytes() == want[1].tobytes() and np.all(beats[n:] == 77) and np.all(offsets[3:] == 77)


def test_a_smaller_call_after_a_larger_one_and_the_other_calls_undisturbed(model):
    from basic_pitch_amd import _native, melody as ME

    rng = np.random.default_rng(4)
    out = TS._segment(rng, 142)
    contour = np.ascontiguousarray(out["contour"])
    before = ME.melody_from_maps(model, [0, 142], contour.ctypes.data, _native.BP_MEM_HOST)
    large = [BC.pulses(rng, 3000, 43), BC.noise(rng, 700)]
    small = [BC.pulses(rng, 60, 25), BC.eighths(rng, 30)]
    _assert_equal(_device(model, large), _host(large), "large")
    for where in ("host", "device"):
        _assert_equal(_device(model, small, None, where), _host(small), ("small after large", where))
    _assert_equal(_device(model, [out["onset"]]), _host([out["onset"]]), "the segment of the other calls")
    after = ME.melody_from_maps(model, [0, 142], contour.ctypes.data, _native.BP_MEM_HOST)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tolist() == after[1].tolist()


def test_planted_beats_come_back_exactly_on_the_device(model):
    problems = [BC.planted(seed) for seed in range(30)]
    maps = [m for m, _, _ in problems]
    got = _device(model, maps, None, "device")
    assert got[0]["status"].tolist() == [0] * 30 and got[0]["period"].tolist() == [p for _, p, _ in problems]
    assert got[1].tolist() == [t for _, _, beats in problems for t in beats]
    _assert_equal(got, _host(maps), "planted")


# ---- clips through the model
def _float_clips(model, sr):
    return [(c.astype(np.float32) / np.float32(32768.0)).reshape(-1, 1) for c in TS._clips_at(model, sr)]


def test_clips_through_the_model_equal_from_maps_on_their_own_onset_rows(model):
    """A few one-window and two-window PCM clips IN ONE CALL of bp_infer_clips_beats against bp_beats_from_maps on the onset
    rows the model gives for them, and Model.transcribe_clips_beats (two sample rates) against Model.beats on Model's outputs."""
    import torch

    from basic_pitch_amd import beat as BT, clips as CL

    clips = _float_clips(model, 22050) + [_float_clips(model, 22050)[1][::-1].copy(), _float_clips(model, 22050)[2][::-1].copy()]
    assert len(clips) == 5
    arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
    outs = [model.predict_pcm(c, 22050) for c in clips]
    rows = [len(o["onset"]) for o in outs]
    assert np.diff(CL.clips_row_offsets(model, arrays, 22050)).tolist() == rows and rows[0] == 0 and min(rows[1:]) > 100
    maps = [np.asarray(o["onset"], np.float32).reshape(-1, 88) for o in outs]
    for prm in (None, dict(threshold_q=100, lag_min=10, lag_max=MAX_LAG, tightness=16)):
        got = BT.infer_clips_beats(model, arrays, 22050, prm)
        _assert_equal(got, _device(model, maps, prm), "bp_infer_clips_beats against bp_beats_from_maps")
        _assert_equal(got, _host(maps, prm), "bp_infer_clips_beats against the checker")
        assert got[0]["status"][0] == 2
    # the Python entries: objects out
    mixed = clips[1:3] + _float_clips(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    m_outs = [model.predict_pcm(c, r) for c, r in zip(mixed, rates)]
    for prm in (None, dict(threshold_q=100, start_bpm=90.0, sd_octaves=0.5)):
        via_clips = model.transcribe_clips_beats(mixed, rates, prm)
        via_maps = model.beats(m_outs, prm)
        via_dev = model.beats([{k: torch.from_numpy(np.asarray(v)).cuda() for k, v in o.items()} for o in m_outs], prm)
        for a, b, d, out in zip(via_clips, via_maps, via_dev, m_outs):
            host = BT.beat_rows(out["onset"], prm)
            for x in (a, b, d):
                assert (x.status, x.period, x.score, x.period_frames, x.bpm) == (host.status, host.period, host.score, host.period_frames, host.bpm)
                assert x.frames.dtype == np.int32 and x.frames.tobytes() == host.frames.tobytes() and x.times_s.tobytes() == host.times_s.tobytes()
            if a.status == 0:
                assert a.bpm == 60 * 22050 / 256 / a.period_frames and len(a.frames) >= 1
    assert model.beats([]) == [] and model.transcribe_clips_beats([], []) == []
    with pytest.raises(TypeError):
        model.beats(m_outs, dict(threshold=0.3))
