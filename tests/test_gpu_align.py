"""Forced alignment on the device (include/basic_pitch_amd_align.h; csrc/align.hip): first_frame, total and status of
bp_align_from_maps are byte for byte those of the host checker bp_align_rows, segment by segment — at the shapes where the
kernels can go wrong (the read-ahead depth, the backtrace tile, the window seams, the wave and workgroup edges of the states,
a lane's second state, BP_ALIGN_MAX_STATES, the forced diagonal, the extreme sums, the K padding) —, several segments of mixed
sizes in one call with a status-1 and a status-2 segment among them, maps in host and in device memory, pool reuse, the other
calls on the handle undisturbed, clips through the model, the non-default handles, and planted paths."""
import ctypes as C

import numpy as np
import pytest

import align_cases as AC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

INV = -1
DEPTH, TILE, LANES, SMALL, MAX_STATES = 8, 128, 1024, 256, 4096  # BP_ALIGN_* (compared with the binding's below)


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import align as AL
    from basic_pitch_amd.inference import Model

    assert (AL.READ_AHEAD, AL.TILE_ROWS, AL.LANES, AL.SMALL_LANES, AL.MAX_STATES) == (DEPTH, TILE, LANES, SMALL, MAX_STATES)
    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host(segs, prm=None):
    """The host checker on every segment: (first frames of all states, totals, statuses)."""
    from basic_pitch_amd import align as AL

    got = [AL.align_rows(n, o, st, prm) if len(n) or len(st) else (np.zeros(0, np.int32), 0, 0) for n, o, st in segs]
    return (np.concatenate([g[0] for g in got]).astype(np.int32), np.array([g[1] for g in got], np.int64), np.array([g[2] for g in got], np.int32))


def _device(model, segs, prm=None, where="host"):
    import torch

    from basic_pitch_amd import _native, align as AL

    offs, note, onset, s_offs, states = AC.stack(segs)
    if where == "host":
        before = (note.copy(), onset.copy())
        got = AL.align_from_maps(model, offs, note.ctypes.data, onset.ctypes.data, _native.BP_MEM_HOST, s_offs, states, prm)
        after = (note, onset)
    else:
        before = (note, onset)
        dn, do = torch.from_numpy(note).cuda(), torch.from_numpy(onset).cuda()
        torch.cuda.synchronize()
        got = AL.align_from_maps(model, offs, dn.data_ptr(), do.data_ptr(), _native.BP_MEM_DEVICE, s_offs, states, prm)
        after = (dn.cpu().numpy(), do.cpu().numpy())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before)), "the maps are left untouched"
    return got


def _assert_equal(got, want, where):
    for g, w, name in zip(got, want, ("first_frame", "total", "status")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (where, name, g[:16], w[:16])


def _problem(seed, rows, S, kind="thousand", windows=False, most=4):
    rng = np.random.default_rng(seed)
    note, onset = AC.random_maps(rng, rows, kind)
    return note, onset, AC.random_states(rng, S, rows, windows=windows, most=most)


# (rows, S) per group: each shape is a call of its own, so that the states of the shape choose the workgroup
SHAPES = {
    # the read-ahead depth and one frame around it, and the shortest segments
    "read_ahead": [(1, 1), (2, 1), (2, 2), (DEPTH - 1, 3), (DEPTH, 3), (DEPTH + 1, 3), (DEPTH + 1, DEPTH + 1), (2 * DEPTH + 1, 5)],
    # the backtrace tile -+ 1, two tiles + 1; the window seams of the model's rows
    "tile": [(TILE - 1, 40), (TILE, 40), (TILE + 1, 40), (2 * TILE + 1, 70), (171, 9), (172, 9), (173, 9), (345, 33)],
    # the waves of the states, the emission tile of 32, the workgroup of 256 lanes -+ 1
    "waves": [(90, 1), (90, 2), (90, 31), (90, 32), (90, 33), (90, 63), (90, 64), (90, 65), (300, SMALL - 1), (300, SMALL), (300, SMALL + 1),
              (600, 2 * SMALL + 1)],
    # the workgroup of 1024 lanes -+ 1, a lane's second state, the step from two to four states a lane
    "lanes": [(LANES + 40, LANES - 1), (LANES + 40, LANES), (LANES + 40, LANES + 1), (2 * LANES + 9, 2 * LANES), (2 * LANES + 9, 2 * LANES + 1)],
    # the bound itself, forced and with three frames to spare; the forced diagonal at small sizes
    "max_states": [(MAX_STATES, MAX_STATES), (MAX_STATES + 3, MAX_STATES)],
    "diagonal": [(100, 100), (65, 65), (SMALL + 1, SMALL + 1)],
}


@pytest.mark.parametrize("group", list(SHAPES))
def test_the_shapes_where_the_kernels_can_go_wrong(model, group):
    moved = 0
    for k, (rows, S) in enumerate(SHAPES[group]):
        for windows in ((False, True) if S > 1 and rows > S and S <= 2 * SMALL + 1 else (False,)):
            segs = [_problem(1000 * len(group) + 10 * k + windows, rows, S, "eighths" if k % 2 else "thousand", windows)]
            want = _host(segs)
            _assert_equal(_device(model, segs), want, (group, rows, S, windows))
            assert want[2][0] == 0 or windows, (group, rows, S)
            if want[2][0] == 0 and rows > S:
                moved += int(np.any(np.diff(want[0]) > 1))
    assert moved > 0 or group in ("max_states", "diagonal") or all(r == s for r, s in SHAPES[group]), group


def test_the_extreme_sums_and_the_k_padding(model):
    """A chord of all 88 pitches with threshold_q 0 and 1024 and onset_weight 16 on maps of ones and zeros (the largest and the
    smallest gains there are), and states of pitch 87 alone and pitch 0 alone beside the padding of K to 96."""
    everything = list(range(88))
    rng = np.random.default_rng(5)
    for fill in (1.0, 0.0, None):
        rows = 70
        if fill is None:
            note, onset = AC.random_maps(rng, rows)
        else:
            note = onset = np.full((rows, 88), fill, np.float32)
        chord = AC.make_states([everything, [], everything, [87], [0], [0, 87], everything], [everything, [], everything, [87], [0], [87], []])
        for prm in (dict(threshold_q=0, onset_weight=16), dict(threshold_q=1024, onset_weight=16), dict(threshold_q=1024, onset_weight=0)):
            want = _host([(note, onset, chord)], prm)
            _assert_equal(_device(model, [(note, onset, chord)], prm), want, (fill, prm))
            assert want[2][0] == 0
    ones = np.ones((3, 88), np.float32)
    want = _host([(ones, ones, AC.make_states([everything], [everything]))], dict(threshold_q=0, onset_weight=16))
    assert want[1][0] == 3 * 88 * 1024 + 16 * 88 * 1024
    # pitch 87 and pitch 0 alone carry the whole gain: the map is zero but for that column
    for pitch in (87, 0):
        note = np.zeros((40, 88), np.float32)
        note[13:, pitch] = 1.0
        onset = np.zeros((40, 88), np.float32)
        onset[13, pitch] = 0.75
        st = AC.make_states([[], [pitch]], [[], [pitch]])
        want = _host([(note, onset, st)])
        _assert_equal(_device(model, [(note, onset, st)]), want, pitch)
        assert want[0].tolist() == [0, 13] and want[1][0] == 27 * (1024 - 307) + 2 * 768


def _mixed_job():
    segs = [_problem(40, 433, 70, windows=True), _problem(41, 9, 3), _problem(42, 172, 1), _problem(43, 64, 64, "eighths"),
            _problem(44, 50, 7), _problem(45, 20, 21), _problem(46, 345, 200), (np.zeros((0, 88), np.float32),) * 2 + (np.zeros(0, AC.STATE),),
            (np.zeros((0, 88), np.float32),) * 2 + (AC.make_states([[3], [4]]),), _problem(47, 130, 40, "eighths", windows=True)]
    segs[4][0][49, 87] = np.nan                       # status 1: the last row, a pitch no state need use
    segs[9][2]["earliest"][5], segs[9][2]["latest"][5] = 128, 129
    segs[9][2]["earliest"][6], segs[9][2]["latest"][6] = 3, 4   # status 2: a window that closes before its predecessor opens
    return segs


@pytest.mark.parametrize("where", ["host", "device"])
def test_several_segments_of_mixed_sizes_in_one_call(model, where):
    segs = _mixed_job()
    want = _host(segs)
    assert want[2].tolist() == [0, 0, 0, 0, 1, 2, 0, 0, 2, 2]
    got = _device(model, segs, None, where)
    _assert_equal(got, want, where)
    # no other segment is affected: each of the others alone gives the same
    for i in (0, 3, 6):
        alone = _device(model, [segs[i]], None, where)
        s_offs = np.concatenate([[0], np.cumsum([len(s[2]) for s in segs])])
        assert alone[0].tobytes() == got[0][s_offs[i]:s_offs[i + 1]].tobytes() and alone[1][0] == got[1][i]


def test_a_smaller_call_after_a_larger_one_and_the_other_calls_undisturbed(model):
    from basic_pitch_amd import _native, melody as ME

    rng = np.random.default_rng(3)
    out = TS._segment(rng, 142)
    note_prm = TS._prm(TS.BASE)
    sets = [TS._prm(dict(TS.BASE, **v)) for v in TS.VARIED[:3]]
    contour = np.ascontiguousarray(out["contour"])

    def others():
        ev = TS._single(model, out, note_prm)
        sw = TS._sweep(model, [out], sets)
        mel = ME.melody_from_maps(model, [0, 142], contour.ctypes.data, _native.BP_MEM_HOST)
        return (ev, sw, mel[0].tobytes(), mel[1].tolist())  # (the events as TS._records' comparable tuples)

    before = others()
    assert len(before[0][0]) > 0 and len(before[1]) == 3
    large = [_problem(60, 700, 300, windows=True), _problem(61, 200, 90)]
    small = [_problem(62, 33, 5), _problem(63, 12, 12, "eighths")]
    _assert_equal(_device(model, large), _host(large), "large")
    for where in ("host", "device"):
        _assert_equal(_device(model, small, None, where), _host(small), ("small after large", where))
    # the maps of the model's own segment: a real score for it from its own events would do no more than random states here
    own = (out["note"], out["onset"], AC.random_states(rng, 11, 142))
    _assert_equal(_device(model, [own]), _host([own]), "the segment of the other calls")
    assert others() == before


def test_nothing_to_do_the_refusals_and_too_little_room(model):
    from basic_pitch_amd import _native, align as AL

    lib = AL.bind(model._lib)
    h = model._handle
    segs = [_problem(70, 30, 4), _problem(71, 20, 3)]
    offs, note, onset, s_offs, states = AC.stack(segs)
    want = _host(segs)
    p = AL.align_params()
    ff = np.full(16, 77, np.int32)
    total, status = np.full(4, 77, np.int64), np.full(4, 77, np.int32)
    zero = np.zeros(4, np.int64)

    def call(n=2, offs=offs, note_p=note.ctypes.data, onset_p=onset.ctypes.data, kind=_native.BP_MEM_HOST, s_offs=s_offs, states=states, p=p,
             ff_p=ff.ctypes.data, room=16, total_p=_p64(total), status_p=status.ctypes.data):
        st = np.ascontiguousarray(states, AC.STATE)
        return lib.bp_align_from_maps(h, n, _p64(offs), note_p, onset_p, kind, _p64(s_offs) if s_offs is not None else None,
                                      st.ctypes.data if len(st) else None, C.addressof(p), ff_p, room, total_p, status_p)

    def refused(rc, *words):
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and "bp_align_from_maps" in msg and all(w in msg for w in words), (rc, msg)
        assert np.all(ff == 77) and np.all(total == 77) and np.all(status == 77), "a refused call wrote to its outputs"

    # zero segments; segments without rows and states; states without rows are infeasible: no device work
    assert call(n=0, offs=zero, note_p=None, onset_p=None, s_offs=None, states=states[:0], ff_p=None, room=0, total_p=None, status_p=None) == 0
    assert call(n=3, offs=zero, note_p=None, onset_p=None, s_offs=zero, states=states[:0], ff_p=None, room=0) == 0
    assert total[:3].tolist() == [0, 0, 0] and status[:3].tolist() == [0, 0, 0]
    some = np.array([0, 2, 2, 3], np.int64)
    assert call(n=3, offs=zero, note_p=None, onset_p=None, s_offs=some, states=states[:3]) == 0
    assert ff[:3].tolist() == [-1, -1, -1] and status[:3].tolist() == [2, 0, 2] and total[:3].tolist() == [0, 0, 0]
    ff[:], total[:], status[:] = 77, 77, 77
    # the refusals, each before anything is queued or written
    refused(call(n=-1), "negative")
    refused(call(offs=np.array([1, 30, 50], np.int64)), "row_offsets")
    refused(call(offs=np.array([0, 30, 29], np.int64)), "row_offsets")
    refused(call(kind=7), "mem_kind")
    refused(call(note_p=None), "null input")
    refused(call(onset_p=None), "null input")
    refused(call(s_offs=np.array([1, 4, 7], np.int64)), "state_offsets")
    refused(call(s_offs=np.array([0, 4, 3], np.int64)), "state_offsets")
    refused(call(s_offs=None), "state_offsets")
    refused(call(total_p=None), "total")
    refused(call(status_p=None), "status")
    refused(call(room=6), "room for 6", "7 states", "nothing has been written")
    refused(call(room=-1), "max_states")
    refused(call(ff_p=None), "without a buffer")
    for field, value in (("threshold_q", 1025), ("onset_weight", 17), ("reserved", 1)):
        refused(call(p=AL.align_params(**{field: value})), "params", field if field != "reserved" else "reserved")
    refused(call(s_offs=np.array([0, 0, 7], np.int64)), "segment 0", "no state")
    broken = states.copy()
    broken["begins"][5, 0] = ~broken["active"][5, 0]
    refused(call(states=broken), "state 5", "subset")
    broken = states.copy()
    broken["earliest"][6], broken["latest"][6] = 4, 3
    refused(call(states=broken), "state 6", "latest")
    many = AC.make_states([[1]] * (MAX_STATES + 1))
    big = np.full(MAX_STATES + 1, 77, np.int32)
    rc = call(n=1, offs=np.array([0, 50], np.int64), s_offs=np.array([0, MAX_STATES + 1], np.int64), states=many, ff_p=big.ctypes.data, room=len(big))
    refused(rc, "segment 0", "BP_ALIGN_MAX_STATES")
    assert np.all(big == 77)
    # the bounds over all segments, refused from the offsets alone (nothing is read)
    refused(call(n=1, offs=np.array([0, 8388609], np.int64), s_offs=np.array([0, 1], np.int64), states=states[:1]), "BP_SWEEP_MAX_ROWS")
    rc = call(n=1, offs=np.array([0, 65537], np.int64), s_offs=np.array([0, MAX_STATES], np.int64), states=many[:MAX_STATES], ff_p=big.ctypes.data,
              room=MAX_STATES)
    refused(rc, "BP_ALIGN_MAX_CELLS", "segment 0")
    assert 65537 * MAX_STATES > AL.MAX_CELLS >= 65536 * MAX_STATES and np.all(big == 77)
    # and the handle is usable: the same arguments, unbroken
    assert call() == 0
    assert ff[:7].tobytes() == want[0].tobytes() and np.all(ff[7:] == 77) and total[:2].tolist() == want[1].tolist() and status[:2].tolist() == [0, 0]


# ---- planted paths, through the device
def test_planted_first_frames_are_recovered_exactly_on_the_device(model):
    problems = [AC.planted(seed) for seed in range(24)]
    segs = [(n, o, st) for n, o, st, _ in problems]
    got = _device(model, segs, None, "device")
    assert got[2].tolist() == [0] * len(segs)
    assert got[0].tolist() == np.concatenate([f for *_, f in problems]).tolist()
    _assert_equal(got, _host(segs), "planted")


# ---- clips through the model
def _float_clips(model, sr):
    return [(c.astype(np.float32) / np.float32(32768.0)).reshape(-1, 1) for c in TS._clips_at(model, sr)]


def _scores_for(rng, rows):
    """A score per segment: states with windows now and then; a segment without rows gets none."""
    return [AC.random_states(rng, min(r, int(rng.integers(1, 30))), r, windows=True) if r else np.zeros(0, AC.STATE) for r in rows]


def test_clips_through_the_model_equal_from_maps_on_their_own_maps(model):
    """Four short PCM clips IN ONE CALL of bp_infer_clips_align against bp_align_from_maps on the maps the model gives for them,
    and Model.transcribe_clips_align (two sample rates) against Model.align on Model's outputs."""
    from basic_pitch_amd import align as AL, clips as CL

    clips = _float_clips(model, 22050) + [_float_clips(model, 22050)[1][::-1].copy()]
    assert len(clips) == 4
    arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
    outs = [model.predict_pcm(c, 22050) for c in clips]
    rows = [len(o["note"]) for o in outs]
    assert np.diff(CL.clips_row_offsets(model, arrays, 22050)).tolist() == rows and rows[0] == 0 and min(rows[1:]) > 100  # (100 samples: no row, and no state)
    rng = np.random.default_rng(8)
    scores = _scores_for(rng, rows)
    s_offs = np.concatenate([[0], np.cumsum([len(s) for s in scores])]).astype(np.int64)
    got = AL.infer_clips_align(model, arrays, 22050, s_offs, np.concatenate(scores))
    segs = [(np.asarray(o["note"], np.float32), np.asarray(o["onset"], np.float32), s) for o, s in zip(outs, scores)]
    _assert_equal(got, _device(model, segs), "bp_infer_clips_align against bp_align_from_maps")
    _assert_equal(got, _host(segs), "bp_infer_clips_align against the checker")
    assert got[2].tolist() == [0, 0, 0, 0]
    # the Python entries: reference notes in, aligned notes out
    mixed = clips[1:3] + _float_clips(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    m_outs = [model.predict_pcm(c, r) for c, r in zip(mixed, rates)]
    refs = [np.array([[0.1, 0.4, 60.0], [0.4, 0.9, 64.2], [0.9, 1.3, 64.0]]), np.array([[0.0, 0.5, 45.0]]), np.zeros((0, 3)),
            np.array([[0.2, 0.6, 72.0], [0.3, 0.6, 76.0]])]
    for how in (dict(), dict(threshold_q=400, onset_weight=0, max_shift_s=1.0, tail=False)):
        via_clips = model.transcribe_clips_align(mixed, rates, refs, **how)
        via_maps = model.align(m_outs, refs, **how)
        for a, b, ref, out in zip(via_clips, via_maps, refs, m_outs):
            assert (a.status, a.total) == (b.status, b.total) and a.first_frame.tobytes() == b.first_frame.tobytes()
            assert a.status == 0 and a.notes.tobytes() == b.notes.tobytes() and a.notes.shape == ref.shape
            states = AL.states_from_notes(ref, len(out["note"]), **{k: v for k, v in how.items() if k in ("max_shift_s", "tail")})[0]
            ff, total, status = AL.align_rows(out["note"], out["onset"], states, **{k: v for k, v in how.items() if k in ("threshold_q", "onset_weight")})
            assert (a.first_frame.tolist(), a.total, a.status) == (ff.tolist(), total, status)
            assert np.all(a.notes[:, 1] >= a.notes[:, 0]) and np.array_equal(a.notes[:, 2], ref[:, 2])
    assert model.align([], []) == []


def test_the_model_entry_takes_host_and_device_outputs(model):
    import torch

    rng = np.random.default_rng(9)
    outs = [TS._segment(rng, 142), TS._segment(rng, 60)]
    refs = [np.array([[0.2, 0.5, 50.0], [0.5, 0.8, 50.0], [0.6, 1.2, 57.0]]), np.array([[0.0, 0.3, 30.0], [0.1, 0.2, 100.0]])]
    host = model.align(outs, refs)
    dev = model.align([{k: torch.from_numpy(v).cuda() for k, v in o.items()} for o in outs], refs)
    for a, b in zip(host, dev):
        assert a.status == b.status == 0 and a.total == b.total and a.first_frame.tobytes() == b.first_frame.tobytes()
        assert a.notes.tobytes() == b.notes.tobytes()
    with pytest.raises(ValueError):
        model.align(outs, refs[:1])
    with pytest.raises(TypeError):
        model.align(outs, refs, threshold=0.3)
    with pytest.raises(ValueError, match="note 1"):
        model.align(outs, [refs[0], np.array([[0.0, 0.3, 30.0], [0.1, 0.2, 120.0]])])


# ---- the non-default handles
@pytest.mark.parametrize("mode", ["bf16_weights", "ext_cqt_44k"])
def test_on_the_non_default_handles_the_call_equals_the_checker_on_that_handles_own_maps(mode):
    """In the manner of tests/test_gpu_mode_matrix.py: the handle's own geometry decides the clips, its own maps the reference."""
    from basic_pitch_amd import align as AL, clips as CL
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8, **{mode: True}) as m:
        sr = m.sample_rate
        clips = _float_clips(m, sr)[1:]
        arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
        outs = [m.predict_pcm(c, sr) for c in clips]
        rows = [len(o["note"]) for o in outs]
        rng = np.random.default_rng(10)
        scores = _scores_for(rng, rows)
        s_offs = np.concatenate([[0], np.cumsum([len(s) for s in scores])]).astype(np.int64)
        segs = [(np.asarray(o["note"], np.float32), np.asarray(o["onset"], np.float32), s) for o, s in zip(outs, scores)]
        want = _host(segs)
        _assert_equal(AL.infer_clips_align(m, arrays, sr, s_offs, np.concatenate(scores)), want, (mode, "clips"))
        _assert_equal(_device(m, segs), want, (mode, "maps"))
        assert want[2].tolist() == [0, 0] and min(rows) > 100
