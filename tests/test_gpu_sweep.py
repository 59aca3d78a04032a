"""Many parameter sets in one device call (bp_note_events_sweep / bp_infer_clips_events_sweep,
include/basic_pitch_amd_sweep.h; csrc/note_track.hip nt_track_sweep_kernel): decode by decode the records of the existing
single-set route on that segment alone — bp_note_events_from_maps (bp_infer_clips_events for clips), and for the fixture
cases the host path bp_note_candidates + bp_notes_decode_candidates — frames, pitch, the float32 amplitude's bit pattern,
times as float64, bend lists, event order and status."""
import ctypes as C
import re

import numpy as np
import pytest

import clip_files as CF
import note_cases

pytestmark = pytest.mark.gpu

MAPS = (("note", 88), ("onset", 88), ("contour", 264))


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


def _cat(outs):
    cat = {k: np.ascontiguousarray(np.concatenate([np.asarray(o[k], np.float32).reshape(-1, w) for o in outs])) for k, w in MAPS}
    offs = np.concatenate([[0], np.cumsum([o["note"].shape[0] for o in outs])]).astype(np.int64)
    return cat, offs


def _single(m, out, prm):
    """bp_note_events_from_maps on one segment alone: (records, status)."""
    from basic_pitch_amd import _native, events as EV

    cat, offs = _cat([out])
    ptr = [cat[k].ctypes.data if offs[-1] else None for k, _ in MAPS]
    events, bends, ev_offs, status = EV.note_events_from_maps(m, offs, *ptr, _native.BP_MEM_HOST, prm)
    return _records(events, bends, 0, int(ev_offs[1]), bool(prm.include_pitch_bends)), int(status[0])


def _unpack(events, bends, ev_offs, status, sets, pairs):
    """What a sweep returned as (records, status) per decode; bend_offset runs through the bends of all decodes in event order."""
    assert ev_offs[0] == 0 and (np.diff(ev_offs) >= 0).all() and len(ev_offs) == len(pairs) + 1 == len(status) + 1
    all_ev = events[: int(ev_offs[-1])]
    assert [e.bend_offset for e in all_ev] == np.concatenate([[0], np.cumsum([e.n_bends for e in all_ev])])[:-1].astype(int).tolist()
    out = []
    for j, (_, p) in enumerate(pairs):
        pb = bool(sets[p].include_pitch_bends)
        recs = _records(events, bends, int(ev_offs[j]), int(ev_offs[j + 1]), pb)
        assert pb or all(r[6] == 0 for r in recs)  # a set without bends contributes none
        out.append((recs, int(status[j])))
    return out


def _sweep(m, outs, sets, pairs=None, room=None):
    """One bp_note_events_sweep call on host maps: [(records, status)] per decode.  The caller's maps are left alone."""
    from basic_pitch_amd import _native, sweep as SW

    cat, offs = _cat(outs)
    before = {k: v.copy() for k, v in cat.items()}
    ptr = [cat[k].ctypes.data if offs[-1] else None for k, _ in MAPS]
    got = SW.note_events_sweep(m, offs, *ptr, _native.BP_MEM_HOST, sets, pairs, room)
    for k in cat:
        assert np.array_equal(cat[k].view(np.uint32), before[k].view(np.uint32)), k
    return _unpack(*got, sets, pairs if pairs is not None else SW.cross_product(len(sets), len(outs)))


def _same(got, want, where):
    assert got[1] == want[1], (where, "status", got[1], want[1])
    g, w = got[0], want[0] or []
    assert len(g) == len(w), (where, len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, (where, k, a, b)


# ---- 1: the fixture cases, each under its own arguments, in one call
def test_the_16_fixture_cases_each_under_its_own_arguments_in_one_call(model):
    names = list(note_cases.CASES)
    assert len(names) == 16
    maps, sets = [], []
    for name in names:
        out, args = note_cases.case_args(name)
        maps.append(out)
        sets.append(_prm({k: v for k, v in args.items() if k not in ("multiple_pitch_bends", "midi_tempo")}))
    got = _sweep(model, maps, sets, [(i, i) for i in range(16)])
    n_events = 0
    for i, name in enumerate(names):
        want = _host(model, maps[i], sets[i])
        _same(got[i], want, name)
        n_events += len(want[0] or [])
    assert n_events >= 100  # the comparison is not one of empty lists


# ---- 2: a cross product over handcrafted segments
BASE = dict(onset_thresh=0.5, frame_thresh=0.3, min_note_len=3, energy_tol=5, infer_onsets=True)
VARIED = [{}, {"onset_thresh": 0.6}, {"onset_thresh": 0.35}, {"onset_thresh": 0.0}, {"frame_thresh": 0.2}, {"min_note_len": 7},
          {"energy_tol": 2}, {"melodia_trick": False}, {"include_pitch_bends": False}, {"min_freq": 80.0}, {"max_freq": 1500.0},
          {"infer_onsets": False}]
ROWS = (0, 1, 5, 142, 432, 433)  # 433: the first that keeps its working state in the scratch buffer
LO_BIN, HI_BIN = 18, 69          # the bins 80 Hz and 1500 Hz round to


def _segment(rng, T):
    """Noise with sustained notes, among them pairs on both sides of the two band edges and notes at bins 0 and 87."""
    m = {"note": rng.uniform(0, 0.05, (T, 88)).astype(np.float32), "onset": rng.uniform(0, 0.3, (T, 88)).astype(np.float32),
         "contour": rng.uniform(0, 1, (T, 264)).astype(np.float32)}

    def put(t0, n, f, peak=0.9):
        t1 = min(T, t0 + n)
        if t0 >= t1:
            return
        m["note"][t0:t1, f] = rng.uniform(0.4, 0.9, t1 - t0).astype(np.float32)
        if peak:
            m["onset"][t0, f] = peak

    if T >= 5:
        put(1, 4, 40)
    if T >= 100:
        for k, f in enumerate((LO_BIN - 2, LO_BIN - 1, LO_BIN, LO_BIN + 1, HI_BIN - 2, HI_BIN - 1, HI_BIN, HI_BIN + 1, 0, 87)):
            put(3 + 5 * k, 30 + 3 * k, f, peak=(0.45, 0.55, 0.7, 0.9)[k % 4])
        put(60, 60, 30, peak=0), put(70, 8, 50), put(70, 5, 52), put(90, 50, 44, peak=0.58)  # melodia's, short ones, near 0.6
        for t0 in range(120, T - 12, 37):
            put(t0, int(rng.integers(4, 36)), int(rng.integers(2, 86)), peak=float(rng.uniform(0.3, 0.95)))
        m["note"][33:43, LO_BIN + 3] = m["note"][100:104, 30] = 0.25  # a tail and a gap between the two frame thresholds
        m["note"][95:98, 44] = 0.01                                     # a gap one of the two tolerances bridges
    if T > 300:
        put(150, 270, 60), put(10, T - 12, 75, peak=0)  # sums over more than 128 and more than 256 rows
    return m


@pytest.fixture(scope="module")
def job(model):
    """The segments, the sets, and every (set, segment) decoded once by the single call: single[p][i] = (records, status)."""
    rng = np.random.default_rng(2024)
    segs = [_segment(rng, T) for T in ROWS]
    sets = [_prm(dict(BASE, **v)) for v in VARIED]
    single = [[_single(model, s, prm) for s in segs] for prm in sets]
    return segs, sets, single


def test_the_reference_of_the_cross_product_tells_the_sets_apart(job):
    """The single calls themselves: every varied field changes some segment's records, both forms of the tracker give events,
    and the statuses are the ones the sets ask for."""
    segs, sets, single = job
    assert [s["note"].shape[0] for s in segs] == list(ROWS)
    for p, v in enumerate(VARIED):
        if v.get("onset_thresh") == 0.0:
            assert [st for _, st in single[p]] == [0, 1, 1, 1, 1, 1]  # the host's; no rows: nothing to decode
            continue
        assert [st for _, st in single[p]] == [0] * len(ROWS), v
        assert p == 0 or any(single[p][i][0] != single[0][i][0] for i in range(len(ROWS))), v
    assert all(len(single[0][i][0]) >= 10 for i in (3, 4, 5))
    assert sum(len(r) for row in single for r, _ in row) >= 500


def test_a_cross_product_equals_the_single_calls(model, job):
    from basic_pitch_amd import sweep as SW

    segs, sets, single = job
    got = _sweep(model, segs, sets)
    assert len(got) == len(sets) * len(segs)
    for j, (i, p) in enumerate(SW.cross_product(len(sets), len(segs))):
        _same(got[j], single[p][i], (VARIED[p], ROWS[i]))


def test_a_shuffled_table_with_duplicates_equals_its_own_permutation(model, job):
    from basic_pitch_amd import sweep as SW

    segs, sets, single = job
    rng = np.random.default_rng(5)
    pairs = SW.cross_product(len(sets), len(segs))
    pairs = pairs + [pairs[k] for k in rng.integers(0, len(pairs), 20)] + [(5, 0), (5, 0), (3, 4)]
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    got = _sweep(model, segs, sets, pairs)
    for j, (i, p) in enumerate(pairs):
        _same(got[j], single[p][i], (j, VARIED[p], ROWS[i]))


# ---- 3: independence
def test_decodes_that_share_rows_do_not_see_each_others_zeroed_cells(model, job):
    segs, _, _ = job
    sets = [_prm(dict(BASE, frame_thresh=ft)) for ft in (0.15, 0.3, 0.45, 0.6)]  # one dense key, four trackers
    pair = [segs[5], segs[3]]
    assert [s["note"].shape[0] for s in pair] == [433, 142]
    from basic_pitch_amd import sweep as SW

    assert len(SW.dense_keys(sets)[0]) == 1
    got = _sweep(model, pair, sets)
    want = [[_single(model, s, prm) for s in pair] for prm in sets]
    for p in range(4):
        for i in range(2):
            _same(got[p * 2 + i], want[p][i], (p, i))
    assert len({tuple(want[p][0][0]) for p in range(4)}) == 4  # the four decodes of the same rows differ


# ---- 4: a NaN outside one set's band and inside another's
def test_a_nan_outside_the_band_of_one_set_and_inside_that_of_another(model, job):
    segs, _, _ = job
    seg = {k: v.copy() for k, v in segs[3].items()}
    seg["note"][50, 5] = np.nan  # bin 5 is below 80 Hz
    clean = segs[3]
    sets = [_prm(dict(BASE, min_freq=80.0)), _prm(BASE), _prm(dict(BASE, max_freq=1500.0))]
    got = _sweep(model, [seg, clean], sets)
    want = [[_single(model, s, prm) for s in (seg, clean)] for prm in sets]
    assert [[w[1] for w in row] for row in want] == [[0, 0], [1, 0], [1, 0]]
    for p in range(3):
        for i in range(2):
            _same(got[p * 2 + i], want[p][i], (p, i))
    assert len(want[0][0][0]) >= 5


# ---- 5: maps in device memory
def test_maps_in_device_memory_equal_the_host_memory_call(model, job):
    import torch

    segs, sets, single = job
    dev = [{k: torch.from_numpy(s[k]).cuda() for k, _ in MAPS} for s in segs]
    before = [{k: d[k].clone() for k in d} for d in dev]
    res = model.sweep_note_events(dev, sets)
    host = model.sweep_note_events(segs, sets)
    torch.cuda.synchronize()
    for d, b in zip(dev, before):
        for k in d:
            assert torch.equal(d[k].view(torch.int32), b[k].view(torch.int32)), k
    assert len(res) == len(sets) and all(len(r) == len(segs) for r in res)
    key = lambda ev: None if ev is None else [(e[0], e[1], e[2], np.float32(e[3]).tobytes(), e[4]) for e in ev]  # noqa: E731
    for p in range(len(sets)):
        pb = bool(sets[p].include_pitch_bends)
        for i in range(len(segs)):
            assert res[p][i][1] == host[p][i][1] == single[p][i][1]
            assert key(res[p][i][0]) == key(host[p][i][0])
            if single[p][i][1] == 0:  # the tuples are the records' fields
                assert key(res[p][i][0]) == [(r[4], r[5], r[2], r[3], list(r[8]) if pb else None) for r in single[p][i][0]]
            else:
                assert res[p][i][0] is None
    # pairs: one tuple per pair
    some = [(5, 2), (3, 0), (5, 2), (0, 1)]
    listed = model.sweep_note_events(dev, sets, pairs=some)
    assert [(key(ev), st) for ev, st in listed] == [(key(res[p][i][0]), res[p][i][1]) for i, p in some]


# ---- 6: buffers too small
def test_buffers_too_small_say_what_is_needed_and_the_repeated_call_succeeds(model, job):
    from basic_pitch_amd import _native, sweep as SW

    segs, sets, single = job
    cat, offs = _cat(segs)
    lib = SW.bind(model._lib)
    arr = SW.sets_array(sets)
    n = len(sets) * len(segs)
    ev_offs, status = np.full(n + 1, -7, np.int64), np.full(n, -7, np.int32)

    def call(events, max_events, bends, max_bends):
        return lib.bp_note_events_sweep(model._handle, len(segs), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                        *[cat[k].ctypes.data for k, _ in MAPS], _native.BP_MEM_HOST, len(sets), C.addressof(arr), n,
                                        None, events, max_events, bends, max_bends, ev_offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                        status.ctypes.data)

    want_ev = sum(len(single[p][i][0] or []) for p in range(len(sets)) for i in range(len(segs)))
    want_b = sum(r[6] for p in range(len(sets)) for i in range(len(segs)) for r in single[p][i][0] or [])
    small = (_native.bp_note_event * 4)()
    few = np.zeros(16, np.int32)
    assert call(C.addressof(small), 4, few.ctypes.data, 16) == _native.BP_ERR_INVALID_ARG
    msg = model._lib.bp_last_error(model._handle).decode()
    m = re.search(r"(\d+) events and (\d+) bends are needed", msg)
    assert m and "bp_note_events_sweep" in msg and "n_decodes" in msg, msg
    assert (int(m.group(1)), int(m.group(2))) == (want_ev, want_b) and ev_offs[n] == want_ev
    pairs = SW.cross_product(len(sets), len(segs))
    assert status.tolist() == [single[p][i][1] for i, p in pairs]  # complete
    assert np.diff(ev_offs).tolist() == [len(single[p][i][0] or []) for i, p in pairs]
    # enough for the events, not for the bends
    events = (_native.bp_note_event * want_ev)()
    assert call(C.addressof(events), want_ev, few.ctypes.data, 16) == _native.BP_ERR_INVALID_ARG
    # exactly the sizes it asked for
    bends = np.zeros(want_b, np.int32)
    _native.check(model._lib, model._handle, call(C.addressof(events), want_ev, bends.ctypes.data, want_b), "bp_note_events_sweep")
    got = _unpack(events, bends, ev_offs, status, sets, pairs)
    for j, (i, p) in enumerate(pairs):
        _same(got[j], single[p][i], (VARIED[p], ROWS[i]))


# ---- 7: refusals
def test_refusals_name_the_index_and_leave_the_handle_usable(model, job):
    from basic_pitch_amd import _native, sweep as SW

    segs, sets, single = job
    INV = _native.BP_ERR_INVALID_ARG
    cat, offs = _cat(segs[:4])
    lib = SW.bind(model._lib)
    h = model._handle
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    events = (_native.bp_note_event * 64)()
    bends = np.zeros(4096, np.int32)

    def call(params, pairs, n_segs=4, n_decodes=None, row_offsets=offs):
        arr = SW.sets_array(params)
        tab = SW.decode_table(pairs) if pairs is not None and not hasattr(pairs, "_length_") else pairs
        n = n_decodes if n_decodes is not None else len(pairs)
        ev_offs, status = np.zeros(n + 1, np.int64), np.zeros(max(1, n), np.int32)
        rc = lib.bp_note_events_sweep(h, n_segs, p64(row_offsets), *[cat[k].ctypes.data for k, _ in MAPS], _native.BP_MEM_HOST,
                                      len(params), C.addressof(arr), n, C.addressof(tab) if tab is not None else None,
                                      C.addressof(events), 64, bends.ctypes.data, 4096, p64(ev_offs), status.ctypes.data)
        return rc, lib.bp_last_error(h).decode()

    def works():  # an ordinary call on the handle
        _same(_single(model, segs[3], sets[0]), single[0][3], "after a refusal")

    def refused(want, *args, **kw):
        rc, msg = call(*args, **kw)
        assert rc == INV and "bp_note_events_sweep" in msg and all(w in msg for w in want), msg
        works()

    good = [_prm(BASE), _prm(BASE), _prm(BASE)]
    refused(("set 1:", "never terminates"), [good[0], _prm(dict(BASE, frame_thresh=-0.1)), good[2]], [(0, 0)])
    refused(("set 2:", "min_note_len"), [good[0], good[1], _prm(dict(BASE, min_note_len=-1))], [(0, 0)])  # named by no decode
    refused(("decode 2:", "params 3"), good, [(0, 0), (1, 1), (2, 3)])
    refused(("decode 1:", "segment 4"), good, [(0, 0), (4, 1)])
    refused(("decode 1:", "segment -1"), good, [(0, 0), (-1, 1)])
    tab = SW.decode_table([(0, 0), (1, 1), (2, 2), (3, 0)])
    tab[3].reserved = 1
    refused(("decode 3:", "reserved"), good, tab, n_decodes=4)
    refused(("n_sets * n_segments",), good, None, n_decodes=11)
    # more decodes than a call takes: nothing could be queued, the segments have no rows
    none = np.zeros(301, np.int64)
    assert 300 * 300 > SW.MAX_DECODES
    refused(("BP_SWEEP_MAX_DECODES", "split the job"), [_prm(BASE)] * 300, None, n_segs=300, n_decodes=90000, row_offsets=none)
    # nothing to do is no error: no sets, no decodes, no rows
    for params, pairs, kw in (([], None, dict(n_decodes=0)), (good, [], {}), (good, None, dict(n_segs=3, n_decodes=9, row_offsets=none))):
        rc, msg = call(params, pairs, **kw)
        assert rc == _native.BP_OK, msg
    works()


# ---- 8: the handle afterwards
def test_the_handle_after_a_sweep(model, job):
    from basic_pitch_amd import _native, clips as CL

    segs, sets, single = job
    x = np.clip(np.round(CF.tones(30000, 1, 22050, 3)[:, 0] * 20000), -32768, 32767).astype(np.int16)
    arrays = [CL.as_clip(x, 0), CL.as_clip(x[:9000], 1)]
    prm = _prm(dict(BASE, min_freq=80.0))

    def candidates():
        offs, note, bits, bend, status = CL.infer_clips_candidates(model, arrays, 22050, prm)
        return offs.tobytes(), note.tobytes(), bits.tobytes(), bend.tobytes(), status.tobytes()

    def track_candidates():
        """bp_infer_pcm_raw_candidates on the first clip: its rows stay on the device for bp_track_maps."""
        T = CL.n_rows(len(x), 22050)
        one = [np.empty((T, w), t) for w, t in ((88, np.float32), (12, np.uint8), (88, np.int8))]
        status = C.c_int(-1)
        rc = model._lib.bp_infer_pcm_raw_candidates(model._handle, x.ctypes.data, _native.BP_PCM_S16, len(x), 1, 22050, C.byref(prm),
                                                    one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, C.byref(status))
        _native.check(model._lib, model._handle, rc, "bp_infer_pcm_raw_candidates")
        return T

    def track_maps(T):
        out = [np.zeros((T, w), np.float32) for _, w in MAPS]
        return model._lib.bp_track_maps(model._handle, T, *[o.ctypes.data for o in out], _native.BP_MEM_HOST)

    before = candidates(), _single(model, segs[3], prm)
    assert len(before[1][0]) >= 5
    T = track_candidates()
    assert T > 0 and track_maps(T) == _native.BP_OK
    got = _sweep(model, segs, sets[:3] + [prm])
    _same(got[3 * len(segs) + 3], before[1], "the sweep itself")
    assert track_maps(T) == _native.BP_ERR_INVALID_ARG  # refused: a sweep leaves no maps, as the other clips calls
    assert candidates() == before[0]
    _same(_single(model, segs[3], prm), before[1], "after a sweep")
    # ... and straight after a sweep, without a call between them that would re-initialise the clips calls' records
    _sweep(model, segs, sets[:2])
    assert candidates() == before[0]


# ---- 9, 10: clips through the model
HANDLES = ("default", "bf16_weights", "ext_cqt_44k")


@pytest.fixture(scope="module")
def handles(model):
    from basic_pitch_amd.inference import Model

    made = {"default": model}

    def get(mode):
        if mode not in made:
            made[mode] = Model(device=0, max_windows=8, **{mode: True})
        return made[mode]

    yield get
    for mode, m in made.items():
        if mode != "default":
            m.close()


def _clips_at(m, sr):
    """100 samples, one window and two windows of tones at `sr`, as int16 mono."""
    rate = m.sample_rate
    hop, lead = 36164 * rate // 22050, 3840 * rate // 22050
    frames = lambda n_model: n_model * sr // rate  # noqa: E731
    clips = []
    for seed, n in ((1, 100), (2, frames(hop - lead)), (3, frames(hop + hop // 3))):
        x = CF.tones(n, 1, sr, seed)
        clips.append(np.clip(np.round(x * (0.85 / np.abs(x).max()) * 32767), -32768, 32767).astype(np.int16))
    return clips


CLIP_SETS = [{}, {"onset_thresh": 0.6, "min_freq": 80.0}, {"infer_onsets": False, "max_freq": 1500.0, "include_pitch_bends": False}]


@pytest.mark.parametrize("mode", HANDLES)
def test_clips_through_the_model_equal_the_single_set_call(handles, mode):
    from basic_pitch_amd import clips as CL, events as EV, sweep as SW

    m = handles(mode)
    sets = [_prm(v) for v in CLIP_SETS]
    assert len(SW.dense_keys(sets)[0]) == 3
    n_events = 0
    for sr in (22050, 44100):
        arrays = [CL.as_clip(c, i) for i, c in enumerate(_clips_at(m, sr))]
        rows = np.diff(CL.clips_row_offsets(m, arrays, sr)).tolist()
        assert rows[0] == 0 and 0 < rows[1] <= 142 < rows[2] <= 284, rows  # no rows, one window, two windows
        want = []
        for prm in sets:
            ev, b, offs, st = EV.infer_clips_events(m, arrays, sr, prm)
            pb = bool(prm.include_pitch_bends)
            want.append([(_records(ev, b, int(offs[i]), int(offs[i + 1]), pb), int(st[i])) for i in range(3)])
        got = _unpack(*SW.infer_clips_events_sweep(m, arrays, sr, sets), sets, SW.cross_product(3, 3))
        for p in range(3):
            for i in range(3):
                _same(got[p * 3 + i], want[p][i], (mode, sr, p, i))
                assert want[p][i][1] == 0
                n_events += len(want[p][i][0])
            assert len(want[p][1][0]) >= 1 and len(want[p][2][0]) >= 1 and want[p][0][0] == []
    assert n_events >= 12


def test_transcribe_clips_sweep_equals_transcribe_clips_per_set(model):
    clips = _clips_at(model, 22050) + _clips_at(model, 44100)
    rates = [22050] * 3 + [44100] * 3
    variants = [dict(onset_threshold=0.5, frame_threshold=0.3), dict(onset_threshold=0.6, frame_threshold=0.3, minimum_frequency=80.0),
                dict(onset_threshold=0.5, frame_threshold=0.2, maximum_frequency=1500.0, melodia_trick=False),
                dict(onset_threshold=0.0, frame_threshold=0.3)]  # the last: every decode is finished by the host route
    from basic_pitch_amd import inference as I, note_creation as NC

    sets = [NC._note_params(v["onset_threshold"], v["frame_threshold"], I._min_note_len_frames(I.DEFAULT_MINIMUM_NOTE_LENGTH_MS), True,
                            v.get("maximum_frequency"), v.get("minimum_frequency"), v.get("melodia_trick", True), NC.ENERGY_TOLERANCE,
                            True) for v in variants]
    got = model.transcribe_clips_sweep(clips, rates, sets)
    assert len(got) == len(sets) and all(len(g) == len(clips) for g in got)
    key = lambda ev: [(e[0], e[1], e[2], np.float32(e[3]).tobytes(), e[4]) for e in ev]  # noqa: E731
    for p, v in enumerate(variants):
        want = model.transcribe_clips(clips, rates, decode="device", **v)
        for i in range(len(clips)):
            assert key(got[p][i]) == key(want[i][1]), (v, i)
        assert sum(len(w[1]) for w in want) >= 4
