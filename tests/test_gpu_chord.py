"""Chords and key on the device (include/basic_pitch_amd_chord.h; csrc/chord.hip): the summaries and labels of
bp_chords_from_maps are byte for byte those of the host checker bp_chord_rows, segment by segment — one job of many segments at
the lengths where the kernels can go wrong (no row, 1, 2, 63, 64, 65 rows, a block of the chroma kernel and a tile of the
backtrace -+ 1, every kind of map, a long segment) under every parameter set of tests/chord_cases.py and every boundary list,
the note map in host memory, in device memory and in device memory off a 16-byte boundary, and left untouched —, a segment with
a NaN among neighbours that do not notice, too little room, the refusals, the Python entries with the beats of Model.beats, and
the call between two other sinks of one handle."""
import ctypes as C
import functools

import numpy as np
import pytest

import chord_cases as CC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

INV = -1
CHROMA_ROWS, TRACE_TILE, PATH_WAVES = 32, 512, 4  # BP_CHORD_* (compared with the binding's and the header's below)


@pytest.fixture(scope="module")
def model():
    import os
    import re

    from basic_pitch_amd import chord as CH
    from basic_pitch_amd.inference import Model
    from conftest import ROOT

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_chord.h")).read()
    for macro, ours, theirs in (("BP_CHORD_CHROMA_ROWS", CHROMA_ROWS, CH.CHROMA_ROWS), ("BP_CHORD_TRACE_TILE", TRACE_TILE, CH.TRACE_TILE),
                                ("BP_CHORD_PATH_WAVES", PATH_WAVES, CH.PATH_WAVES)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == ours == theirs, macro
    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


@functools.lru_cache(maxsize=None)
def _job():
    segs = CC.job_segments(CHROMA_ROWS, TRACE_TILE)
    return [s[0] for s in segs], [s[1] for s in segs]


def _host(maps, prm=None, bounds=None):
    """The host checker on every segment: (summaries, labels of all rows), the outputs of the device call."""
    from basic_pitch_amd import chord as CH

    got = [CH.chord_rows_raw(m, prm, None if bounds is None else bounds[i]) for i, m in enumerate(maps)]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got] + [np.zeros(0, np.uint8)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _wanted(name, mode):
    """The checker's results of the job under one parameter set and one boundary list: computed once, shared, left alone."""
    from basic_pitch_amd import chord as CH

    _, maps = _job()
    want = _host(maps, CH.chord_params(CC.PARAM_SETS[name]), CC.job_bounds(mode, maps, CHROMA_ROWS))
    for a in want:
        a.setflags(write=False)
    return want


def _device(model, maps, prm=None, where="host", bounds=None):
    import torch

    from basic_pitch_amd import _native, chord as CH

    offs = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    note = np.ascontiguousarray(np.concatenate(maps), np.float32)
    if where == "host":
        before = note.copy()
        got = CH.chords_from_maps(model, offs, note.ctypes.data, _native.BP_MEM_HOST, prm, bounds)
        after = note
    else:
        before = note
        shift = 1 if where == "device_unaligned" else 0  # one float: 4 bytes off a 16-byte boundary
        dev = torch.empty(note.size + 4, dtype=torch.float32, device="cuda")
        assert dev.data_ptr() % 16 == 0
        view = dev[shift : shift + note.size]
        view.copy_(torch.from_numpy(note.reshape(-1)))
        torch.cuda.synchronize()
        assert (view.data_ptr() % 16 != 0) == bool(shift)
        got = CH.chords_from_maps(model, offs, view.data_ptr(), _native.BP_MEM_DEVICE, prm, bounds)
        after = view.cpu().numpy().reshape(note.shape)
    assert after.tobytes() == before.tobytes(), "the map is left untouched"
    return got


def _assert_equal(got, want, where):
    for g, w, name in zip(got, want, ("summaries", "labels")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (where, name, g[:8], w[:8])


def test_the_jobs_cases_do_what_they_are_there_for():
    """Properties of the checker's results, before the device is asked."""
    names, maps = _job()
    assert [len(m) for m in maps[:7]] == [0, 1, 2, 63, 64, 65, CHROMA_ROWS - 1]
    assert {CHROMA_ROWS, CHROMA_ROWS + 1, TRACE_TILE - 1, TRACE_TILE, TRACE_TILE + 1, 2049} <= {len(m) for m in maps}
    summaries, labels = _wanted("default", "none")
    status = dict(zip(names, summaries["status"].tolist()))
    assert status["no rows"] == status["150 silence"] == status["150 under"] == 2 and sum(s == 2 for s in status.values()) >= 3
    assert int(summaries["n_changes"].sum()) > 50, "more than 50 changes in all"
    offs = np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    tie, raised = names.index("97 tie"), names.index("97 tie, one cell raised")
    assert labels[offs[tie]:offs[tie + 1]].tolist() == [1] * 97 and labels[offs[raised]:offs[raised + 1]].tolist() == [13] * 97  # C:maj, C:min
    for mode in CC.BOUND_MODES[1:]:
        bounds = CC.job_bounds(mode, maps, CHROMA_ROWS)
        assert len(bounds) == len(maps) and all(np.all(np.diff([0] + b + [len(m)]) > 0) for b, m in zip(bounds, maps) if len(m))
    assert CC.job_bounds("every", maps, CHROMA_ROWS)[5] == list(range(1, 65))
    spans = CC.job_bounds("spans", maps, CHROMA_ROWS)[-1]
    assert np.diff(spans)[:5].tolist() == [1, 1, 2 * CHROMA_ROWS + 5, 1, 1]  # units of one frame beside one that spans two blocks
    mixed = CC.job_bounds("mixed", maps, CHROMA_ROWS)
    assert any(len(b) for b in mixed) and any(not b and len(m) > 1 for b, m in zip(mixed, maps))
    every = _wanted("default", "every")
    assert every[0].tobytes() == summaries.tobytes() and every[1].tobytes() == labels.tobytes()  # boundaries at every frame: frame units


@pytest.mark.parametrize("where", ["host", "device", "device_unaligned"])
@pytest.mark.parametrize("name", list(CC.PARAM_SETS))
def test_one_job_of_many_segments_equals_the_checker_byte_for_byte(model, name, where):
    from basic_pitch_amd import chord as CH

    prm = CH.chord_params(CC.PARAM_SETS[name])
    _, maps = _job()
    for mode in CC.BOUND_MODES:
        _assert_equal(_device(model, maps, prm, where, CC.job_bounds(mode, maps, CHROMA_ROWS)), _wanted(name, mode), (name, where, mode))


def test_a_segment_with_a_nan_has_status_1_and_its_neighbours_do_not_notice(model):
    rng = np.random.default_rng(3)
    maps = [CC.triads(rng, 300, 25), CC.noise(rng, 130), CC.triads(rng, 500), CC.noise(rng, 10), CC.plateaux(rng, 433)]
    offs = np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    bounds = [CC.irregular(rng, len(m)) if i % 2 == 0 else [] for i, m in enumerate(maps)]
    clean = _device(model, maps, None, "host", bounds)
    _assert_equal(clean, _host(maps, None, bounds), "clean")
    for i, (row, pitch) in ((1, (129, 87)), (0, (0, 0)), (3, (4, 40)), (2, (257, 3))):
        bad = [m.copy() for m in maps]
        bad[i][row, pitch] = np.nan
        got = _device(model, bad, None, "device", bounds)
        _assert_equal(got, _host(bad, None, bounds), ("a NaN in", i))
        assert got[0][i].tolist() == (1, -1, 0, 0, 0, 0) and not got[1][offs[i]:offs[i + 1]].any()
        for j in range(len(maps)):
            if j != i:  # the others: the bytes they have without it
                assert got[0][j].tobytes() == clean[0][j].tobytes()
                assert got[1][offs[j]:offs[j + 1]].tobytes() == clean[1][offs[j]:offs[j + 1]].tobytes()


def test_nothing_to_do_the_refusals_and_too_little_room(model):
    from basic_pitch_amd import _native, chord as CH

    lib = CH.bind(model._lib)
    h = model._handle
    rng = np.random.default_rng(70)
    maps = [CC.triads(rng, 200, 20), CC.noise(rng, 90)]
    offs = np.array([0, 200, 290], np.int64)
    note = np.concatenate(maps)
    bound_lists = [[50, 51, 120], [45]]
    want = _host(maps, None, bound_lists)
    p = CH.chord_params()
    b_offs = np.array([0, 3, 4], np.int64)
    b = np.array([50, 51, 120, 45], np.int32)
    summaries = np.zeros(4, CC.SUMMARY)
    labels = np.full(400, 77, np.uint8)
    zero = np.zeros(4, np.int64)

    def fresh():
        summaries.view(np.uint8)[:] = 77
        labels[:] = 77

    def call(n=2, offs=offs, note_p=note.ctypes.data, kind=_native.BP_MEM_HOST, p=p, b_offs=b_offs, b=b, summaries_p=summaries.ctypes.data,
             labels_p=labels.ctypes.data, room=290):
        return lib.bp_chords_from_maps(h, n, _p64(offs), note_p, kind, C.addressof(p) if p is not None else None,
                                       _p64(b_offs) if b_offs is not None else None, b.ctypes.data if b is not None else None, summaries_p,
                                       labels_p, room)

    def refused(rc, *words):
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and "bp_chords_from_maps" in msg and all(w in msg for w in words), (rc, msg)
        assert np.all(summaries.view(np.uint8) == 77) and np.all(labels == 77), "a refused call wrote to its outputs"

    fresh()
    # zero segments; segments without rows: no device work, status 2
    assert call(n=0, offs=zero, note_p=None, b_offs=None, b=None, summaries_p=None, labels_p=None, room=0) == 0
    assert call(n=3, offs=zero, note_p=None, b_offs=None, b=None, labels_p=None, room=0) == 0
    assert summaries[:3].tolist() == [(2, -1, 0, 0, 0, 0)] * 3 and np.all(labels == 77)
    fresh()
    # the refusals, each before anything is queued or written
    refused(call(n=-1), "negative")
    refused(call(offs=np.array([1, 200, 290], np.int64)), "row_offsets")
    refused(call(offs=np.array([0, 200, 199], np.int64)), "row_offsets")
    refused(call(kind=7), "mem_kind")
    refused(call(note_p=None), "null input")
    refused(call(summaries_p=None), "summaries")
    refused(call(p=None), "params")
    refused(call(room=289), "room for 289", "290", "nothing has been written")  # one below the rows
    refused(call(room=-1), "max_labels")
    refused(call(labels_p=None), "without a buffer")
    refused(call(b=None), "go together")
    refused(call(b_offs=None), "go together")
    refused(call(b_offs=np.array([1, 3, 4], np.int64)), "bound_offsets")
    refused(call(b_offs=np.array([0, 3, 2], np.int64)), "bound_offsets")
    for bad, seg in (([50, 50, 120, 45], 0), ([50, 51, 200, 45], 0), ([0, 51, 120, 45], 0), ([50, 51, 120, 90], 1), ([50, 51, 120, -3], 1),
                     ([51, 50, 120, 45], 0)):
        refused(call(b=np.array(bad, np.int32)), f"segment {seg}", "boundaries")
    for field, value, word in (("threshold_q", 1025, "threshold_q"), ("n_states", 0, "n_states"), ("n_states", 65, "n_states"),
                               ("switch_penalty", 1025, "switch_penalty"), ("max_pitch", 88, "max_pitch"), ("reserved", 1, "reserved"),
                               ("reserved", (0, 0, 1), "reserved")):
        refused(call(p=CH.chord_params(**{field: value})), "params", word)
    table = np.zeros((64, 12), np.int64)
    table[63, 11] = 1025
    refused(call(p=CH.chord_params(weights=table, n_states=2)), "params", "weights")
    refused(call(p=CH.chord_params(bias=[0, -1025], n_states=2)), "params", "bias")
    refused(call(p=CH.chord_params(key_profile=np.full((2, 12), 2000))), "params", "key_profile")
    # the bounds, refused from the offsets alone (nothing is read): the segment is named
    big = np.array([0, 10, 10 + CH.MAX_ROWS + 1], np.int64)
    refused(call(offs=big, room=10 ** 6, b_offs=None, b=None), "segment 1", "BP_CHORD_MAX_ROWS")
    many = np.arange(0, 18 * CH.MAX_ROWS, CH.MAX_ROWS, dtype=np.int64)
    refused(call(n=17, offs=many, room=10 ** 7, b_offs=None, b=None), "BP_SWEEP_MAX_ROWS")
    # and the handle is usable: the same arguments, unbroken, with exactly the room the rows ask for
    assert call() == 0
    assert summaries[:2].tobytes() == want[0].tobytes() and labels[:290].tobytes() == want[1].tobytes() and np.all(labels[290:] == 77)
    assert np.all(summaries[2:].view(np.uint8) == 77)


def test_the_chord_call_between_two_other_sinks_leaves_their_bytes_unchanged(model):
    """Events before, beats after, on one handle: both give the bytes they give without the chord calls between them (a larger
    one, then smaller ones, which also shows the grow-only buffers reused)."""
    from basic_pitch_amd import _native, beat as BT, events as EV
    from test_gpu_clips_events import _prm, _records

    rng = np.random.default_rng(4)
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in TS._segment(rng, 142).items()}
    offs = np.array([0, 142], np.int64)
    prm = _prm({})

    def events():
        ev, bends, ev_offs, status = EV.note_events_from_maps(model, offs, out["note"].ctypes.data, out["onset"].ctypes.data,
                                                              out["contour"].ctypes.data, _native.BP_MEM_HOST, prm)
        return _records(ev, bends, 0, int(ev_offs[-1]), True), ev_offs.tobytes(), status.tobytes()

    def beats():
        return tuple(x.tobytes() for x in BT.beats_from_maps(model, offs, out["onset"].ctypes.data, _native.BP_MEM_HOST))

    events_alone, beats_alone = events(), beats()
    events_before = events()
    large = [CC.triads(rng, 3000, 30), CC.noise(rng, 700)]
    small = [CC.triads(rng, 60, 5), CC.plateaux(rng, 30)]
    _assert_equal(_device(model, large), _host(large), "large")
    for where in ("host", "device"):
        _assert_equal(_device(model, small, None, where, [[7, 30], []]), _host(small, None, [[7, 30], []]), ("small after large", where))
    _assert_equal(_device(model, [out["note"]]), _host([out["note"]]), "the segment of the other calls")
    beats_after = beats()
    assert events_before == events_alone and beats_after == beats_alone and events() == events_alone
    assert len(events_alone[0]) > 0


# ---- the Python entries and clips through the model
def _float_clips(model, sr):
    return [(c.astype(np.float32) / np.float32(32768.0)).reshape(-1, 1) for c in TS._clips_at(model, sr)]


def test_the_python_entries_with_beats_and_clips_through_the_model_equal_the_checker(model, tmp_path):
    """Model.chords with beats=Model.beats(...), and Model.transcribe_clips_chords (two sample rates), against the checker on the
    maps of the single-clip call."""
    import torch

    from basic_pitch_amd import chord as CH

    mixed = _float_clips(model, 22050)[1:3] + _float_clips(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    outs = [model.predict_pcm(c, r) for c, r in zip(mixed, rates)]
    assert min(len(o["note"]) for o in outs) > 100
    beats = model.beats(outs)
    assert any(len(b.frames) >= 2 for b in beats)
    beats[0].frames = np.concatenate([[0], beats[0].frames[beats[0].frames != 0]]).astype(np.int32)  # a beat at frame 0 is dropped
    for prm in (None, dict(vocabulary="sevenths", switch_penalty=32, threshold_q=200)):
        names = CH.chord_names((prm or {}).get("vocabulary", "majmin"))
        for given in (None, beats):
            via_maps = model.chords(outs, prm, beats=given)
            via_dev = model.chords([{k: torch.from_numpy(np.asarray(v)).cuda() for k, v in o.items()} for o in outs], prm, beats=given)
            via_clips = model.transcribe_clips_chords(mixed, rates, prm, bounds=given)
            for i, (a, b, d, out) in enumerate(zip(via_maps, via_dev, via_clips, outs)):
                host = CH.chord_rows(out["note"], prm, None if given is None else given[i])
                for x in (a, b, d):
                    assert (x.status, x.key, x.key_index, x.n_units, x.n_changes, x.score, x.key_score, x.runs) == \
                        (host.status, host.key, host.key_index, host.n_units, host.n_changes, host.score, host.key_score, host.runs)
                    assert x.labels.dtype == np.uint8 and x.labels.tobytes() == host.labels.tobytes() and x.times_s.tobytes() == host.times_s.tobytes()
                if a.status == 0:
                    assert a.key in CH.KEY_NAMES and all(name in names for _, _, name in a.runs)
                    assert a.n_units == (len(out["note"]) if given is None or not len(CH._boundaries(given[i])) else len(CH._boundaries(given[i])) + 1)
    path = tmp_path / "clip.lab"
    CH.write_lab(str(path), via_maps[0])
    lines = path.read_text().splitlines()
    assert len(lines) == len(via_maps[0].runs) and lines[0].split()[0] == f"{via_maps[0].times_s[0, 0]:.6f}" and lines[-1].split()[2] == via_maps[0].runs[-1][2]
    assert model.chords([]) == [] and model.transcribe_clips_chords([], []) == []
    with pytest.raises(TypeError):
        model.chords(outs, dict(threshold=0.3))
    with pytest.raises(ValueError):
        model.chords(outs, beats=beats[:1])
