"""Note events from the device for a job of clips, the part that needs no GPU: the calls of
include/basic_pitch_amd_events.h are exported with the prototypes that header declares, the capacity of a clip's region equals
its Python mirror, and argument errors are refused before anything is queued.

A handle needs a device.  Where one can be made the refusals are read from `bp_last_error`; without one the native calls'
answer to a null handle and the refusals of the Python layer are what is checked."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("bp_events_capacity", "bp_infer_clips_events", "bp_note_events_from_maps")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, clips, events

    build.build_library()
    return events.bind(clips.bind(_native.load_library()))


@pytest.fixture(scope="module")
def model():
    """A model where a device is visible, else None."""
    from basic_pitch_amd import _native
    from basic_pitch_amd.inference import Model

    try:
        m = Model(device=0, max_windows=8)
    except _native.NativeLibraryError:
        yield None
        return
    yield m
    m.close()


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p}


def _ctype_of(param):
    """The rule of tests/test_clips_cpu.py: handles and plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_every_symbol_of_the_events_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, events
    from basic_pitch_amd.inference import Model

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_events.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert '#include "basic_pitch_amd_clips.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(events.PROTOTYPES) == set(_native.EVENTS_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert events.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["params", "events", "max_events", "bends", "max_bends", "event_offsets", "status"]
    assert names("bp_infer_clips_events") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert names("bp_note_events_from_maps") == ["h", "n_clips", "row_offsets", "note", "onset", "contour", "mem_kind"] + tail
    assert re.search(r"#define BP_EVENTS_MAX_ROWS (\d+)", header).group(1) == str(events.MAX_ROWS)
    # the existing headers and lists are what they were
    assert not set(NEW) & (set(_native.EXPORTED_SYMBOLS) | set(_native.CLIPS_SYMBOLS))
    assert hasattr(Model, "note_events")


def test_the_capacity_of_a_region_equals_its_python_mirror(lib):
    from basic_pitch_amd import events

    rows = [-1, 0, 1, 2, 3, 11, 12, 13, 23, 24, 25, 141, 142, 143, 432, 433, 568, 700, 2130, 8191, 8192, 8193, 10 ** 6]
    for r in rows:
        for mnl in (-3, 0, 1, 3, 10, 11, 12, 141, 142, 5000):
            assert lib.bp_events_capacity(r, mnl) == events.events_capacity(r, mnl), (r, mnl)
    # the documented formula on the shapes the job of clips has: 88 pitches x the disjoint notes of min_note_len + 1 rows
    assert events.events_capacity(142, 11) == 88 * 12 and events.events_capacity(144, 11) == 88 * 12
    assert events.events_capacity(145, 11) == 88 * 13 and events.events_capacity(64, 0) == 88 * 64
    assert events.events_capacity(8193, 11) == 0 == events.bends_capacity(8193) and events.bends_capacity(142) == 88 * 142


def test_argument_errors_are_refused_with_a_message(lib, model):
    from basic_pitch_amd import _native, clips

    INV = _native.BP_ERR_INVALID_ARG
    offs = np.zeros(4, np.int64)
    p_offs = offs.ctypes.data_as(C.POINTER(C.c_int64))
    prm = _native.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    good = [np.zeros((100, 2), np.int16), np.zeros(50, np.float32), np.zeros((0, 1), np.uint8)]
    tab = clips.clip_table([clips.as_clip(c, i) for i, c in enumerate(good)])
    status = np.zeros(4, np.int32)
    # the native calls without a handle
    assert lib.bp_infer_clips_events(None, 3, tab, 44100, 0, C.addressof(prm), None, 0, None, 0, p_offs, status.ctypes.data) == INV
    assert lib.bp_note_events_from_maps(None, 1, p_offs, None, None, None, 0, C.addressof(prm), None, 0, None, 0, p_offs,
                                        status.ctypes.data) == INV
    with pytest.raises(ValueError, match="decode must be"):
        clips.transcribe_clips(None, good, 44100, 0.5, 0.3, 127.7, None, None, False, True, 120, decode="gpu")
    if model is None:
        return
    h = model._handle
    err = lambda: lib.bp_last_error(h).decode()  # noqa: E731
    ev = (_native.bp_note_event * 8)()
    bends = np.zeros(64, np.int32)
    rows = np.array([0, 2, 2, 5], np.int64)
    p_rows = rows.ctypes.data_as(C.POINTER(C.c_int64))
    maps = [np.zeros((5, 88), np.float32), np.zeros((5, 88), np.float32), np.zeros((5, 264), np.float32)]

    def both(want, prm=prm, n=3, events=C.addressof(ev), max_events=8, bends_p=bends.ctypes.data, max_bends=64, eo=p_offs,
             st=status.ctypes.data):
        rc = lib.bp_infer_clips_events(h, n, tab, 44100, _native.BP_MEM_HOST, C.addressof(prm) if prm is not None else None,
                                       events, max_events, bends_p, max_bends, eo, st)
        assert rc == INV and want in err() and "bp_infer_clips_events" in err(), err()
        rc = lib.bp_note_events_from_maps(h, n, p_rows, *[a.ctypes.data for a in maps], _native.BP_MEM_HOST,
                                          C.addressof(prm) if prm is not None else None, events, max_events, bends_p, max_bends, eo, st)
        assert rc == INV and want in err() and "bp_note_events_from_maps" in err(), err()

    both("null params", prm=None)
    both("negative n_clips", n=-1)
    both("event_offsets", eo=None)
    both("status", st=None)
    both("max_events", max_events=-1)
    both("room without a buffer", events=None)
    both("room without a buffer", bends_p=None)
    bad = _native.bp_note_params()
    lib.bp_note_params_default(C.byref(bad))
    bad.frame_threshold = -0.1
    both("never terminates", prm=bad)
    bad.frame_threshold, bad.min_note_len = 0.3, -1
    both("min_note_len", prm=bad)
    # the clips' own argument domain, and the maps'
    t = clips.clip_table([clips.as_clip(c, i) for i, c in enumerate(good)])
    t[1].channels = 0
    rc = lib.bp_infer_clips_events(h, 3, t, 44100, _native.BP_MEM_HOST, C.addressof(prm), C.addressof(ev), 8, bends.ctypes.data, 64,
                                   p_offs, status.ctypes.data)
    assert rc == INV and "clip 1:" in err()
    args = (C.addressof(prm), C.addressof(ev), 8, bends.ctypes.data, 64, p_offs, status.ctypes.data)
    for bad_rows in ([1, 2, 2, 5], [0, 3, 2, 5]):
        r = np.array(bad_rows, np.int64)
        rc = lib.bp_note_events_from_maps(h, 3, r.ctypes.data_as(C.POINTER(C.c_int64)), *[a.ctypes.data for a in maps], 0, *args)
        assert rc == INV and "row_offsets" in err()
    assert lib.bp_note_events_from_maps(h, 3, None, *[a.ctypes.data for a in maps], 0, *args) == INV and "row_offsets" in err()
    assert lib.bp_note_events_from_maps(h, 3, p_rows, *[a.ctypes.data for a in maps], 5, *args) == INV and "mem_kind" in err()
    assert lib.bp_note_events_from_maps(h, 3, p_rows, maps[0].ctypes.data, None, maps[2].ctypes.data, 0, *args) == INV
    assert "null input pointer" in err()
