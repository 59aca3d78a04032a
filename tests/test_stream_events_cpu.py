"""Note events of many live streams from the device, the part that needs no GPU: the calls of
include/basic_pitch_amd_stream_events.h are exported with the prototypes and the struct that header declares, the layout's
arithmetic equals its Python mirror, and `transcripts` checks its arguments."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("bp_streams_events_layout", "bp_streams_events")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, events, streaming

    build.build_library()
    return events.bind(streaming.bind(_native.load_library()))


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "bp_stream": C.c_void_p}


def _ctype_of(param):
    """The rule of tests/test_clips_events_cpu.py: handles and plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_every_symbol_of_the_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, streaming
    from basic_pitch_amd.inference import Model

    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_stream_events.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "basic_pitch_amd_update.h"' in header and '#include "basic_pitch_amd_events.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(streaming.STREAM_EVENTS_PROTOTYPES) == set(_native.STREAM_EVENTS_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert streaming.STREAM_EVENTS_PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    assert names("bp_streams_events") == ["h", "n", "u", "with_tail", "events", "max_events", "bends", "max_bends", "event_offsets"]
    assert names("bp_streams_events_layout") == ["h", "n", "u", "with_tail", "events_capacity", "bends_capacity"]
    # the struct, field by field
    body = re.search(r"typedef struct bp_stream_events \{(.*?)\} bp_stream_events;", header, flags=re.S).group(1)
    fields = [(t, n) for t, n in re.findall(r"(\w+)\s+(\w+);", body)]
    ctypes_of = {"bp_stream": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(_native.bp_stream_events._fields_)
    assert [n for _, n in fields] == ["stream", "first_row", "n_rows", "status"] and C.sizeof(_native.bp_stream_events) == 32
    # the existing headers and lists are what they were
    others = (set(_native.EXPORTED_SYMBOLS) | set(_native.LIVE_SYMBOLS) | set(_native.ROLLING_SYMBOLS) | set(_native.UPDATE_SYMBOLS)
              | set(_native.CLIPS_SYMBOLS) | set(_native.EVENTS_SYMBOLS))
    assert not set(NEW) & others
    assert _native.UPDATE_SYMBOLS == ["bp_streams_update_layout", "bp_streams_candidates"]
    assert "decode" in Model.transcripts.__code__.co_varnames and "midi" in Model.transcripts.__code__.co_varnames


def test_the_layouts_arithmetic_equals_its_python_mirror(lib):
    from basic_pitch_amd import events, streaming

    for rows_out in (0, 1, 141, 142, 284, 431, 432, 433, 5168, 8192, 8193, 10 ** 7):
        for tail in (0, 1, 142, 284):
            assert streaming.slice_first_row(rows_out, tail, None) == (0, rows_out + tail)
            for horizon in (3, 150, 432, 5168, 8192, 1 << 40):
                a, T = streaming.slice_first_row(rows_out, tail, horizon)
                assert T == rows_out + tail and a == lib.bp_stream_horizon_first_row(T, horizon) and T - a == min(T, horizon)
    slices = [(0, 11, True), (1, 0, True), (433, 11, False), (5452, 11, True), (8192, 5, True), (8193, 11, True), (300, 0, False)]
    cap_e, cap_b = streaming.streams_events_capacity(slices)
    assert cap_e == sum(lib.bp_events_capacity(r, m) for r, m, _ in slices)
    assert cap_b == 88 * (1 + 5452 + 8192)  # streams with bends, none for a slice the device leaves out
    assert events.events_capacity(8193, 11) == 0 and streaming.streams_events_capacity([]) == (0, 0)


def test_arguments_are_checked_before_any_device_work(lib):
    from basic_pitch_amd import _native, streaming

    INV = _native.BP_ERR_INVALID_ARG
    offs = (C.c_int64 * 2)()
    tab = (_native.bp_stream_events * 1)()
    cap = C.c_int64(0)
    assert lib.bp_streams_events(None, 1, C.addressof(tab), 1, None, 0, None, 0, offs) == INV
    assert lib.bp_streams_events_layout(None, 1, C.addressof(tab), 1, C.byref(cap), C.byref(cap)) == INV
    for bad in ("gpu", "", None):
        with pytest.raises(ValueError, match="decode must be"):
            streaming.transcripts(None, [], decode=bad)
    assert streaming.transcripts(None, [], decode="device", midi=False) == [] == streaming.transcripts(None, [])

    class NotLive:
        live = False

    for decode in ("host", "device"):
        with pytest.raises(ValueError, match="live=True"):
            streaming.transcripts(None, [NotLive()], decode=decode)
