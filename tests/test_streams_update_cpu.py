"""The many-stream update, the part that needs no GPU: the calls of include/basic_pitch_amd_update.h are exported with the
prototypes that header declares, `bp_stream_update` in ctypes has the header's fields in the header's order, the scatter of
packed rows into a transcriber's host arrays, and `transcripts` of no transcriber."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("bp_streams_update_layout", "bp_streams_candidates")
_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "bp_stream": C.c_void_p}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basic_pitch_amd_update.h")).read(), flags=re.S)


def _ctype_of(param: str):
    """The rule of tests/test_stream_rolling_cpu.py: plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_the_new_calls_are_exported_with_the_headers_prototypes():
    from basic_pitch_amd import _native, build, streaming

    build.build_library()
    lib = streaming.bind(_native.load_library())
    header = _header()
    assert '#include "basic_pitch_amd_rolling.h"' in header
    protos = {name: (ret, params) for ret, name, params in re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(streaming.UPDATE_PROTOTYPES) == set(_native.UPDATE_SYMBOLS)
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert streaming.UPDATE_PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    assert names("bp_streams_update_layout") == ["h", "n", "u", "with_tail", "note_rows", "bits_rows"]
    assert names("bp_streams_candidates") == ["h", "n", "u", "with_tail", "note_out", "bend_out", "bits_out", "note_capacity_rows",
                                              "bits_capacity_rows"]
    assert not set(NEW) & (set(_native.EXPORTED_SYMBOLS) | set(_native.LIVE_SYMBOLS) | set(_native.ROLLING_SYMBOLS))
    assert os.path.basename(build.UPDATE_HEADER) in [os.path.basename(h) for h in build.HEADERS]


def test_the_ctypes_struct_has_the_headers_fields_in_the_headers_order():
    from basic_pitch_amd import _native

    body = re.search(r"typedef struct bp_stream_update \{(.*?)\} bp_stream_update;", _header(), flags=re.S).group(1)
    fields = [tuple(f.split()) for f in body.split(";") if f.strip()]
    ctypes_of = {"bp_stream": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int}
    assert [(name, ctypes_of[t]) for t, name in fields] == list(_native.bp_stream_update._fields_)
    assert [name for _, name in fields] == ["stream", "held_rows", "first_row", "n_rows", "new_row", "note_offset", "bits_offset", "status"]
    # a pointer, six int64 and an int, padded to the pointer's alignment: what a C compiler lays out on this ABI
    assert C.sizeof(_native.bp_stream_update) == 64 and _native.bp_stream_update.status.offset == 56
    assert [getattr(_native.bp_stream_update, n).offset for n, _ in _native.bp_stream_update._fields_] == list(range(0, 64, 8))


@pytest.mark.parametrize("ring_rows, r0, r1", [
    (2000, 0, 700), (2000, 123, 700), (2000, 700, 700),  # linear: an array that never wraps
    (457, 0, 300), (457, 100, 457), (457, 460, 900),     # a ring, the rows inside one lap
    (457, 300, 600), (457, 456, 458), (457, 900, 1357), (457, 5000 - 173, 5000 + 284),  # rows that wrap
])
def test_packed_rows_are_scattered_to_their_slots(ring_rows, r0, r1):
    from basic_pitch_amd import streaming

    rng = np.random.default_rng(r0 + r1)
    for width, dtype in ((88, np.float32), (12, np.uint8), (88, np.int8)):
        packed = rng.integers(1, 100, (r1 - r0, width)).astype(dtype)
        ring = np.zeros((ring_rows, width), dtype)
        want = ring.copy()
        want[np.arange(r0, r1) % ring_rows] = packed
        streaming.scatter_rows(ring, packed, r0, r1)
        assert np.array_equal(ring, want)
        assert np.array_equal(ring[np.arange(r0, r1) % ring_rows], packed)


def test_transcripts_of_no_transcriber():
    from basic_pitch_amd import streaming

    assert streaming.transcripts(None, []) == []  # no model is looked at
    import basic_pitch_amd

    assert basic_pitch_amd.transcripts is streaming.transcripts and hasattr(basic_pitch_amd.Model, "transcripts")
