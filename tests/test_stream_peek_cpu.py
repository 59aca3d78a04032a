"""Peek and live transcripts, the part that needs no GPU: the calls of include/basic_pitch_amd_live.h are exported with the
prototypes that header declares (the comparison tests/test_stream_geometry_cpu.py makes for the family of
include/basic_pitch_amd.h, which stays the eight calls it pins), and the row count of a peek follows from the two counts
`bp_stream_rows_after` already gives."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HOP, WIN, LEAD = 36164, 43844, 3840
NEW = ("bp_stream_peek", "bp_streams_peek", "bp_stream_keep", "bp_stream_candidates")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, streaming

    build.build_library()
    return streaming.bind(_native.load_library())


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "bp_stream": C.c_void_p}


def _ctype_of(param: str):
    """The ctypes type of one C parameter, by the rule tests/test_stream_geometry_cpu.py states for the family: handles and
    plain data pointers (structs, bytes, `int*` among them) are void pointers, `int64_t*` a pointer to int64, pointers to
    pointers and arrays of stream handles pointers to void pointers."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    if base in ("bp_stream", "bp_handle") or stars == 2:
        assert stars <= 2 and (stars == 1 or base in ("void", "float")), param
        return C.POINTER(C.c_void_p)
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_the_new_calls_are_exported_with_the_headers_prototypes(lib):
    from basic_pitch_amd import _native, streaming
    import basic_pitch_amd

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_live.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert '#include "basic_pitch_amd.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_streams?_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(streaming.LIVE_PROTOTYPES) == set(_native.LIVE_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (None if ret == "void" else _SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert streaming.LIVE_PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    # the parameter lists themselves, as the issue gives them
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    assert names("bp_stream_peek") == ["s", "note", "onset", "contour", "capacity_rows", "out_mem_kind", "rows"]
    assert names("bp_streams_peek") == ["h", "n", "streams", "note", "onset", "contour", "capacity_rows", "out_mem_kind", "rows"]
    assert names("bp_stream_keep") == ["s", "params", "max_rows"]
    assert names("bp_stream_candidates") == ["s", "with_tail", "note_out", "cand_bits", "bend_map", "first_row",
                                             "capacity_rows", "n_rows", "status"]
    for public in ("Stream", "StreamingTranscriber", "peek_streams", "push_streams"):
        assert hasattr(basic_pitch_amd, public), public
    assert hasattr(streaming.Stream, "peek") and hasattr(streaming.StreamingTranscriber, "transcript")


def _final_rows(n):
    """inference.py:207,242,277-279 restated: min(n_windows * 142, int(n / 36164 * 142))."""
    if n <= 0:
        return 0
    return min(-(-(n + LEAD) // HOP) * 142, int(n / HOP * 142))


def test_the_rows_of_a_peek_are_the_final_count_minus_the_emitted_count(lib):
    """A peek gives the rows a finish would: bp_stream_rows_after(n, 1) - bp_stream_rows_after(n, 0) for a model-rate signal
    of n samples (tests/test_gpu_stream_peek.py holds the device to this).  Both terms against the definitions; the
    difference is never negative and never more than the two windows the kept maps reserve behind their rows."""
    from basic_pitch_amd import _native

    for name in _native.LIVE_SYMBOLS:  # the geometry is that of calls this library has
        assert hasattr(lib, name), name
    assert "bp_stream_peek" in _native.LIVE_SYMBOLS
    expect = {0: 0, 1: 0, 40003: 157, 40004: 15, 40005: 15, 76168: 15, 120000: 45}
    for n, rows in expect.items():
        complete = 0 if n < WIN - LEAD else (n - (WIN - LEAD)) // HOP + 1
        assert lib.bp_stream_rows_after(n, 0) == 142 * complete, n
        assert lib.bp_stream_rows_after(n, 1) == _final_rows(n) == lib.bp_track_n_frames(n), n
        peek = lib.bp_stream_rows_after(n, 1) - lib.bp_stream_rows_after(n, 0)
        assert peek == rows and 0 <= peek <= 2 * 142, (n, peek)
    # 76168 = 36164 + 40004 completes window 1 exactly; one sample less leaves it, and nearly two windows, to the peek
    assert lib.bp_stream_rows_after(76167, 1) - lib.bp_stream_rows_after(76167, 0) == _final_rows(76167) - 142 == 157
