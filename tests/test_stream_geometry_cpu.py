"""Streaming sessions, the part that needs no GPU: when rows are final (`bp_stream_rows_after`) and that the header's
prototypes and the Python bindings agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HOP, WIN, LEAD = 36164, 43844, 3840
FIRST = WIN - LEAD  # 40004: the signal length that completes window 0


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, streaming

    build.build_library()
    return streaming.bind(_native.load_library())


def _lengths():
    rng = np.random.default_rng(20)
    ns = list(range(0, 3 * HOP + WIN + 1))
    big = [int(v) for v in rng.integers(3 * HOP + WIN, 400_000_000, 300)]
    for w in [int(v) for v in rng.integers(4, 10_000, 100)] + [4, 5, 1000, 11061]:
        big += [w * HOP - 1, w * HOP, w * HOP + 1, w * HOP + FIRST - 1, w * HOP + FIRST, w * HOP + FIRST + 1]
    big += [FIRST - 1, FIRST, FIRST + 1]
    return ns, sorted(set(big))


def test_rows_after_is_the_count_of_complete_windows_and_never_passes_the_final_count(lib):
    """Before finish a stream has emitted 142 rows per COMPLETE window (w * 36164 + 40004 <= n); that count is monotone and
    never exceeds bp_track_n_frames(n), the row count of the one-shot call on the signal so far — rows can therefore
    leave before the length is known (it follows from 40004 > 36164: w complete windows need more than w hops of signal,
    and int(n / 36164 * 142) >= 142 w then).  After finish the count IS bp_track_n_frames(n)."""
    dense, sparse = _lengths()
    for ns in (dense, sparse):
        prev = 0
        for n in ns:
            got = lib.bp_stream_rows_after(n, 0)
            if n <= 3 * HOP + WIN:
                complete = sum(1 for w in range(5) if w * HOP + FIRST <= n)  # the definition, window by window
            else:  # the last window that fits and the first that does not
                complete = (n - FIRST) // HOP + 1
                assert (complete - 1) * HOP + FIRST <= n < complete * HOP + FIRST, n
            assert got == 142 * complete, n
            assert got % 142 == 0 and got >= prev, n
            final = lib.bp_track_n_frames(n)
            assert got <= final, (n, got, final)
            assert lib.bp_stream_rows_after(n, 1) == final, n
            prev = got
    assert lib.bp_stream_rows_after(FIRST - 1, 0) == 0 and lib.bp_stream_rows_after(FIRST, 0) == 142
    assert lib.bp_stream_rows_after(HOP + FIRST, 0) == 284
    assert lib.bp_stream_rows_after(-5, 0) == 0 and lib.bp_stream_rows_after(-5, 1) == 0


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "bp_stream": C.c_void_p}


def _ctype_of(param: str):
    """The ctypes type of one C parameter of the streaming family: handles and plain data pointers are void pointers,
    `int64_t*` a pointer to int64, pointers to pointers (and the stream handle's out-parameter / array) pointers to void
    pointers."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    words = [w for w in words if w != "*"]
    base = words[0]
    if stars == 0:
        return _SCALAR[base]
    if base in ("bp_stream", "bp_handle") or stars == 2:
        assert stars <= 2 and (stars == 1 or base in ("void", "float")), param
        return C.POINTER(C.c_void_p)
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_header_and_bindings_declare_the_same_prototypes(lib):
    from basic_pitch_amd import _native, streaming

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef\s+struct\s+bp_stream_state\s*\*\s*bp_stream\s*;", header)
    protos = re.findall(r"\b(void|int|int64_t)\s+(bp_streams?_[a-z_]+)\s*\(([^)]*)\)\s*;", header)
    found = {}
    for ret, name, params in protos:
        args = [_ctype_of(p.strip()) for p in params.split(",")]
        found[name] = (None if ret == "void" else _SCALAR[ret], args)
    assert set(found) == set(streaming.PROTOTYPES) == {s for s in _native.EXPORTED_SYMBOLS if s.startswith("bp_stream")}
    assert len(found) == 8
    for name, (restype, argtypes) in found.items():
        assert streaming.PROTOTYPES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
