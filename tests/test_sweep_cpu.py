"""A sweep of parameter sets in one device call, the part that needs no GPU: the calls of include/basic_pitch_amd_sweep.h are
exported with the prototypes that header declares, the decode record is the 16 bytes the header says, the cross product is
listed set-major, and the sets group into dense keys as the native planner groups them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("bp_note_events_sweep", "bp_infer_clips_events_sweep")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, sweep

    build.build_library()
    return sweep.bind(_native.load_library())


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


def _header():
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_sweep.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_every_symbol_of_the_sweep_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, sweep
    from basic_pitch_amd.inference import Model

    _, header = _header()
    assert '#include "basic_pitch_amd_events.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(sweep.PROTOTYPES) == set(_native.SWEEP_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert sweep.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["n_sets", "sets", "n_decodes", "decodes", "events", "max_events", "bends", "max_bends", "event_offsets", "status"]
    assert names("bp_note_events_sweep") == ["h", "n_segments", "row_offsets", "note", "onset", "contour", "mem_kind"] + tail
    assert names("bp_infer_clips_events_sweep") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert re.search(r"#define BP_SWEEP_MAX_DECODES (\d+)", header).group(1) == str(sweep.MAX_DECODES) == "65536"
    assert re.search(r"#define BP_SWEEP_MAX_ROWS (\d+)", header).group(1) == str(sweep.MAX_ROWS)
    # the existing headers and lists are what they were, the new header is one the build watches
    assert not set(NEW) & (set(_native.EXPORTED_SYMBOLS) | set(_native.CLIPS_SYMBOLS) | set(_native.EVENTS_SYMBOLS))
    assert "basic_pitch_amd_sweep.h" in [os.path.basename(h) for h in build.HEADERS]
    assert hasattr(Model, "sweep_note_events") and hasattr(Model, "transcribe_clips_sweep")


def test_both_symbols_are_exported_by_both_libraries(lib):
    import subprocess

    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_decode_record_is_the_sixteen_bytes_the_header_declares():
    from basic_pitch_amd import _native, sweep

    text, header = _header()
    body = re.search(r"typedef struct bp_sweep_decode \{(.*?)\} bp_sweep_decode;", header, flags=re.S).group(1)
    fields = re.findall(r"\b(int64_t|int32_t)\s+([a-z_]+)\s*;", body)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_native.bp_sweep_decode._fields_)
    assert [n for _, n in fields] == ["segment", "params", "reserved"]
    assert C.sizeof(_native.bp_sweep_decode) == 16 and "16 bytes" in text
    tab = sweep.decode_table([(3, 1), (0, 2)])
    assert [(d.segment, d.params, d.reserved) for d in tab] == [(3, 1, 0), (0, 2, 0)]
    assert bytes(tab)[:16] == (3).to_bytes(8, "little") + (1).to_bytes(4, "little") + bytes(4)


def test_the_cross_product_is_set_major():
    from basic_pitch_amd import sweep

    pairs = sweep.cross_product(3, 4)
    assert len(pairs) == 12
    for p in range(3):
        for i in range(4):
            assert pairs[p * 4 + i] == (i, p)  # decode p * n_segments + i is segment i under set p
    assert sweep.cross_product(0, 5) == [] == sweep.cross_product(5, 0)


def _prm(**kw):
    from basic_pitch_amd import note_creation as NC

    return NC._note_params(kw.get("onset_thresh", 0.5), kw.get("frame_thresh", 0.3), kw.get("min_note_len", 11),
                           kw.get("infer_onsets", True), kw.get("max_freq"), kw.get("min_freq"), kw.get("melodia_trick", True),
                           kw.get("energy_tol", 11), kw.get("include_pitch_bends", True))


def test_sets_group_into_dense_keys(lib):
    from basic_pitch_amd import _native, sweep

    sets = [_prm(), _prm(frame_thresh=0.1, min_note_len=3, energy_tol=5, melodia_trick=False, include_pitch_bends=False),
            _prm(onset_thresh=0.6), _prm(min_freq=80.0), _prm(min_freq=80.0, frame_thresh=0.2), _prm(max_freq=1500.0),
            _prm(infer_onsets=False), _prm(onset_thresh=0.0), _prm(min_freq=80.0, max_freq=1500.0)]
    keys, of_set = sweep.dense_keys(sets)
    # 0.5 groups with 0.5 whatever the tracker's own parameters are; what the dense half reads separates
    assert of_set[0] == of_set[1] and of_set[3] == of_set[4]
    assert len({of_set[i] for i in (0, 2, 3, 5, 6, 8)}) == 6 == len(keys)
    assert of_set[7] is None  # an onset threshold of 0: no dense half
    assert keys == sorted(keys)  # by band: a band's keys are neighbours
    # sets that differ in min_freq only
    a, b = _prm(min_freq=80.0), _prm(min_freq=160.0)
    assert sweep.dense_key(a) != sweep.dense_key(b) and sweep.dense_key(a)[1:] == sweep.dense_key(b)[1:]
    assert sweep.dense_key(_prm()) == (0, 88, True, 0.5)
    # the bands are the native decoder's
    lib.bp_internal_freq_limits.restype, lib.bp_internal_freq_limits.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p]
    for lo_hz, hi_hz in ((None, None), (80.0, None), (None, 1500.0), (27.5, 4186.0), (20.0, 9000.0), (440.0, 440.0), (29.0, 30.0),
                         (1.0, 2.0), (3000.5, 123.4)):
        prm = _prm(min_freq=lo_hz, max_freq=hi_hz)
        lo, hi = C.c_int(-1), C.c_int(-1)
        lib.bp_internal_freq_limits(C.addressof(prm), C.addressof(lo), C.addressof(hi))
        assert sweep.freq_limits(prm) == (lo.value, hi.value), (lo_hz, hi_hz)
    arr = sweep.sets_array(sets)
    assert bytes(arr)[: C.sizeof(_native.bp_note_params)] == bytes(sets[0]) and arr[2].onset_threshold == 0.6


def test_a_null_handle_is_refused(lib):
    from basic_pitch_amd import _native

    offs = (C.c_int64 * 2)()
    st = (C.c_int * 1)()
    p_offs = C.cast(offs, C.POINTER(C.c_int64))
    assert lib.bp_note_events_sweep(None, 0, p_offs, None, None, None, 0, 0, None, 0, None, None, 0, None, 0, p_offs,
                                    C.addressof(st)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_clips_events_sweep(None, 0, None, 22050, 0, 0, None, 0, None, None, 0, None, 0, p_offs,
                                           C.addressof(st)) == _native.BP_ERR_INVALID_ARG
