"""The melody decode, the part that needs no GPU (include/basic_pitch_amd_melody.h): the header's symbols are exported by both
libraries with the prototypes it declares, the structures are the bytes it says, and the two host checkers — bp_melody_rows and
bp_score_melody_frames — give what an independent restatement gives (tests/melody_cases.py: numpy float32 one operation at a
time, the refinement in float64, and every path of small quantised problems enumerated) on seeded maps and on crafted ones;
the checkers' source runs clean under the host sanitizers as a program of its own.  The calls that take a handle are in
tests/test_gpu_melody.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import melody_cases as MC
from conftest import ROOT

NEW = ("bp_melody_params_default", "bp_melody_rows", "bp_score_melody_frames", "bp_melody_from_maps", "bp_infer_clips_melody",
       "bp_melody_sweep_score", "bp_infer_clips_melody_sweep_score")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, melody

    build.build_library()
    return melody.bind(_native.load_library())


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "void": None}


def _ctype_of(param):
    """The rule of tests/test_score_cpu.py: handles and plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def _header():
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_melody.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- header and ABI
def test_every_symbol_of_the_melody_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, melody
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_multipitch.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(melody.PROTOTYPES) == set(_native.MELODY_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert melody.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    out = ["p", "points", "max_points", "status"]
    tail = ["n_sets", "sets", "n_decodes", "decodes", "ref_pitch", "score_params", "scores", "status"]
    assert names("bp_melody_rows") == ["contour", "rows", "p", "points", "max_points", "status"]
    assert names("bp_score_melody_frames") == ["est", "ref_pitch", "n_frames", "p", "out"]
    assert names("bp_melody_from_maps") == ["h", "n_segments", "row_offsets", "contour", "mem_kind"] + out
    assert names("bp_infer_clips_melody") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + out
    assert names("bp_melody_sweep_score") == ["h", "n_segments", "row_offsets", "contour", "mem_kind"] + tail
    assert names("bp_infer_clips_melody_sweep_score") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    # the statements the header owes: unpinned twice (the tracker, mir_eval), the recurrence lines, the figures
    flat = " ".join(text.replace("*", " ").split())
    assert flat.count("UNPINNED") >= 2 and "mir_eval.melody" in flat
    for said in ("pen[d] = jump_penalty (float)d", "D[0][s] = e[0][s]", "P[s] = D[t-1][s] - D[t-1][U]", "P[b'] - pen[|b - b'|]",
                 "P[U] - voicing_penalty", "P[b'] - voicing_penalty", "strictly greater than all before it",
                 "TIES GO TO THE LOWEST BIN, AND TO U LAST", "D[t][s] = e[t][s] + best", "first maximum of D[rows-1] in state order",
                 "RECORD r OF A SEGMENT IS ROW r", "pitch_midi = 21.0 + ((double)bin + delta) / 3.0",
                 "delta = 0.5 (l - r) / ((l - 2.0 c) + r)", "magnitude above 65536", "Hz are NOT produced",
                 "ONE workgroup barrier per frame", "2.3 GB", "37,788 bytes", "52 bytes per decode"):
        assert said in flat, said
    for macro, value in (("BP_MELODY_MAX_JUMP", melody.MAX_JUMP), ("BP_MELODY_READ_AHEAD", melody.READ_AHEAD),
                         ("BP_MELODY_TILE_ROWS", melody.TILE_ROWS), ("BP_MELODY_PRED_STRIDE", melody.PRED_STRIDE)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert (melody.MAX_JUMP, melody.PRED_STRIDE) == (16, 272)
    assert 2 * 296 * 4 + 2 * 5 * 8 + melody.TILE_ROWS * melody.PRED_STRIDE + melody.TILE_ROWS * 2 + 5 * 5 * 8 + (melody.MAX_JUMP + 1) * 4 == 37788
    assert round(8388608 * melody.PRED_STRIDE / 1e9, 1) == 2.3
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.MULTIPITCH_SYMBOLS) | set(_native.FRAME_SCORE_SYMBOLS) | set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | \
        set(_native.EVENTS_SYMBOLS) | set(_native.EXPORTED_SYMBOLS) | set(_native.FLAC_CLIPS_SYMBOLS)
    assert not set(NEW) & old
    assert os.path.basename(build.MELODY_HEADER) == "basic_pitch_amd_melody.h" and build.MELODY_HEADER in build.HEADERS
    assert {"melody.hip", "melody_host.cpp"} <= set(build.SOURCES)
    for entry in ("melody", "transcribe_clips_melody", "sweep_melody_scores", "transcribe_clips_sweep_melody_scores"):
        assert hasattr(Model, entry), entry
    unpinned = open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()
    assert "basic_pitch_amd_melody.h" in unpinned and "mir_eval.melody" in unpinned


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, melody

    text, header = _header()
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double, "int64_t": C.c_int64}
    for name, size in (("bp_melody_params", 32), ("bp_melody_point", 16), ("bp_melody_score", 48)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = []
        for t, decl in re.findall(r"\b(float|int32_t|double|int64_t)\s+([a-z_0-9, \[\]]+);", body):
            for n in decl.split(","):
                arr = re.fullmatch(r"\s*([a-z_]+)\[(\d+)\]\s*", n)
                fields.append((arr.group(1), ctype[t] * int(arr.group(2))) if arr else (n.strip(), ctype[t]))
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, (name, fields)
        assert f"/* {size} bytes */" in text
    assert melody.MELODY_POINT.itemsize == 16 and [melody.MELODY_POINT.fields[n][1] for n in melody.MELODY_POINT.names] == [0, 4, 8]
    assert melody.MELODY_POINT == MC.POINT
    p = melody.melody_params()
    assert (p.threshold, p.jump_penalty, p.voicing_penalty) == (np.float32(0.3), np.float32(0.05), np.float32(0.5))
    assert (p.max_jump, p.min_bin, p.max_bin, p.reserved[0], p.reserved[1]) == (4, 0, 263, 0, 0)
    assert MC.DEFAULT == dict(threshold=0.3, jump_penalty=0.05, voicing_penalty=0.5, max_jump=4, min_bin=0, max_bin=263)


# ---- bp_melody_rows against the restatement
def _same(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    assert got.tobytes() == want.tobytes(), where  # bin, salience and pitch_midi as bits


@pytest.fixture(scope="module")
def references():
    """{(rows, kind, set index): (map, records, status)} of the restatement, made once."""
    out = {}
    for rows in MC.ROWS:
        for kind, c in MC.case_maps(rows):
            for k, s in enumerate(MC.SETS):
                out[rows, kind, k] = (c,) + MC.restate(c, **s)
    return out


def test_the_reference_alone_meets_its_conditions(references):
    """Jumps of every size 0 ... max_jump; every set of the sweep has a segment with at least 10 % voiced and 10 % unvoiced
    frames; the quantised map's path differs from the path under the opposite tie-break."""
    assert [s.get("max_jump", 4) for s in MC.SETS[:4]] == [4, 0, 1, 16]
    assert any(s.get("min_bin") == s.get("max_bin") for s in MC.SETS if "min_bin" in s)
    assert any(s.get("min_bin") == 0 for s in MC.SETS) and any(s.get("max_bin") == 263 and "min_bin" in s for s in MC.SETS)
    for k, s in enumerate(MC.SETS):
        jumps, mixed = set(), False
        for (rows, kind, kk), (c, rec, status) in references.items():
            if kk != k or rows < 173:
                continue
            assert status == 0
            b = rec["bin"]
            v = b >= 0
            jumps |= set(np.abs(np.diff(b))[v[1:] & v[:-1]].tolist())
            mixed = mixed or 0.1 <= v.mean() <= 0.9
        width = MC.params(**s)["max_bin"] - MC.params(**s)["min_bin"]
        assert jumps == set(range(min(MC.params(**s)["max_jump"], width) + 1)), (k, sorted(jumps))
        assert mixed, k
    for rows in (173, 433):
        c = dict(MC.case_maps(rows))["quantised"]
        low, high = MC.restate_path(c, **MC.QUANTISED)[0], MC.restate_path(c, tie="high", **MC.QUANTISED)[0]
        assert (low != high).sum() >= 1, rows


def test_the_rows_checker_equals_the_restatement_as_bytes(lib, references):
    from basic_pitch_amd import melody

    voiced = 0
    for (rows, kind, k), (c, want, status) in references.items():
        got, got_status = melody.melody_rows(c, MC.params(**MC.SETS[k]))
        assert got_status == status == 0
        _same(got, want, (rows, kind, k))
        voiced += int((got["bin"] >= 0).sum())
    assert voiced > 10000


def test_the_returned_path_is_an_optimum_over_all_paths(lib):
    """Cells and parameters in eighths, a band of at most 4 bins, at most 5 rows: every float32 sum is exact, and the total of
    the checker's path equals the largest total over ALL paths, enumerated."""
    from basic_pitch_amd import melody

    rng = np.random.default_rng(11)
    seen_voiced = seen_unvoiced = 0
    for k in range(60):
        rows, lo = int(rng.integers(1, 6)), int(rng.choice([0, 100, 260]))
        width = int(rng.integers(1, 5))
        c = (rng.integers(0, 9, (rows, 264)) / 8.0).astype(np.float32)
        prm = dict(threshold=float(rng.integers(2, 8)) / 8.0, jump_penalty=float(rng.integers(0, 3)) / 8.0,
                   voicing_penalty=float(rng.integers(0, 4)) / 8.0, max_jump=int(rng.integers(0, 4)), min_bin=lo, max_bin=lo + width - 1)
        got, status = melody.melody_rows(c, MC.params(**prm))
        assert status == 0
        total = MC.path_total(c, got["bin"].tolist(), **prm)
        assert total is not None and total == MC.best_total_by_enumeration(c, **prm), (k, prm)
        _same(got, MC.restate(c, **prm)[0], k)
        seen_voiced += int((got["bin"] >= 0).sum())
        seen_unvoiced += int((got["bin"] < 0).sum())
    assert seen_voiced > 30 and seen_unvoiced > 30


def test_the_crafted_maps_say_what_they_were_made_to_say(lib):
    from basic_pitch_amd import melody

    zero = np.zeros((12, 264), np.float32)
    for threshold, bins in ((0.0, 50), (0.1, -1), (-0.1, 50)):
        got, status = melody.melody_rows(zero, MC.params(threshold=threshold, min_bin=50, max_bin=90))
        assert status == 0 and got["bin"].tolist() == [bins] * 12, threshold  # ties: the lowest bin, and U last
        _same(got, MC.restate(zero, threshold=threshold, min_bin=50, max_bin=90)[0], threshold)
    assert np.all(melody.melody_rows(zero, MC.params(threshold=0.0))[0]["pitch_midi"] == 21.0)
    # a voice that leaps max_jump + 1 bins: the path cannot follow in one step
    leap = np.zeros((20, 264), np.float32)
    leap[:10, 100], leap[10:, 105] = 0.9, 0.9
    got, _ = melody.melody_rows(leap, MC.params())
    steps = np.diff(got["bin"])
    assert got["bin"][0] == 100 and got["bin"][-1] == 105 and np.all(got["bin"] >= 0) and np.abs(steps).max() <= 4 and (steps != 0).sum() >= 2
    _same(got, MC.restate(leap)[0], "leap")
    got5, _ = melody.melody_rows(leap, MC.params(max_jump=5))
    assert (np.diff(got5["bin"]) != 0).sum() == 1 and np.abs(np.diff(got5["bin"])).max() == 5
    # a path on a shoulder (the one-bin band beside a peak) and on bins 0 / 263: delta 0
    hill = np.zeros((6, 264), np.float32)
    hill[:, 119:122] = (0.5, 0.9, 0.6)
    hill[:, 0], hill[:, 263] = 0.8, 0.7
    for b in (119, 121, 0, 263):
        got, _ = melody.melody_rows(hill, MC.params(min_bin=b, max_bin=b))
        assert got["bin"].tolist() == [b] * 6 and np.all(got["pitch_midi"] == 21.0 + np.float64(b) / 3.0), b
        assert np.all(got["salience"] == hill[0, b])
    got, _ = melody.melody_rows(hill, MC.params(min_bin=100, max_bin=140))
    assert got["bin"].tolist() == [120] * 6 and np.all(got["pitch_midi"] != 61.0)
    # delta near +0.5 and -0.5
    skew = np.zeros((4, 264), np.float32)
    skew[:, 119:122] = (0.001, 0.75, np.nextafter(np.float32(0.75), np.float32(0)))
    got, _ = melody.melody_rows(skew, MC.params())
    delta = (got["pitch_midi"] - 21.0) * 3.0 - 120.0
    assert got["bin"].tolist() == [120] * 4 and np.all((0.49 < delta) & (delta <= 0.5)), delta
    got, _ = melody.melody_rows(skew[:, ::-1].copy(), MC.params())
    delta = (got["pitch_midi"] - 21.0) * 3.0 - 143.0
    assert got["bin"].tolist() == [143] * 4 and np.all((-0.5 <= delta) & (delta < -0.49)), delta
    _same(got, MC.restate(skew[:, ::-1].copy())[0], "skew")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 65537.0, -65537.0])
def test_a_cell_out_of_range_outside_the_band_gives_status_1_and_unvoiced_records(lib, value):
    from basic_pitch_amd import melody

    c = dict(MC.case_maps(65))["glide"]
    prm = MC.params(min_bin=30, max_bin=230)
    assert (melody.melody_rows(c, prm)[0]["bin"] >= 0).any()
    for row, bin_ in ((0, 0), (64, 263), (7, 29), (11, 231), (30, 100)):  # the last inside the band
        bad = MC.with_cell(c, value, row, bin_)
        got, status = melody.melody_rows(bad, prm)
        assert status == 1 and MC.restate(bad, **prm)[1] == 1
        _same(got, MC.records(bad, np.full(65, -1)), (value, row, bin_))
    for edge in (65536.0, -65536.0):
        ok = MC.with_cell(c, edge, 7, 29)
        got, status = melody.melody_rows(ok, prm)
        assert status == 0
        _same(got, MC.restate(ok, **prm)[0], edge)


@pytest.mark.parametrize("fields, named", [
    (dict(threshold=np.nan), "threshold"), (dict(threshold=np.inf), "threshold"), (dict(threshold=65537.0), "threshold"),
    (dict(threshold=-65537.0), "threshold"), (dict(jump_penalty=np.nan), "jump_penalty"), (dict(jump_penalty=-0.125), "jump_penalty"),
    (dict(jump_penalty=65537.0), "jump_penalty"), (dict(voicing_penalty=np.inf), "voicing_penalty"),
    (dict(voicing_penalty=-1.0), "voicing_penalty"), (dict(voicing_penalty=1e9), "voicing_penalty"), (dict(max_jump=-1), "max_jump"),
    (dict(max_jump=17), "max_jump"), (dict(min_bin=-1), "min_bin"), (dict(max_bin=264), "max_bin"),
    (dict(min_bin=120, max_bin=119), "min_bin"), (dict(reserved=1), "reserved"), (dict(reserved=(0, 1)), "reserved"),
])
def test_every_malformed_parameter_set_is_refused_by_name(lib, fields, named):
    from basic_pitch_amd import melody

    p = melody.melody_params(**fields)
    lib.bp_internal_melody_bad_params.restype, lib.bp_internal_melody_bad_params.argtypes = C.c_char_p, [C.c_void_p]
    why = lib.bp_internal_melody_bad_params(C.addressof(p))
    assert why and named in why.decode(), (fields, why)
    c = dict(MC.case_maps(2))["noise"]
    status = C.c_int(-7)
    buf = np.zeros(2, MC.POINT)
    buf.view(np.uint8)[:] = 0x5A
    assert lib.bp_melody_rows(c.ctypes.data, 2, C.addressof(p), buf.ctypes.data, 2, C.byref(status)) == -1
    assert np.all(buf.view(np.uint8) == 0x5A) and status.value == -7
    for fine in (dict(), dict(threshold=65536.0), dict(threshold=-65536.0), dict(jump_penalty=0.0, voicing_penalty=65536.0), dict(max_jump=16)):
        assert lib.bp_internal_melody_bad_params(C.addressof(melody.melody_params(**fine))) is None
    with pytest.raises(ValueError, match="bp_melody_params"):
        melody.melody_rows(c, p)
    with pytest.raises(TypeError, match="unknown field"):
        melody.melody_params(treshold=0.1)


def test_the_other_bad_arguments_of_the_rows_checker_are_refused(lib):
    from basic_pitch_amd import melody

    p = melody.melody_params()
    c = dict(MC.case_maps(2))["noise"]
    status = C.c_int(0)
    buf = np.zeros(4, MC.POINT)
    buf.view(np.uint8)[:] = 0x5A
    args = lambda **kw: [kw.get("c", c.ctypes.data), kw.get("rows", 2), kw.get("p", C.addressof(p)), kw.get("pts", buf.ctypes.data),  # noqa: E731
                         kw.get("room", 2), kw.get("st", C.byref(status))]
    for bad in (dict(c=None), dict(rows=-1), dict(p=None), dict(pts=None), dict(room=1), dict(room=-1), dict(st=None)):
        assert lib.bp_melody_rows(*args(**bad)) == -1, bad
        assert np.all(buf.view(np.uint8) == 0x5A), bad  # one record short of the rows: refused, and nothing is written
    assert lib.bp_melody_rows(*args(c=None, rows=0, pts=None, room=0)) == 0 and status.value == 0
    assert lib.bp_melody_rows(*args(room=4)) == 0 and np.all(buf[2:].view(np.uint8) == 0x5A)


# ---- bp_score_melody_frames against the restatement
def _track(bins):
    """Records on bin centres: pitch 21 + bin / 3 (exact for multiples of three), -1 unvoiced."""
    rec = np.zeros(len(bins), MC.POINT)
    rec["bin"] = bins
    voiced = rec["bin"] >= 0
    rec["salience"][voiced] = 0.5
    rec["pitch_midi"][voiced] = 21.0 + rec["bin"][voiced] / 3.0
    return rec


def test_the_counts_equal_the_restatement_on_seeded_tracks(lib):
    from basic_pitch_amd import melody

    rng = np.random.default_rng(4)
    seen = np.zeros(6, np.int64)
    strict_matters = 0
    for k in range(120):
        rows = int(rng.choice([1, 40, 173]))
        c = MC.case_maps(rows, seed=k % 5)[k % 3][1]
        points = MC.restate(c, **MC.SETS[k % len(MC.SETS)])[0]
        ref = MC.ref_for(rng, points)
        tol = dict(pitch_tolerance_cents=float(rng.choice([0.0, 30.0, 50.0, 100.0])), strict=int(rng.integers(0, 2)))
        want = MC.restate_counts(points, ref, **tol)
        got = melody.score_melody_frames(points, ref, **tol)
        assert tuple(int(got[f]) for f in melody._FIELDS) == want and int(got["status"]) == 0, (k, got, want, tol)
        seen += np.array(want) > 0
        assert want[5] >= want[4] and want[3] >= want[5] and min(want[1], want[2]) >= want[3]
        if tol["pitch_tolerance_cents"] == 50.0:
            strict_matters += MC.restate_counts(points, ref, pitch_tolerance_cents=50.0, strict=1 - tol["strict"]) != want
    assert min(seen) > 40, seen  # (the reference is not trivial: every count is exercised by many cases)
    assert strict_matters > 0


def test_octaves_the_exact_tolerance_unvoiced_references_and_zero_frames(lib):
    from basic_pitch_amd import melody

    est = _track([30, 30, 30, 30, -1, -1, 66, 66])  # MIDI 31 and 43
    count = lambda ref, **tol: tuple(int(melody.score_melody_frames(est, ref, **tol)[f]) for f in melody._FIELDS)  # noqa: E731
    # exactly 12 and 24 semitones off: chroma yes, pitch no
    assert count([43.0, 19.0, 55.0, 31.0, 0.0, 50.0, 43.0, 0.0]) == (8, 6, 6, 5, 2, 5)
    # exactly at the tolerance (half a semitone, both sides; 50.0 cents exactly in float64), strict and not
    ref = [31.5, 30.5, 43.5, 31.0, 0.0, 0.0, 43.0, 42.5]
    assert count(ref) == (8, 6, 6, 6, 5, 6) and count(ref, strict=1) == (8, 6, 6, 6, 2, 2)
    assert count(ref, pitch_tolerance_cents=49.0) == (8, 6, 6, 6, 2, 2) and count(ref, pitch_tolerance_cents=1200.0)[4:] == (5, 6)  # (43.5 against 31 is 1,250 cents)
    assert count(np.zeros(8)) == (8, 0, 6, 0, 0, 0)
    none = melody.score_melody_frames(np.zeros(0, MC.POINT), np.zeros(0))
    assert tuple(int(none[f]) for f in melody._FIELDS) == (0, 0, 0, 0, 0, 0)
    # the refusals
    for bad in (-1.0, np.nan, np.inf):
        ref = np.zeros(8)
        ref[5] = bad
        with pytest.raises(ValueError, match="ref_pitch"):
            melody.score_melody_frames(est, ref)
    broken = est.copy()
    broken["pitch_midi"][1] = np.nan
    with pytest.raises(ValueError):
        melody.score_melody_frames(broken, np.zeros(8))
    broken["bin"][1] = -1  # an unvoiced record's pitch is not read
    assert int(melody.score_melody_frames(broken, np.zeros(8))["est_voiced"]) == 5
    for tol in (dict(pitch_tolerance_cents=-1.0), dict(pitch_tolerance_cents=np.nan), dict(reserved=1)):
        with pytest.raises(ValueError):
            melody.score_melody_frames(est, np.zeros(8), **tol)
    with pytest.raises(ValueError, match="one entry per row"):
        melody.score_melody_frames(est, np.zeros(7))
    lib.bp_internal_melody_bad_ref.restype, lib.bp_internal_melody_bad_ref.argtypes = C.c_int64, [C.c_void_p, C.c_int64]
    ref = np.array([0.0, 60.0, -0.5, np.nan])
    assert lib.bp_internal_melody_bad_ref(ref.ctypes.data, 4) == 2 and lib.bp_internal_melody_bad_ref(ref.ctypes.data, 2) == -1


def test_the_measures_follow_from_the_counts(lib):
    from basic_pitch_amd import melody

    counts = np.zeros(3, melody.MELODY_COUNTS)
    counts[0] = (100, 60, 50, 40, 30, 35, 0)
    counts[1] = (10, 0, 0, 0, 0, 0, 0)   # nothing voiced on either side: every frame is right
    counts[2] = (0, 0, 0, 0, 0, 0, 0)    # no frames: every denominator is zero
    m = melody.measures(counts)
    assert set(m) == {"voicing_recall", "voicing_false_alarm", "raw_pitch_accuracy", "raw_chroma_accuracy", "overall_accuracy"}
    assert m["voicing_recall"].tolist() == [40 / 60, 0.0, 0.0] and m["voicing_false_alarm"].tolist() == [10 / 40, 0.0, 0.0]
    assert m["raw_pitch_accuracy"].tolist() == [30 / 60, 0.0, 0.0] and m["raw_chroma_accuracy"].tolist() == [35 / 60, 0.0, 0.0]
    assert m["overall_accuracy"].tolist() == [(30 + 100 - 60 - 50 + 40) / 100, 1.0, 0.0]
    assert melody.measures(counts.reshape(3, 1))["overall_accuracy"].shape == (3, 1)
    assert float(melody.measures(counts[0])["voicing_recall"]) == 40 / 60


def test_ref_track_takes_the_nearest_sample_with_ties_to_the_earlier_one(lib):
    from basic_pitch_amd import melody
    from basic_pitch_amd.note_creation import model_frames_to_time

    at = model_frames_to_time(6)
    assert at[0] == 0.0 and np.all(np.diff(at) > 0)
    # a sample on frame 0, one a quarter of a step before frame 2 and a non-positive one a quarter after it, one far behind
    step = at[2] - at[1]
    times = np.array([at[0], at[2] - 0.25 * step, at[3] + 0.25 * step, at[5] + 1.0])
    ref = melody.ref_track(times, np.array([440.0, 220.0, -1.0, 880.0]), 6)
    assert ref.tolist() == [69.0, 57.0, 57.0, 0.0, 0.0, 0.0]  # frame 1 is nearer the second sample; <= 0 Hz is unvoiced: 0.0
    # frame 3 is exactly between the two samples (2 * at[3] is exact): the tie goes to the earlier one
    ties = melody.ref_track(np.array([0.0, 2.0 * at[3]]), np.array([440.0, 880.0]), 6)
    assert ties.tolist() == [69.0, 69.0, 69.0, 69.0, 81.0, 81.0]
    assert melody.ref_track(np.array([0.0]), np.array([0.0]), 4).tolist() == [0.0] * 4
    assert melody.ref_track(np.array([1.0]), np.array([220.0]), 3).tolist() == [57.0] * 3
    assert melody.ref_track(np.zeros(0), np.zeros(0), 3).tolist() == [0.0] * 3 and len(melody.ref_track([0.0], [1.0], 0)) == 0
    with pytest.raises(ValueError):
        melody.ref_track([0.0, 1.0], [440.0], 3)
    with pytest.raises(ValueError):
        melody.ref_track([1.0, 0.0], [440.0, 440.0], 3)


def test_the_python_result_follows_from_the_records(lib):
    from basic_pitch_amd import melody
    from basic_pitch_amd.note_creation import model_frames_to_time

    c = dict(MC.case_maps(433))["glide"]
    points, status = melody.melody_rows(c)
    est = melody.Melody.from_points(points, status)
    assert np.array_equal(est.times_s, model_frames_to_time(433)) and np.array_equal(est.voiced, est.bins >= 0)
    assert 0.1 < est.voiced.mean() < 0.9
    assert np.array_equal(est.freqs_hz[est.voiced], 440.0 * np.exp2((est.pitch_midi[est.voiced] - 69.0) / 12.0))
    assert np.all(est.freqs_hz[~est.voiced] == 0.0) and np.all(est.pitch_midi[~est.voiced] == 0.0) and np.all(est.salience[~est.voiced] == 0.0)
    assert est.salience.dtype == np.float32 and est.bins.dtype == np.int32 and est.status == 0
    assert np.array_equal(est.salience[est.voiced], c[np.flatnonzero(est.voiced), est.bins[est.voiced]])


# ---- the source alone, under the host sanitizers
def test_the_checkers_link_without_a_device_and_run_clean_under_the_sanitizers(tmp_path):
    """tests/test_multipitch_cpu.py's pattern: the checkers' source with the device-free sources it calls into and
    tools/sanitize/melody_host.cpp, plain g++, once with -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    csrc = os.path.join(ROOT, "basic_pitch_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", "sanitize", "melody_host.cpp")] + \
        [os.path.join(csrc, s) for s in ("melody_host.cpp", "note_frames_host.cpp", "note_score_host.cpp", "note_decode.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"melody_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("melody 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["voiced"]) > 2000 and int(sums["unvoiced"]) > 2000 and int(sums["jumps"]) > 500 and int(sums["flagged"]) > 0
    assert int(sums["refused"]) >= 500 and int(sums["pitch_ok"]) > 0 and int(sums["chroma_ok"]) > int(sums["pitch_ok"])
