"""Multi-pitch estimates, the part that needs no GPU (include/basic_pitch_amd_multipitch.h): the header's symbols are exported
by both libraries with the prototypes it declares, the structures are the bytes it says, and the two host checkers —
bp_multipitch_rows and bp_score_f0_frames — give what an independent restatement gives (tests/multipitch_cases.py:
scipy.signal.argrelmax, the refinement in numpy float64, scipy's maximum bipartite matching per frame) on seeded maps and on
crafted rows; the checker's source runs clean under the host sanitizers as a program of its own.  The calls that take a
handle are in tests/test_gpu_multipitch.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import multipitch_cases as MC
import score_cases as SC
from conftest import ROOT

NEW = ("bp_mp_params_default", "bp_multipitch_rows", "bp_score_f0_frames", "bp_multipitch_from_maps", "bp_infer_clips_multipitch",
       "bp_multipitch_sweep_frame_score", "bp_infer_clips_multipitch_sweep_frame_score")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, multipitch

    build.build_library()
    return multipitch.bind(_native.load_library())


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
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_multipitch.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- header and ABI
def test_every_symbol_of_the_multipitch_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, multipitch
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_frame_score.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(multipitch.PROTOTYPES) == set(_native.MULTIPITCH_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert multipitch.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    out = ["p", "points", "max_points", "point_offsets", "status"]
    tail = ["n_sets", "sets", "n_decodes", "decodes", "ref_offsets", "refs", "score_params", "frames", "status"]
    assert names("bp_multipitch_rows") == ["contour", "rows", "p", "points", "max_points", "n_points", "status"]
    assert names("bp_score_f0_frames") == ["est", "n_est", "ref", "n_ref", "n_frames", "p", "out"]
    assert names("bp_multipitch_from_maps") == ["h", "n_segments", "row_offsets", "contour", "mem_kind"] + out
    assert names("bp_infer_clips_multipitch") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + out
    assert names("bp_multipitch_sweep_frame_score") == ["h", "n_segments", "row_offsets", "contour", "mem_kind"] + tail
    assert names("bp_infer_clips_multipitch_sweep_frame_score") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    # the statements the header owes
    flat = " ".join(text.replace("*", " ").split())
    for said in ("UNPINNED", "scipy.signal.argrelmax", "AT MOST 131 PEAKS", "delta = 0.5 (l - r) / ((l - 2.0 c) + r)",
                 "pitch_midi = 21.0 + ((double)b + delta) / 3.0", "strictly ascending", "Hz are NOT produced", "THE ORDER IS PART OF THE CONTRACT",
                 "4,384 bytes", "44 bytes per decode"):
        assert said in flat, said
    assert int(re.search(r"#define BP_MP_SCAN_TILE_ROWS (\d+)", header).group(1)) == multipitch.SCAN_TILE_ROWS
    assert int(re.search(r"#define BP_MP_MAX_PEAKS_PER_ROW (\d+)", header).group(1)) == multipitch.MAX_PEAKS_PER_ROW == 131
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.FRAME_SCORE_SYMBOLS) | set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | \
        set(_native.EXPORTED_SYMBOLS)
    assert not set(NEW) & old
    assert "basic_pitch_amd_multipitch.h" in [os.path.basename(h) for h in build.HEADERS]
    assert {"multipitch.hip", "multipitch_host.cpp"} <= set(build.SOURCES)
    for entry in ("multipitch", "transcribe_clips_multipitch", "sweep_multipitch_frame_scores", "transcribe_clips_sweep_multipitch_frame_scores"):
        assert hasattr(Model, entry), entry
    assert "multipitch" in open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, multipitch

    text, header = _header()
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double}
    for name, size in (("bp_mp_params", 16), ("bp_f0_point", 16)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = [(n, ctype[t]) for t, n in re.findall(r"\b(float|int32_t|double)\s+([a-z_]+);", body)]
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, name
    assert text.count("16 bytes */") >= 2
    assert multipitch.F0_POINT.itemsize == 16 and [multipitch.F0_POINT.fields[n][1] for n in multipitch.F0_POINT.names] == [0, 4, 8]
    assert multipitch.F0_POINT == MC.POINT
    p = multipitch.mp_params()
    assert (p.threshold, p.min_bin, p.max_bin, p.reserved) == (np.float32(0.3), 1, 262, 0)


# ---- bp_multipitch_rows against the restatement
def _same_points(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    assert got.tobytes() == want.tobytes(), where  # frame, salience and pitch_midi as bits


@pytest.fixture(scope="module")
def case_maps():
    """The case maps with their names, made once: the segments of the GPU job (bumps, dense noise, the crafted rows)."""
    return [(f"segment of {len(c)} rows", c) for c in MC.segment_job()] + [("crafted", MC.crafted()[1])]


def test_the_rows_checker_equals_the_restatement_field_for_field(lib, case_maps):
    from basic_pitch_amd import multipitch

    n_points = 0
    for name, c in case_maps:
        for lo, hi in MC.BANDS:
            for threshold in (0.3, 0.0, -1.0, 0.8, 10.0):
                prm = MC.params(threshold=threshold, min_bin=lo, max_bin=hi)
                want, status, delta = MC.restate_points(c, **prm)
                got, got_status = multipitch.multipitch_rows(c, prm)
                assert got_status == status == 0
                _same_points(got, want, (name, prm))
                assert np.all(np.abs(delta) <= 0.5), (name, prm)
                same_frame = np.diff(got["frame"]) == 0
                assert np.all(np.diff(got["frame"]) >= 0) and np.all(np.diff(got["pitch_midi"])[same_frame] > 0), (name, prm)
                n_points += len(got)
    assert n_points > 100000


def test_the_crafted_rows_say_what_they_were_made_to_say(lib):
    from basic_pitch_amd import multipitch

    names, c = MC.crafted()
    got, status = multipitch.multipitch_rows(c)
    assert status == 0
    on = lambda name: got[got["frame"] == names[name]]  # noqa: E731
    bins = lambda name: np.rint((on(name)["pitch_midi"] - 21.0) * 3.0).astype(int).tolist()  # noqa: E731
    assert len(on("alternating_131")) == 131 == multipitch.MAX_PEAKS_PER_ROW and bins("alternating_131") == list(range(1, 262, 2))
    assert len(on("plateaus")) == 0 and len(on("edge_cells")) == 0 and len(on("all_zero")) == 0
    assert bins("peaks_at_1_and_262") == [1, 262]
    assert bins("threshold_exact_and_one_step_below") == [40]
    skew = on("delta_near_half")
    delta = (skew["pitch_midi"] - 21.0) * 3.0 - np.array([120.0, 200.0])
    assert len(skew) == 2 and 0.49 < delta[0] <= 0.5 and -0.5 <= delta[1] < -0.49, delta
    # a row of 131 peaks is the most a row can have: the dense maps stay below it
    dense = MC.dense(np.random.default_rng(3), 400)
    pts, _ = multipitch.multipitch_rows(dense, MC.params(threshold=-1.0))
    per_row = np.bincount(pts["frame"], minlength=400)
    assert 70 <= per_row.mean() <= 100 and per_row.max() <= 131  # about a third of the bins


def test_too_little_room_reports_the_count_and_the_repeat_succeeds(lib):
    from basic_pitch_amd import multipitch

    c = MC.dense(np.random.default_rng(5), 7)
    p = multipitch.mp_params()
    want, _, _ = MC.restate_points(c, **MC.DEFAULT)
    n, status = C.c_int64(-1), C.c_int(-1)
    buf = np.zeros(len(want) + 1, MC.POINT)
    buf.view(np.uint8)[:] = 0x5A
    rc = lib.bp_multipitch_rows(c.ctypes.data, len(c), C.addressof(p), buf.ctypes.data, len(want) - 1, C.byref(n), C.byref(status))
    assert rc == -1 and n.value == len(want) and status.value == 0
    assert np.all(buf.view(np.uint8) == 0x5A), "nothing is written when the room is too small"
    rc = lib.bp_multipitch_rows(c.ctypes.data, len(c), C.addressof(p), buf.ctypes.data, n.value, C.byref(n), C.byref(status))
    assert rc == 0 and n.value == len(want)
    _same_points(buf[: len(want)], want, "repeat")
    assert np.all(buf[len(want):].view(np.uint8) == 0x5A)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_cell_that_is_not_finite_outside_the_band_gives_status_1_and_no_points(lib, value):
    from basic_pitch_amd import multipitch

    c = MC.dense(np.random.default_rng(9), 20)
    prm = MC.params(min_bin=100, max_bin=150)
    assert len(multipitch.multipitch_rows(c, prm)[0]) > 0
    for row, bin_ in ((0, 0), (19, 263), (7, 30), (11, 200)):  # all outside min_bin ... max_bin
        bad = MC.with_nonfinite(c, value, row, bin_)
        got, status = multipitch.multipitch_rows(bad, prm)
        assert status == 1 and len(got) == 0
        assert MC.restate_points(bad, **prm)[1] == 1


@pytest.mark.parametrize("fields, named", [
    (dict(threshold=np.nan), "threshold"), (dict(threshold=np.inf), "threshold"), (dict(min_bin=0), "min_bin"),
    (dict(max_bin=263), "max_bin"), (dict(min_bin=120, max_bin=119), "min_bin"), (dict(reserved=1), "reserved"),
])
def test_every_malformed_parameter_set_is_refused_by_name(lib, fields, named):
    from basic_pitch_amd import multipitch

    p = multipitch.mp_params(**fields)
    lib.bp_internal_mp_bad_params.restype, lib.bp_internal_mp_bad_params.argtypes = C.c_char_p, [C.c_void_p]
    why = lib.bp_internal_mp_bad_params(C.addressof(p))
    assert why and named in why.decode(), (fields, why)
    c = MC.bumps(np.random.default_rng(1), 3)
    n, status = C.c_int64(-7), C.c_int(-7)
    buf = np.zeros(1000, MC.POINT)
    assert lib.bp_multipitch_rows(c.ctypes.data, 3, C.addressof(p), buf.ctypes.data, 1000, C.byref(n), C.byref(status)) == -1
    assert lib.bp_internal_mp_bad_params(C.addressof(multipitch.mp_params())) is None


def test_the_other_bad_arguments_of_the_rows_checker_are_refused(lib):
    from basic_pitch_amd import multipitch

    p = multipitch.mp_params()
    c = MC.bumps(np.random.default_rng(1), 3)
    n, status = C.c_int64(0), C.c_int(0)
    args = lambda **kw: [kw.get("c", c.ctypes.data), kw.get("rows", 3), kw.get("p", C.addressof(p)), kw.get("pts", None),  # noqa: E731
                         kw.get("room", 0), kw.get("n", C.byref(n)), kw.get("st", C.byref(status))]
    for bad in (dict(c=None), dict(rows=-1), dict(p=None), dict(room=-1), dict(room=5), dict(n=None), dict(st=None)):
        assert lib.bp_multipitch_rows(*args(**bad)) == -1, bad
    assert lib.bp_multipitch_rows(*args(c=None, rows=0)) == 0 and n.value == 0 and status.value == 0


# ---- bp_score_f0_frames against the restatement
def _seeded_score_cases(n=300, seed=0):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        rows = int(rng.choice([0, 1, 40, 172, 173, 200]))
        c = MC.bumps(rng, rows) if k % 3 else MC.dense(rng, min(rows, 40))
        prm = MC.params(threshold=float(rng.choice([0.3, 0.5, 0.9])))
        points = MC.restate_points(c, **prm)[0]
        refs = MC.refs_for(rng, c, prm, n=int(rng.integers(0, 14)))
        if len(points) and len(refs):  # fractional refs half a semitone from a peak: at the exact tolerance
            for r in refs[:: 4]:
                on = points[points["frame"] == int(rng.integers(0, len(c)))]
                if len(on):
                    r[2] = float(on["pitch_midi"][0]) + float(rng.choice([0.5, -0.5]))
        tol = dict(pitch_tolerance_cents=float(rng.choice([0.0, 30.0, 50.0, 100.0])), strict=int(rng.integers(0, 2)))
        cases.append((points, refs, len(c), tol))
    return cases


def test_the_frame_counts_equal_the_restatement_on_seeded_cases(lib):
    from basic_pitch_amd import multipitch

    seen = np.zeros(6, np.int64)
    strict_matters = 0
    for k, (points, refs, n_frames, tol) in enumerate(_seeded_score_cases()):
        want, (e_miss, e_fa) = MC.restate_counts(points, refs, n_frames, **tol)
        got = multipitch.score_f0_frames(points, refs, n_frames, **tol)
        assert tuple(int(got[f]) for f in ("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub")) == want, (k, got, want, tol)
        assert want[1] == want[3] + want[4] + e_miss and want[2] == want[3] + want[4] + e_fa
        seen += (1, want[3] > 0, want[4] > 0, e_miss > 0, e_fa > 0, 0)
        if tol["pitch_tolerance_cents"] == 50.0:
            other = MC.restate_counts(points, refs, n_frames, pitch_tolerance_cents=50.0, strict=1 - tol["strict"])[0]
            strict_matters += other != want
    assert min(seen[1:5]) > 50, seen  # (the reference is not trivial: every count is exercised by many cases)
    assert strict_matters > 5, "no case sits exactly on the tolerance"


def test_a_ref_exactly_half_a_semitone_from_a_peak_hits_only_when_not_strict(lib):
    from basic_pitch_amd import multipitch

    points = np.zeros(2, MC.POINT)
    points["frame"], points["pitch_midi"] = [5, 5], [60.25, 64.0]
    refs = SC.notes([(SC.frame_time(5), SC.frame_time(6), 60.75), (SC.frame_time(5), SC.frame_time(6), 64.5)])
    for strict, tp in ((0, 2), (1, 0)):
        got = multipitch.score_f0_frames(points, refs, 10, pitch_tolerance_cents=50.0, strict=strict)
        assert (int(got["true_pos"]), int(got["e_sub"]), int(got["ref_frames"]), int(got["est_frames"])) == (tp, 2 - tp, 2, 2)
    # a point outside the segment's frames counts nowhere; equal pitches on a frame are one estimate; a bad pitch is refused
    extra = np.zeros(4, MC.POINT)
    extra["frame"], extra["pitch_midi"] = [5, 5, 10, -1], [60.25, 60.25, 60.0, 60.0]
    got = multipitch.score_f0_frames(extra, refs, 10)
    assert int(got["est_frames"]) == 1 and int(got["true_pos"]) == 1
    extra["pitch_midi"][0] = np.nan
    with pytest.raises(ValueError):
        multipitch.score_f0_frames(extra, refs, 10)
    with pytest.raises(ValueError):
        multipitch.score_f0_frames(points, refs, -1)


def test_the_python_result_follows_from_frames_and_pitches(lib):
    from basic_pitch_amd import multipitch
    from basic_pitch_amd.note_creation import model_frames_to_time

    points, _ = multipitch.multipitch_rows(MC.bumps(np.random.default_rng(2), 400))
    est = multipitch.MultiPitch.from_points(points)
    assert np.array_equal(est.times_s, model_frames_to_time(400)[est.frames])
    assert np.array_equal(est.freqs_hz, 440.0 * np.exp2((est.pitch_midi - 69.0) / 12.0))
    assert multipitch.midi_to_hz(np.array([69.0, 57.0]))[0] == 440.0 and abs(multipitch.midi_to_hz(np.array([57.0]))[0] - 220.0) < 1e-12
    assert est.salience.dtype == np.float32 and est.frames.dtype == np.int32 and est.status == 0


# ---- the source alone, under the host sanitizers
def test_the_checkers_link_without_a_device_and_run_clean_under_the_sanitizers(tmp_path):
    """tests/test_frame_score_cpu.py's pattern: the checkers' source with the three device-free sources it calls into and
    tools/sanitize/multipitch_host.cpp, plain g++, once with -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    csrc = os.path.join(ROOT, "basic_pitch_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", "sanitize", "multipitch_host.cpp")] + \
        [os.path.join(csrc, s) for s in ("multipitch_host.cpp", "note_frames_host.cpp", "note_score_host.cpp", "note_decode.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"multipitch_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("multipitch 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["points"]) > 10000 and int(sums["flagged"]) > 0 and int(sums["repeated"]) > 50 and int(sums["refused"]) >= 400
    assert int(sums["true_pos"]) > 0 and int(sums["e_sub"]) > 0
