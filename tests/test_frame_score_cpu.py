"""Frame-level scoring, the part that needs no GPU (include/basic_pitch_amd_frame_score.h): the header's symbols are exported
by both libraries with the prototypes it declares, bp_frame_score is the 40 bytes it says, and the host checker
bp_score_note_frames gives the counts of an independent restatement (tests/frame_score_cases.py: a numpy roll, scipy's maximum
bipartite matching per frame) on seeded random cases, on chains only a maximum matching completes, at the boundaries of a
frame and of the tolerance, with empty sides, and on the golden recording's events; the checker's source runs clean under the
host sanitizers as a program of its own.  The calls that take a handle are in tests/test_gpu_frame_score.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_score_cases as FC
import score_cases as SC
from conftest import ROOT

NEW = ("bp_score_note_frames", "bp_note_events_sweep_frame_score", "bp_infer_clips_events_sweep_frame_score")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, frame_score

    build.build_library()
    return frame_score.bind(_native.load_library())


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
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_frame_score.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- header and ABI
def test_every_symbol_of_the_frame_score_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, frame_score
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_score.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(frame_score.PROTOTYPES) == set(_native.FRAME_SCORE_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert frame_score.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["n_sets", "sets", "n_decodes", "decodes", "ref_offsets", "refs", "score_params", "scores", "frames", "status"]
    assert names("bp_note_events_sweep_frame_score") == ["h", "n_segments", "row_offsets", "note", "onset", "contour", "mem_kind"] + tail
    assert names("bp_infer_clips_events_sweep_frame_score") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert names("bp_score_note_frames") == ["est", "n_est", "ref", "n_ref", "n_frames", "p", "out"]
    # the statements the header owes
    flat = " ".join(text.replace("*", " ").split())
    for said in ("mir_eval 0.7", "UNPINNED", "strictly increasing", "e_miss = ref_frames - true_pos - e_sub",
                 "e_fa = est_frames - true_pos - e_sub", "n_ref(fr) = tp(fr) + e_sub(fr) + e_miss(fr)", "chroma", "ALLOWED, not required"):
        assert said in flat, said
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | set(_native.EXPORTED_SYMBOLS)
    assert not set(NEW) & old
    assert "basic_pitch_amd_frame_score.h" in [os.path.basename(h) for h in build.HEADERS]
    assert {"note_frames.hip", "note_frames_host.cpp"} <= set(build.SOURCES)
    assert hasattr(Model, "sweep_frame_scores") and hasattr(Model, "transcribe_clips_sweep_frame_scores")


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_record_is_the_40_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, frame_score

    text, header = _header()
    body = re.search(r"typedef struct bp_frame_score \{(.*?)\} bp_frame_score;", header, flags=re.S).group(1)
    fields = [(n.strip(), C.c_int64) for t, names in re.findall(r"\b(int64_t)\s+([a-z_, ]+);", body) for n in names.split(",")]
    assert fields == list(_native.bp_frame_score._fields_) and C.sizeof(_native.bp_frame_score) == 40 and "40 bytes" in text
    assert [n for n, _ in fields] == list(FC.FIELDS) == list(frame_score.FRAME_COUNTS.names[:5])
    assert frame_score.FRAME_COUNTS.names[5] == "status" and frame_score.FRAME_COUNTS["true_pos"] == np.int64


# ---- the checker against the restatement
def _checker(est, ref, n_frames, **tolerances):
    from basic_pitch_amd import frame_score

    c = frame_score.score_note_frames(SC.notes(est), SC.notes(ref), n_frames, **tolerances)
    assert c["status"] == 0
    return tuple(int(c[f]) for f in FC.FIELDS)


@pytest.fixture(scope="module")
def restated():
    """The 2,000 seeded cases with the restatement's sums, computed once."""
    return [(case, FC.restate(case[0], case[1], case[2], **case[3])) for case in FC.seeded_cases()]


def test_the_restatement_is_not_trivial_on_the_seeded_cases(restated):
    n = len(restated)
    assert n == 2000
    partial = sum(0 < w[3] < min(w[1], w[2]) for (w, _) in (r for _, r in restated))
    subs = sum(w[4] > 0 for _, (w, _) in restated)
    distinct = len({w for _, (w, _) in restated})
    print("partial matchings", partial, "with substitutions", subs, "distinct tuples", distinct)
    assert partial >= 0.3 * n and subs >= 0.2 * n and distinct >= 200
    assert {c[2] for c, _ in restated} == set(FC.N_FRAMES) and {c[3]["pitch_tolerance_cents"] for c, _ in restated} == set(FC.TOLERANCES)
    assert {c[3]["strict"] for c, _ in restated} == {0, 1}


def test_seeded_random_cases_equal_the_restatement_and_the_identities_hold(lib, restated):
    for k, ((est, ref, n_frames, tol), (want, (e_miss, e_fa))) in enumerate(restated):
        got = _checker(est, ref, n_frames, **tol)
        assert got == want, (k, got, want, tol)
        # misses and false alarms, summed per frame by the restatement, against the identity on the checker's counts
        assert got[1] == got[3] + got[4] + e_miss and got[2] == got[3] + got[4] + e_fa, (k, got, e_miss, e_fa)


# ---- chains
@pytest.mark.parametrize("which", range(4))
def test_the_minimal_chain_in_every_order(lib, which):
    est, ref = FC.chains()[which]
    want, _ = FC.restate(est, ref, 50)
    assert want == (50, 40, 40, 40, 0)  # 20 frames, two a side, both matched
    assert _checker(est, ref, 50) == want
    # on every sounding frame the maximum is 2, and a first fit in ref order is smaller for at least one of the four orders
    stranded = 0
    for e, r in FC.chains():
        (counts, g) = FC.per_frame(e, r, 50)[15]
        assert counts[:3] == (2, 2, 2) and SC.matching_size(g) == 2
        stranded += SC.first_fit(g.T) < 2
    assert stranded >= 1
    # with `strict` 60.5 hits neither: one true positive and one substitution per frame
    assert _checker(est, ref, 50, strict=1) == (50, 40, 40, 20, 20) == FC.restate(est, ref, 50, strict=1)[0]


@pytest.mark.parametrize("decoy_low", (True, False))
def test_a_long_chain_matches_all_eight_on_every_frame(lib, decoy_low):
    est, ref = SC.long_chain(60, decoy_low, start=SC.frame_time(160), end=SC.frame_time(200))
    frames = FC.per_frame(est, ref, 345)
    counts, g = frames[172]
    # a first fit in ref order that takes the est nearest the decoy's side strands one ref (the ests of g are ascending)
    assert counts[:3] == (8, 8, 8) and min(SC.first_fit(g.T), SC.first_fit(g[:, ::-1].T)) == 7
    want, _ = FC.restate(est, ref, 345)
    assert want == (345, 320, 320, 320, 0)
    assert _checker(est, ref, 345) == want


# ---- boundaries
def test_the_boundaries_of_a_frame_and_of_the_tolerance(lib):
    t = SC.frame_time
    est = [(t(0), t(400), 60)]
    one = lambda ref, n=200, **tol: _checker(est, [ref], n, **tol)  # noqa: E731
    # a start exactly on a frame time sounds there, an end exactly on a frame time does not; just past it, it does
    assert one((t(10), t(20), 60.0)) == (200, 10, 200, 10, 0)
    assert one((np.nextafter(t(10), np.inf), t(20), 60.0))[1] == 9 and one((t(10), np.nextafter(t(20), np.inf), 60.0))[1] == 11
    # ... also at the step down of the time at frame 172, where the frame before is only 1.3 ms earlier
    assert 0 < t(172) - t(171) < 0.0013 and t(173) - t(172) > 0.0116
    assert one((t(172), t(173), 60.0)) == (200, 1, 200, 1, 0) and one((t(171), t(172), 60.0))[1] == 1
    assert one((np.nextafter(t(171), np.inf), t(172), 60.0))[1] == 0
    for ref in ((t(172), t(173), 60.0), (t(171), t(172), 60.0), (np.nextafter(t(171), np.inf), t(172), 60.0)):
        assert one(ref) == FC.restate(est, [ref], 200)[0]
    # no length: sounds nowhere; before 0 and past the end: clipped
    assert one((t(10), t(10), 60.0)) == (200, 0, 200, 0, 0)
    assert one((-1.0, t(5), 60.0)) == (200, 5, 200, 5, 0) and one((t(190), 100.0, 60.0)) == (200, 10, 200, 10, 0)
    assert one((-5.0, 100.0, 60.0)) == (200, 200, 200, 200, 0) and one((-5.0, -1.0, 60.0))[1] == 0 and one((50.0, 60.0, 60.0))[1] == 0
    # two refs of one pitch over one frame count twice (one is matched, one missed), two events of one pitch once
    twice = [(t(10), t(20), 60.0), (t(15), t(25), 60.0)]
    assert _checker(est, twice, 200) == (200, 20, 200, 15, 0) == FC.restate(est, twice, 200)[0]
    doubled = [(t(10), t(20), 60), (t(15), t(25), 60)]
    assert _checker(doubled, [(t(0), t(30), 60.0)], 200) == (200, 30, 15, 15, 0) == FC.restate(doubled, [(t(0), t(30), 60.0)], 200)[0]
    # exactly the tolerance hits with <= and misses with <; a substitution is a ref and an est on one frame that do not hit
    assert one((t(10), t(20), 60.5)) == (200, 10, 200, 10, 0) and one((t(10), t(20), 60.5), strict=1) == (200, 10, 200, 0, 10)
    assert one((t(10), t(20), 59.5))[3] == 10 and one((t(10), t(20), 60.5000001))[3:] == (0, 10)
    assert one((t(10), t(20), 61.25), pitch_tolerance_cents=125.0)[3] == 10 and one((t(10), t(20), 60.0), pitch_tolerance_cents=0.0)[3] == 10
    # pitches outside 21 ... 108 and fractional ones are pitches like any other
    assert _checker([(t(0), t(20), 120)], [(t(0), t(20), 120.25)], 50) == (50, 20, 20, 20, 0)
    assert _checker([(t(0), t(20), 3)], [(t(0), t(20), 2.4)], 50) == (50, 20, 20, 0, 20)


def test_empty_sides_and_no_frames(lib):
    t = SC.frame_time
    some = [(t(1), t(11), 60.0), (t(5), t(15), 62.0)]
    assert _checker([], some, 100) == (100, 20, 0, 0, 0) and _checker(some, [], 100) == (100, 0, 20, 0, 0)
    assert _checker([], [], 100) == (100, 0, 0, 0, 0) and _checker(some, some, 0) == (0, 0, 0, 0, 0) and _checker([], [], 0) == (0,) * 5
    assert _checker(some, some, 8) == (8, 10, 10, 10, 0)


def test_the_checker_refuses_what_the_header_says(lib):
    from basic_pitch_amd import _native, frame_score, score

    INV, OK = _native.BP_ERR_INVALID_ARG, _native.BP_OK
    est, n = score.events_array([(1.0, 2.0, 60)])
    out = _native.bp_frame_score()
    keep = {}

    def call(ref_rows, n_est=1, n_frames=300, est_ptr=C.addressof(est), out_ptr=C.addressof(out), **tol):
        ref = np.ascontiguousarray(ref_rows, np.float64).reshape(-1, 3)
        keep["p"] = score.score_params(**tol)  # alive over the call
        return lib.bp_score_note_frames(est_ptr, n_est, ref.ctypes.data if len(ref) else None, len(ref), n_frames,
                                        C.addressof(keep["p"]), out_ptr)

    good = [(1.0, 2.0, 60.0)]
    assert call(good) == OK and out.n_frames == 300 and out.true_pos == out.ref_frames == out.est_frames > 80
    for bad in ([(np.nan, 2.0, 60.0)], [(1.0, np.inf, 60.0)], [(1.0, 2.0, np.nan)], [(2.0, 1.0, 60.0)], good + [(3.0, 2.9, 60.0)]):
        assert call(bad) == INV, bad
    assert call([(1.0, 1.0, 60.0)]) == OK and out.ref_frames == 0  # an empty ref is a ref
    for field in ("onset_tolerance_s", "offset_ratio", "offset_min_tolerance_s", "pitch_tolerance_cents"):
        for v in (-1e-9, np.nan, np.inf):
            assert call(good, **{field: v}) == INV, (field, v)  # the fields the frame level does not read are validated too
    assert call(good, reserved=1) == INV
    assert call(good, n_frames=-1) == INV and call(good, n_frames=0) == OK and out.n_frames == 0
    assert call(good, n_est=-1) == INV and call(good, est_ptr=None) == INV and call(good, out_ptr=None) == INV
    assert call(good, n_est=0, est_ptr=None) == OK and out.est_frames == 0
    assert lib.bp_score_note_frames(C.addressof(est), 1, None, 0, 10, None, C.addressof(out)) == INV  # null params
    with pytest.raises(ValueError):
        frame_score.score_note_frames([(1.0, 2.0, 60)], good, -1)
    with pytest.raises(TypeError):
        frame_score.score_note_frames([(1.0, 2.0, 60)], good, 10, pitch_tolerance=50.0)


def test_a_null_handle_is_refused(lib):
    from basic_pitch_amd import _native

    offs = (C.c_int64 * 2)()
    st = (C.c_int * 1)()
    fr = _native.bp_frame_score()
    p_offs = C.cast(offs, C.POINTER(C.c_int64))
    assert lib.bp_note_events_sweep_frame_score(None, 0, p_offs, None, None, None, 0, 0, None, 0, None, p_offs, None, None, None,
                                                C.addressof(fr), C.addressof(st)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_clips_events_sweep_frame_score(None, 0, None, 22050, 0, 0, None, 0, None, p_offs, None, None, None,
                                                       C.addressof(fr), C.addressof(st)) == _native.BP_ERR_INVALID_ARG


# ---- the rates
def test_frame_metrics_against_hand_computed_values():
    from basic_pitch_amd import frame_score as FS

    #                 n_frames ref est tp sub
    counts = np.array([(100, 40, 50, 30, 5, 0), (100, 0, 10, 0, 0, 0), (100, 10, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (10, 8, 8, 8, 0, 1)],
                      FS.FRAME_COUNTS)
    m = FS.frame_metrics(counts)
    assert set(m) == {"precision", "recall", "accuracy", "e_sub", "e_miss", "e_fa", "e_tot"}
    assert m["precision"].tolist() == [0.6, 0.0, 0.0, 0.0, 1.0] and m["recall"].tolist() == [0.75, 0.0, 0.0, 0.0, 1.0]
    assert m["accuracy"].tolist() == [0.5, 0.0, 0.0, 0.0, 1.0]               # 30 / (40 + 50 - 30)
    assert m["e_sub"].tolist() == [0.125, 0.0, 0.0, 0.0, 0.0]                # 5 / 40
    assert m["e_miss"].tolist() == [0.125, 0.0, 1.0, 0.0, 0.0]               # (40 - 30 - 5) / 40; 10 / 10
    assert m["e_fa"].tolist() == [0.375, 0.0, 0.0, 0.0, 0.0]                 # (50 - 30 - 5) / 40; no refs: 0, not 10 / 0
    assert m["e_tot"].tolist() == [0.625, 0.0, 1.0, 0.0, 0.0]
    shaped = FS.frame_metrics(counts[:4].reshape(2, 2))
    assert shaped["accuracy"].shape == (2, 2)


def test_best_set_by_accuracy_sums_over_the_segments_and_breaks_ties_low():
    from basic_pitch_amd import frame_score as FS

    c = np.zeros((3, 2), FS.FRAME_COUNTS)
    c["ref_frames"], c["est_frames"] = 10, 10
    c["true_pos"] = [[10, 0], [5, 5], [3, 8]]  # sums 10, 10, 11
    assert FS.best_set_by_accuracy(c) == 2
    c["true_pos"][2] = [2, 8]                  # all 10: the tie goes to set 0
    assert FS.best_set_by_accuracy(c) == 0
    with pytest.raises(ValueError):
        FS.best_set_by_accuracy(c[0])


# ---- the recording
def test_the_golden_events_against_themselves_and_against_refs_made_from_them(lib):
    from basic_pitch_amd import frame_score as FS

    z = np.load(os.path.join(GOLDEN, "vocadito_10_note_events.npz"))
    est = np.stack([z["start_s"], z["end_s"], z["pitch"].astype(np.float64)], axis=1)
    n_frames = int(np.ceil(est[:, 1].max() * 22050.0 / 256.0)) + 20
    assert len(est) == 28 and SC.frame_time(n_frames - 1) > est[:, 1].max()
    same = _checker(est, est, n_frames)
    assert same == FC.restate(est, est, n_frames)[0]
    assert same[1] == same[2] == same[3] > 500 and same[4] == 0
    m = FS.frame_metrics(FS.score_note_frames(est, est, n_frames))
    assert (m["precision"], m["recall"], m["accuracy"], m["e_tot"]) == (1.0, 1.0, 1.0, 0.0)
    # refs made from them: every third a semitone up (substitutions), every fourth dropped (false alarms), one added (misses)
    refs = est.copy()
    refs[::3, 2] += 1.0
    refs = np.concatenate([np.delete(refs, np.s_[1::4], axis=0), [(0.0, SC.frame_time(5), 30.0)]])
    want, (e_miss, e_fa) = FC.restate(est, refs, n_frames)
    got = _checker(est, refs, n_frames)
    assert got == want and all(v > 0 for v in got) and e_miss > 0 and e_fa > 0
    # the tuples the Python API returns score the same as rows
    tuples = [(float(a), float(b), int(c), np.float32(0.5), None) for a, b, c in est]
    c = FS.score_note_frames(tuples, refs, n_frames)
    assert tuple(int(c[f]) for f in FC.FIELDS) == want


# ---- the source alone, under the host sanitizers
def test_the_checker_links_without_a_device_and_runs_clean_under_the_sanitizers(tmp_path):
    """tests/test_host_sources_cpu.py's pattern: the checker's source with the two device-free sources it calls into and
    tools/sanitize/frame_score_host.cpp, plain g++, once with -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    csrc = os.path.join(ROOT, "basic_pitch_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", "sanitize", "frame_score_host.cpp")] + \
        [os.path.join(csrc, s) for s in ("note_frames_host.cpp", "note_score_host.cpp", "note_decode.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"frame_score_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "300"], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("frame scores 300 cases: ")
    sums = dict(zip(outs[0].split()[4::2], map(int, outs[0].split()[5::2])))
    assert sums["true_pos"] > 0 and sums["e_sub"] > 0 and sums["ref_frames"] > sums["true_pos"] and sums["refused"] >= 500
