"""Note-level scoring, the part that needs no GPU (include/basic_pitch_amd_score.h): the header's symbols are exported by both
libraries with the prototypes it declares, the three records are the bytes it says, and the host checker
bp_score_note_events gives the counts of an independent restatement (tests/score_cases.py: numpy predicates, scipy's maximum
bipartite matching) on seeded random cases, on chains only an augmenting matcher completes, at the boundaries of every
tolerance, with empty sides, and on the golden recording's events.  The refusals of the calls that take a handle are in
tests/test_gpu_score.py: a handle needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_cases as SC
from conftest import ROOT

NEW = ("bp_score_params_default", "bp_score_note_events", "bp_note_events_sweep_score", "bp_infer_clips_events_sweep_score")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, score

    build.build_library()
    return score.bind(_native.load_library())


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "void": None}


def _ctype_of(param):
    """The rule of tests/test_sweep_cpu.py: handles and plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def _header():
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_score.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- header and ABI
def test_every_symbol_of_the_score_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, score
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_sweep.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(score.PROTOTYPES) == set(_native.SCORE_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert score.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["n_sets", "sets", "n_decodes", "decodes", "ref_offsets", "refs", "score_params", "scores", "status"]
    assert names("bp_note_events_sweep_score") == ["h", "n_segments", "row_offsets", "note", "onset", "contour", "mem_kind"] + tail
    assert names("bp_infer_clips_events_sweep_score") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert names("bp_score_note_events") == ["est", "n_est", "ref", "n_ref", "p", "out"]
    bound = int(re.search(r"#define BP_SCORE_MAX_NOTES (\d+)", header).group(1))
    assert bound == score.MAX_NOTES and bound >= 4096
    # the bound's arithmetic is beside it and fits a compute unit's LDS; the statements the header owes
    assert f"{bound:,} notes x 6.125 bytes = {int(bound * 6.125):,} bytes" in text and bound * 6.125 <= 160 * 1024 < 2 * bound * 6.125
    for said in ("mir_eval 0.7", "UNPINNED", "without a logarithm", "average overlap ratio is NOT", "no bend map",
                 "do not filter the refs"):
        assert said in text, said
    # the existing headers and lists are what they were, the new header is one the build watches
    assert not set(NEW) & (set(_native.EXPORTED_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS))
    assert "basic_pitch_amd_score.h" in [os.path.basename(h) for h in build.HEADERS]
    assert {"note_score.hip", "note_score_host.cpp"} <= set(build.SOURCES)
    assert hasattr(Model, "sweep_note_scores") and hasattr(Model, "transcribe_clips_sweep_scores")


def test_the_symbols_are_exported_by_both_libraries(lib):
    import subprocess

    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_records_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native

    text, header = _header()
    ctype = {"double": C.c_double, "int32_t": C.c_int32}

    def fields(name):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        out = []
        for t, names in re.findall(r"\b(double|int32_t)\s+([a-z_, ]+);", body):
            out += [(n.strip(), ctype[t]) for n in names.split(",")]
        return out

    assert fields("bp_ref_note") == list(_native.bp_ref_note._fields_) and C.sizeof(_native.bp_ref_note) == 24
    assert [n for n, _ in fields("bp_ref_note")] == ["start_s", "end_s", "pitch_midi"]
    assert fields("bp_score_params") == list(_native.bp_score_params._fields_) and C.sizeof(_native.bp_score_params) == 40
    assert [n for n, _ in fields("bp_score_params")] == ["onset_tolerance_s", "offset_ratio", "offset_min_tolerance_s",
                                                         "pitch_tolerance_cents", "strict", "reserved"]
    assert fields("bp_note_score") == list(_native.bp_note_score._fields_) and C.sizeof(_native.bp_note_score) == 16
    assert [n for n, _ in fields("bp_note_score")] == ["n_ref", "n_est", "matched_onset", "matched_offset"]
    assert "24 bytes" in text and "16 bytes" in text and "40 bytes" in text
    p = _native.bp_score_params(1, 1, 1, 1, 1, 1)
    lib.bp_score_params_default(C.addressof(p))
    assert (p.onset_tolerance_s, p.offset_ratio, p.offset_min_tolerance_s, p.pitch_tolerance_cents, p.strict, p.reserved) == \
        (0.05, 0.2, 0.05, 50.0, 0, 0)
    assert {k: getattr(p, k) for k in SC.DEFAULTS} == SC.DEFAULTS


# ---- the checker against the restatement
def _checker(est, ref, **tolerances):
    from basic_pitch_amd import score

    c = score.score_note_events(SC.notes(est), SC.notes(ref), **tolerances)
    assert c["status"] == 0
    return int(c["n_ref"]), int(c["n_est"]), int(c["matched_onset"]), int(c["matched_offset"])


def test_seeded_random_cases_equal_the_restatement(lib):
    rng = np.random.default_rng(0)
    told_apart = 0
    for case in range(2000):
        est, ref = SC.random_case(rng)
        want = SC.restate(est, ref)
        assert _checker(est, ref) == want, (case, est, ref)
        told_apart += sum(SC.first_fit(g) < SC.matching_size(g) for g in SC.graphs(est, ref))
    print("graphs of 4000 in which a first fit is smaller than the maximum:", told_apart)
    assert told_apart >= 1  # the set tells a matcher that does not augment from one that does


@pytest.mark.parametrize("which", range(4))
def test_the_minimal_chain_in_every_scan_order(lib, which):
    est, ref = SC.CHAINS[which]
    g = SC.graphs(est, ref)[0]
    assert SC.matching_size(g) == 2
    assert SC.first_fit(g) == (1 if which == 0 else 2)  # arrangement 0 is the one that fails ests and refs in index order
    assert _checker(est, ref)[:3] == (2, 2, 2)
    assert sum(SC.first_fit(SC.graphs(e[::d], r[::c])[0]) == 1 for e, r in SC.CHAINS for d in (1, -1) for c in (1, -1)) == 4


@pytest.mark.parametrize("decoy_low", (True, False))
def test_a_long_chain_matches_all_eight(lib, decoy_low):
    est, ref = SC.long_chain(60, decoy_low)
    g = SC.graphs(est, ref)[0]
    assert g.sum(axis=0).tolist() == [2] * 7 + [1] == g.sum(axis=1).tolist()  # one path through all 16 notes: the decoy and the last est end it
    assert SC.matching_size(g) == 8 and SC.first_fit(g) == 7
    assert _checker(est, ref) == (8, 8, 8, 8) == SC.restate(est, ref)


def test_the_boundaries_of_every_tolerance(lib):
    ref = [(1.0, 2.0, 60.0)]
    # an onset distance that rounds to the tolerance counts, the next that does not, and `strict` makes 0.05 itself a miss
    assert _checker([(1.0500004, 2.0, 60)], ref)[2] == 1 == SC.restate([(1.0500004, 2.0, 60)], ref)[2]
    assert _checker([(1.0500006, 2.0, 60)], ref)[2] == 0 == SC.restate([(1.0500006, 2.0, 60)], ref)[2]
    assert abs(1.0500004 - 1.0) > 0.05  # it is the rounding that lets it in
    assert _checker([(0.05, 1.0, 60)], [(0.0, 1.0, 60.0)])[2] == 1 and _checker([(0.05, 1.0, 60)], [(0.0, 1.0, 60.0)], strict=1)[2] == 0
    assert SC.restate([(0.05, 1.0, 60)], [(0.0, 1.0, 60.0)], strict=1)[2] == 0
    # exactly 50 cents
    assert _checker([(1.0, 2.0, 60)], [(1.0, 2.0, 60.5)])[2] == 1 and _checker([(1.0, 2.0, 60)], [(1.0, 2.0, 60.5)], strict=1)[2] == 0
    assert _checker([(1.0, 2.0, 60)], [(1.0, 2.0, 59.5)])[2] == 1 and _checker([(1.0, 2.0, 60)], [(1.0, 2.0, 60.5000001)])[2] == 0
    # the offset tolerance: 0.2 x 1 s = 0.2 s rules over the minimum, 0.2 x 0.1 s = 0.02 s does not
    long_ref, short_ref = [(1.0, 2.0, 60.0)], [(1.0, 1.1, 60.0)]
    for est_end, ref_, want in ((2.2, long_ref, 1), (2.2000006, long_ref, 0), (1.8, long_ref, 1), (1.15, short_ref, 1),
                                (1.1500006, short_ref, 0), (1.13, short_ref, 1)):
        got = _checker([(1.0, est_end, 60)], ref_)
        assert got == (1, 1, 1, want) == SC.restate([(1.0, est_end, 60)], ref_), (est_end, ref_)
    assert _checker([(1.0, 2.2, 60)], long_ref, strict=1)[3] == 0 and _checker([(1.0, 2.1, 60)], long_ref, strict=1)[3] == 1
    # other tolerances than the defaults
    t = dict(onset_tolerance_s=0.1, offset_ratio=0.5, offset_min_tolerance_s=0.0, pitch_tolerance_cents=120.0)
    for est in ([(1.1, 2.5, 61)], [(1.1000006, 2.5, 61)], [(1.1, 2.5000006, 61)], [(1.0, 2.0, 62)]):
        assert _checker(est, ref, **t) == SC.restate(est, ref, **t), est
    # the second matching is a maximum matching of its own: two ests hit the ref at the onset, only the second at the offset
    est = [(1.0, 3.0, 60), (1.01, 2.0, 60)]
    assert _checker(est, ref) == (1, 2, 1, 1) == SC.restate(est, ref)


def test_empty_sides(lib):
    from basic_pitch_amd import score

    some = [(1.0, 2.0, 60.0), (2.0, 3.0, 62.0)]
    assert _checker([], some) == (2, 0, 0, 0) and _checker(some, []) == (0, 2, 0, 0) and _checker([], []) == (0, 0, 0, 0)
    counts = np.array([(2, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 0, 0, 0), (4, 2, 2, 1, 0)], score.COUNTS)
    p, r, f = score.precision_recall_f1(counts, offsets=False)
    assert p.tolist() == [0, 0, 0, 1.0] and r.tolist() == [0, 0, 0, 0.5] and f.tolist()[:3] == [0, 0, 0] and abs(f[3] - 2 / 3) < 1e-15
    p, r, f = score.precision_recall_f1(counts)
    assert (p[3], r[3]) == (0.5, 0.25) and abs(f[3] - 1 / 3) < 1e-15
    p, r, f = score.precision_recall_f1(np.array([(1, 1, 0, 0, 0)], score.COUNTS))
    assert f.tolist() == [0.0]  # nothing matched: no division by zero


def test_best_set_sums_over_the_segments_and_breaks_ties_low():
    from basic_pitch_amd import score

    c = np.zeros((3, 2), score.COUNTS)
    c["n_ref"], c["n_est"] = 4, 4
    c["matched_offset"] = [[4, 0], [2, 2], [1, 4]]  # sums 4, 4, 5
    c["matched_onset"] = [[4, 4], [4, 4], [1, 4]]
    assert score.best_set(c) == 2 and score.best_set(c, offsets=False) == 0  # the tie of sets 0 and 1 goes to 0
    with pytest.raises(ValueError):
        score.best_set(c[0])


def test_the_checker_refuses_what_the_header_says(lib):
    from basic_pitch_amd import _native, score

    INV, OK = _native.BP_ERR_INVALID_ARG, _native.BP_OK
    est, n = score.events_array([(1.0, 2.0, 60)])
    out = _native.bp_note_score()

    def call(ref_rows, n_est=1, est_ptr=C.addressof(est), out_ptr=C.addressof(out), p=None, **tol):
        ref = np.ascontiguousarray(ref_rows, np.float64).reshape(-1, 3)
        keep["p"] = score.score_params(**tol)  # alive over the call
        p = p if p is not None else C.addressof(keep["p"])
        return lib.bp_score_note_events(est_ptr, n_est, ref.ctypes.data if len(ref) else None, len(ref), p, out_ptr)

    keep = {}
    good = [(1.0, 2.0, 60.0)]
    assert call(good) == OK and (out.n_ref, out.n_est, out.matched_onset, out.matched_offset) == (1, 1, 1, 1)
    for bad in ([(np.nan, 2.0, 60.0)], [(1.0, np.inf, 60.0)], [(1.0, 2.0, np.nan)], [(2.0, 1.0, 60.0)], good + [(3.0, 2.9, 60.0)]):
        assert call(bad) == INV, bad
    assert call([(1.0, 1.0, 60.0)]) == OK  # an empty ref is a ref
    for field in ("onset_tolerance_s", "offset_ratio", "offset_min_tolerance_s", "pitch_tolerance_cents"):
        for v in (-1e-9, np.nan, np.inf):
            assert call(good, **{field: v}) == INV, (field, v)
    assert call(good, reserved=1) == INV
    assert call(good, n_est=-1) == INV and call(good, est_ptr=None) == INV and call(good, out_ptr=None) == INV
    assert call(good, n_est=0, est_ptr=None) == OK and out.n_est == 0
    assert lib.bp_score_note_events(C.addressof(est), 1, None, 0, None, C.addressof(out)) == INV  # null params
    with pytest.raises(ValueError):
        score.score_note_events([(1.0, 2.0, 60)], [(2.0, 1.0, 60.0)])
    with pytest.raises(TypeError):
        score.score_params(onset_tolerance=0.1)


def test_a_null_handle_is_refused(lib):
    from basic_pitch_amd import _native

    offs = (C.c_int64 * 2)()
    st = (C.c_int * 1)()
    sc = _native.bp_note_score()
    p_offs = C.cast(offs, C.POINTER(C.c_int64))
    assert lib.bp_note_events_sweep_score(None, 0, p_offs, None, None, None, 0, 0, None, 0, None, p_offs, None, None, C.addressof(sc),
                                          C.addressof(st)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_clips_events_sweep_score(None, 0, None, 22050, 0, 0, None, 0, None, p_offs, None, None, C.addressof(sc),
                                                 C.addressof(st)) == _native.BP_ERR_INVALID_ARG


# ---- the recording
def test_the_golden_events_against_themselves_and_with_moved_onsets(lib):
    from basic_pitch_amd import score

    z = np.load(os.path.join(GOLDEN, "vocadito_10_note_events.npz"))
    est = np.stack([z["start_s"], z["end_s"], z["pitch"].astype(np.float64)], axis=1)
    n = len(est)
    assert n == 28
    assert _checker(est, est) == (n, n, n, n) == SC.restate(est, est)
    moved = est.copy()
    moved[::2, 0] += 0.06  # every second onset by 60 ms: outside the tolerance, the offsets stay
    moved[:, 1] = np.maximum(moved[:, 1], moved[:, 0])
    want = SC.restate(est, moved)
    assert _checker(est, moved) == want
    assert want[2] < n and want[2] >= n // 2  # the moved ones are lost (unless a neighbour of the same pitch takes them)
    # the tuples the Python API returns score the same as rows
    tuples = [(float(a), float(b), int(c), np.float32(0.5), None) for a, b, c in est]
    c = score.score_note_events(tuples, moved)
    assert (int(c["n_ref"]), int(c["n_est"]), int(c["matched_onset"]), int(c["matched_offset"])) == want
