"""Forced alignment, the part that needs no GPU (include/basic_pitch_amd_align.h): the header's symbols are exported by both
libraries with the prototypes it declares, the structures are the bytes it says, the host checker bp_align_rows gives what an
independent restatement gives (tests/align_cases.py: numpy int64) on seeded maps and state lists, the best of ALL monotone
paths of small problems under the header's tie rule, and the planted first frames of planted problems; the statuses and the
refusals; the Python layer on the golden clip; the checker's source under the host sanitizers as a program of its own.  The
calls that take a handle are in tests/test_gpu_align.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_cases as AC
from conftest import GOLDEN, ROOT

NEW = ("bp_align_params_default", "bp_align_rows", "bp_align_from_maps", "bp_infer_clips_align")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, align, build

    build.build_library()
    return align.bind(_native.load_library())


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p, "void": None}


def _ctype_of(param):
    """The rule of tests/test_score_cpu.py: handles and plain data pointers are void pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", re.sub(r"/\*.*?\*/", " ", param)).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def _header():
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_align.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _check(got, want, where):
    (ff, total, status), (w_ff, w_total, w_status) = got, want
    assert (status, total) == (w_status, w_total), where
    assert ff.dtype == np.int32 and ff.tolist() == np.asarray(w_ff).tolist(), where


# ---- header and ABI
def test_every_symbol_of_the_align_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, align, build
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_score.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(align.PROTOTYPES) == set(_native.ALIGN_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert align.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["state_offsets", "states", "p", "first_frame", "max_states", "total", "status"]
    assert names("bp_align_rows") == ["note", "onset", "rows", "states", "n_states", "p", "first_frame", "max_states", "total", "status"]
    assert names("bp_align_from_maps") == ["h", "n_segments", "row_offsets", "note", "onset", "mem_kind"] + tail
    assert names("bp_infer_clips_align") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    # the statements the header owes: unpinned, the quantisation, the gains, the recurrence lines, the tie rule, the figures
    flat = " ".join(text.replace("*", " ").split())
    for said in ("UNPINNED", "q(x) = (int)floorf(min(max(x, 0.0f), 1.0f) 1024.0f + 0.5f)",
                 "g[t][j] = sum over p in active_j of qn[t][p] - threshold_q |active_j|",
                 "b[t][j] = onset_weight sum over p in begins_j of qo[t][p]",
                 "D[0][0] = g[0][0] + b[0][0] if earliest_0 <= 0", "stay = D[t-1][j] + g[t][j]",
                 "enter = D[t-1][j-1] + g[t][j] + b[t][j]", "earliest_j <= t <= latest_j", "D[t][j] = max(stay, enter)",
                 "unreachable stays unreachable", "ENTER ONLY WHEN STRICTLY GREATER", "ties stay",
                 "smallest first_frame[S - 1], then the smallest first_frame[S - 2]", "L1 distance", "they are not tuned",
                 "ONE barrier per frame", "ONE BIT per cell", "88 x 1024 < 2^24", "163,840 bytes", "66,576",
                 "268,435,456 cells x 8 bytes = 2,147,483,648 bytes", "33,554,432 bytes"):
        assert said in flat, said
    for macro, value in (("BP_ALIGN_PITCHES", align.PITCHES), ("BP_ALIGN_Q_ONE", align.Q_ONE), ("BP_ALIGN_MAX_ONSET_WEIGHT", align.MAX_ONSET_WEIGHT),
                         ("BP_ALIGN_LANES", align.LANES), ("BP_ALIGN_SMALL_LANES", align.SMALL_LANES),
                         ("BP_ALIGN_STATES_PER_LANE", align.STATES_PER_LANE), ("BP_ALIGN_MAX_CELLS", align.MAX_CELLS),
                         ("BP_ALIGN_READ_AHEAD", align.READ_AHEAD), ("BP_ALIGN_READ_AHEAD_WIDE", align.READ_AHEAD_WIDE),
                         ("BP_ALIGN_TILE_ROWS", align.TILE_ROWS), ("BP_ALIGN_EMIT_ROWS", align.EMIT_ROWS)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert "#define BP_ALIGN_MAX_STATES (BP_ALIGN_LANES * BP_ALIGN_STATES_PER_LANE)" in header
    assert align.MAX_STATES == align.LANES * align.STATES_PER_LANE >= 4096
    assert align.TILE_ROWS * align.MAX_STATES // 8 + 2 * align.STATES_PER_LANE * (align.LANES // 64) * 8 + 16 == 66576 < 163840
    assert align.MAX_CELLS * 8 == 2147483648 and align.MAX_CELLS // 8 == 33554432 and 15500 * 4096 == 63488000
    assert align.PITCHES * align.Q_ONE < 2 ** 24 and align.ALIGN_STATE == AC.STATE and align.FREE == AC.FREE
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.MELODY_SYMBOLS) | set(_native.MULTIPITCH_SYMBOLS) | set(_native.FRAME_SCORE_SYMBOLS) | set(_native.SCORE_SYMBOLS) | \
        set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | set(_native.EXPORTED_SYMBOLS) | set(_native.FLAC_CLIPS_SYMBOLS) | \
        set(_native.CONTAINERS_SYMBOLS) | set(_native.ADPCM_SYMBOLS)
    assert not set(NEW) & old
    assert len(_native.MELODY_SYMBOLS) == 7 and len(_native.MULTIPITCH_SYMBOLS) == 7 and len(_native.SCORE_SYMBOLS) == 4
    assert os.path.basename(build.ALIGN_HEADER) == "basic_pitch_amd_align.h" and build.ALIGN_HEADER in build.HEADERS
    assert {"align.hip", "align_host.cpp"} <= set(build.SOURCES)
    for entry in ("align", "transcribe_clips_align"):
        assert hasattr(Model, entry), entry
    unpinned = open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()
    assert "basic_pitch_amd_align.h" in unpinned and "aligner" in unpinned


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, align

    text, header = _header()
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64}
    for name, size in (("bp_align_state", 40), ("bp_align_params", 16)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = []
        for t, decl in re.findall(r"\b(int32_t|uint64_t)\s+([a-z_0-9, \[\]]+);", body):
            for n in decl.split(","):
                arr = re.fullmatch(r"\s*([a-z_]+)\[(\d+)\]\s*", n)
                fields.append((arr.group(1), ctype[t] * int(arr.group(2))) if arr else (n.strip(), ctype[t]))
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, (name, fields)
        assert f"/* {size} bytes */" in text
    assert align.ALIGN_STATE.itemsize == 40 and [align.ALIGN_STATE.fields[n][1] for n in align.ALIGN_STATE.names] == [0, 16, 32, 36]
    p = align.align_params()
    assert (p.threshold_q, p.onset_weight, list(p.reserved)) == (307, 2, [0, 0])
    assert align.align_params(threshold_q=5).threshold_q == 5 and align.align_params(dict(onset_weight=3)).onset_weight == 3
    with pytest.raises(TypeError):
        align.align_params(threshold=1)


# ---- the checker against the restatement
@pytest.mark.parametrize("kind", ["thousand", "eighths"])
def test_the_checker_equals_the_numpy_restatement_on_seeded_problems(lib, kind):
    from basic_pitch_amd import align

    rng = np.random.default_rng(11 if kind == "thousand" else 12)
    seen = {0: 0, 2: 0}
    for case in range(60):
        rows = int(rng.choice([1, 2, 3, 9, 33, 64, 65, 130, 173]))
        S = int(rng.integers(1, min(rows, 70) + 1))
        note, onset = AC.random_maps(rng, rows, kind)
        states = AC.random_states(rng, S, rows, windows=case % 2 == 1)
        prm = dict(threshold_q=int(rng.choice([0, 128, 307, 512, 1024])), onset_weight=int(rng.integers(0, 17)))
        want = AC.restate(note, onset, states, **prm)
        _check(align.align_rows(note, onset, states, **prm), want, (kind, case, rows, S, prm))
        seen[want[2]] += 1
        if want[2] == 0:
            ff = want[0]
            assert ff[0] == 0 and np.all(np.diff(ff) > 0) and ff[-1] < rows
    assert seen[0] >= 40, seen


def test_the_quantisation_clamps_and_rounds_as_the_header_says(lib):
    """One state with one pitch, no onset weight, threshold 0: the total of a one-row segment is q(x) itself."""
    from basic_pitch_amd import align

    st = AC.make_states([[5]])
    for x, q in ((0.0, 0), (1.0, 1024), (-3.0, 0), (7.5, 1024), (0.5, 512), (0.00048828125, 1), (0.000487, 0), (0.3, 307),
                 (np.inf, 1024), (-np.inf, 0), (1023.5 / 1024.0, 1024), (1023.4 / 1024.0, 1023)):
        note = np.zeros((1, 88), np.float32)
        note[0, 5] = x
        ff, total, status = align.align_rows(note, np.zeros((1, 88), np.float32), st, threshold_q=0, onset_weight=0)
        assert (ff.tolist(), total, status) == ([0], q, 0), x
        assert int(AC.quantise(np.float32(x))) == q


# ---- every path of small problems
def test_the_best_of_all_monotone_paths_under_the_tie_rule(lib):
    from basic_pitch_amd import align

    rng = np.random.default_rng(21)
    prm = dict(threshold_q=384, onset_weight=1)  # 3/8: gains are multiples of 128 and ties are frequent
    tied = infeasible = 0
    for case in range(120):
        rows = int(rng.integers(1, 11))
        S = int(rng.integers(1, min(rows, 5) + 1))
        if case % 6 == 5:  # all-equal maps
            note = np.full((rows, 88), rng.integers(0, 9) / 8.0, np.float32)
            onset = np.full((rows, 88), rng.integers(0, 9) / 8.0, np.float32)
        else:
            note, onset = AC.random_maps(rng, rows, "eighths")
        states = AC.random_states(rng, S, rows, most=2)
        if case % 3 == 2:  # windows, some of which cannot be met
            for j in range(1, S):
                lo = int(rng.integers(0, rows))
                states["earliest"][j], states["latest"][j] = lo, lo + int(rng.integers(0, 3))
        want = AC.best_by_enumeration(note, onset, states, **prm)
        _check(align.align_rows(note, onset, states, **prm), want, (case, rows, S))
        _check(AC.restate(note, onset, states, **prm), want, ("the restatement", case))
        infeasible += want[2] == 2
        if want[2] == 0 and S > 1:  # is the maximum shared by another path?  then the tie rule decided
            g, b = AC.gains(note, onset, states, **prm)
            f = want[0].tolist()
            later = f[:-1] + [f[-1] + 1]
            if later[-1] < rows and states["latest"][S - 1] >= later[-1]:
                ends = later[1:] + [rows]
                tied += sum(int(g[later[j]:ends[j], j].sum()) + int(b[later[j], j]) for j in range(S)) == want[1]
    assert tied >= 5 and infeasible >= 3, (tied, infeasible)
    # all-zero gains without windows: every path is optimal, and the rule singles out f[j] = j
    for rows, S in ((10, 5), (7, 1), (4, 4)):
        z = np.zeros((rows, 88), np.float32)
        ff, total, status = align.align_rows(z, z, AC.make_states([[3]] * S), threshold_q=0, onset_weight=0)
        assert (ff.tolist(), total, status) == (list(range(S)), 0, 0)


# ---- planted paths
@pytest.mark.parametrize("seed", range(24))
def test_planted_first_frames_are_recovered_exactly_with_the_defaults(lib, seed):
    from basic_pitch_amd import align

    note, onset, states, f = AC.planted(seed)
    ff, total, status = align.align_rows(note, onset, states)
    assert status == 0 and ff.tolist() == f.tolist(), (seed, len(states), len(note))
    _check((ff, total, status), AC.restate(note, onset, states), seed)


def test_the_planted_problems_cover_their_range():
    sizes = [(len(AC.planted(s)[2]), len(AC.planted(s)[0])) for s in range(24)]
    assert min(s for s, _ in sizes) <= 5 and max(s for s, _ in sizes) >= 60 and max(r for _, r in sizes) >= 400
    repeats = 0
    for s in range(24):
        st = AC.planted(s)[2]
        same = np.all(st["active"][1:] == st["active"][:-1], axis=1)
        assert np.all(st["begins"][1:][same].any(axis=1))  # adjacent states differ in their set or carry a begins
        repeats += int(same.sum())
    assert repeats >= 3


# ---- statuses and refusals
def test_status_1_a_nan_in_either_map_in_a_band_no_state_uses(lib):
    from basic_pitch_amd import align

    rng = np.random.default_rng(31)
    note, onset = AC.random_maps(rng, 40)
    states = AC.make_states([[10], [10, 12], [12]], [[10], [12], []])
    assert align.align_rows(note, onset, states)[2] == 0
    for which in (0, 1):
        for row, pitch in ((0, 87), (17, 0), (39, 50)):
            maps = [note.copy(), onset.copy()]
            maps[which][row, pitch] = np.nan
            ff, total, status = align.align_rows(maps[0], maps[1], states)
            assert (ff.tolist(), total, status) == ([-1, -1, -1], 0, 1), (which, row, pitch)
            _check((ff, total, status), AC.restate(maps[0], maps[1], states), (which, row, pitch))
    # an infinity is clamped, not flagged; a NaN decides before infeasibility does
    note[3, 3] = np.inf
    assert align.align_rows(note, onset, states)[2] == 0
    note[3, 3] = np.nan
    assert align.align_rows(note[:2], onset[:2], states)[2] == 2 and align.align_rows(note[:4], onset[:4], AC.make_states([[1]] * 5))[2] == 1


def test_status_2_more_states_than_rows_a_late_first_state_and_windows_that_cannot_be_met(lib):
    from basic_pitch_amd import align

    rng = np.random.default_rng(32)
    note, onset = AC.random_maps(rng, 12)
    gone = lambda st: ([-1] * len(st), 0, 2)  # noqa: E731
    cases = {
        "S = rows + 1": AC.make_states([[1]] * 13),
        "earliest_0 > 0": AC.make_states([[1], [2]], earliest=[1, 0]),
        "a window that closes before its predecessor can open": AC.make_states([[1], [2], [3]], earliest=[0, 6, 2], latest=[AC.FREE, 8, 5]),
        "a window beyond the segment": AC.make_states([[1], [2]], earliest=[0, 12]),
    }
    for name, st in cases.items():
        ff, total, status = align.align_rows(note, onset, st)
        assert (ff.tolist(), total, status) == gone(st), name
        _check((ff, total, status), AC.restate(note, onset, st), name)
    # the same lists are feasible once the obstacle is gone
    assert align.align_rows(note, onset, AC.make_states([[1]] * 12))[0].tolist() == list(range(12))
    assert align.align_rows(note, onset, AC.make_states([[1], [2], [3]], earliest=[0, 6, 7], latest=[AC.FREE, 8, 9]))[2] == 0
    # states without a row: infeasible; nothing at all: status 0
    z = np.zeros((0, 88), np.float32)
    assert align.align_rows(z, z, AC.make_states([[1]]))[1:] == (0, 2)
    assert align.align_rows(z, z, np.zeros(0, AC.STATE))[1:] == (0, 0)


def test_every_malformed_params_value_or_state_is_refused(lib):
    from basic_pitch_amd import _native, align

    rng = np.random.default_rng(33)
    note, onset = AC.random_maps(rng, 9)
    good = AC.make_states([[0], [87], [5, 6]], [[0], [], [6]])
    ff = np.zeros(8, np.int32)
    total, status = C.c_int64(7), C.c_int(7)

    def call(states, p, rows=9, n=None, room=8, note_p=note.ctypes.data, ff_p=ff.ctypes.data, total_p=C.byref(total), status_p=C.byref(status)):
        st = np.ascontiguousarray(states, AC.STATE)
        return lib.bp_align_rows(note_p, onset.ctypes.data, rows, st.ctypes.data, len(st) if n is None else n, C.addressof(p), ff_p, room,
                                 total_p, status_p)

    ok = align.align_params()
    assert call(good, ok) == _native.BP_OK
    for field, value in (("threshold_q", -1), ("threshold_q", 1025), ("onset_weight", -1), ("onset_weight", 17), ("reserved", 1), ("reserved", (0, 1))):
        assert call(good, align.align_params(**{field: value})) == _native.BP_ERR_INVALID_ARG, (field, value)
    for field, value in (("threshold_q", 0), ("threshold_q", 1024), ("onset_weight", 0), ("onset_weight", 16)):
        assert call(good, align.align_params(**{field: value})) == _native.BP_OK, (field, value)
    bad_index = C.c_int64(-1)
    lib.bp_internal_align_bad_states.restype = C.c_char_p
    lib.bp_internal_align_bad_states.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    for j in range(3):
        for what, edit in (("bit 88", lambda s: s["active"].__setitem__((j, 1), s["active"][j, 1] | np.uint64(1 << 24))),
                           ("bit 127 of begins", lambda s: s["begins"].__setitem__((j, 1), np.uint64(1 << 63))),
                           ("begins outside active", lambda s: s["begins"].__setitem__((j, 0), s["begins"][j, 0] | np.uint64(1 << 40))),
                           ("earliest < 0", lambda s: s["earliest"].__setitem__(j, -1)),
                           ("earliest > latest", lambda s: (s["earliest"].__setitem__(j, 5), s["latest"].__setitem__(j, 4)))):
            st = good.copy()
            edit(st)
            assert call(st, ok) == _native.BP_ERR_INVALID_ARG, (j, what)
            why = lib.bp_internal_align_bad_states(st.ctypes.data, 3, C.byref(bad_index))
            assert why and bad_index.value == j, (j, what)  # the state is named by its index
            with pytest.raises(ValueError):
                align.align_rows(note, onset, st)
    assert lib.bp_internal_align_bad_states(good.ctypes.data, 3, C.byref(bad_index)) is None
    # the other arguments
    assert call(good, ok, rows=-1) == _native.BP_ERR_INVALID_ARG and call(good, ok, n=-1) == _native.BP_ERR_INVALID_ARG
    assert call(good, ok, room=2) == _native.BP_ERR_INVALID_ARG and call(good, ok, n=0) == _native.BP_ERR_INVALID_ARG  # rows without a state
    assert call(good, ok, note_p=None) == _native.BP_ERR_INVALID_ARG and call(good, ok, ff_p=None) == _native.BP_ERR_INVALID_ARG
    assert call(good, ok, total_p=None) == _native.BP_ERR_INVALID_ARG and call(good, ok, status_p=None) == _native.BP_ERR_INVALID_ARG
    many = AC.make_states([[1]] * (align.MAX_STATES + 1))
    big = np.zeros(align.MAX_STATES + 1, np.int32)
    assert call(many, ok, room=len(big), ff_p=big.ctypes.data) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_align_rows(None, None, 0, None, 0, C.addressof(ok), None, 0, C.byref(total), C.byref(status)) == _native.BP_OK
    assert (total.value, status.value) == (0, 0)


# ---- the Python layer
def _golden():
    z = np.load(os.path.join(GOLDEN, "vocadito_10_note_events.npz"))
    notes = np.stack([z["start_s"], z["end_s"], z["pitch"].astype(np.float64)], axis=1)
    maps = np.load(os.path.join(GOLDEN, "vocadito_10_model_output.npz"))
    return notes, maps["note"], maps["onset"]


def test_states_and_notes_round_trip_on_the_golden_events(lib):
    from basic_pitch_amd import align
    from basic_pitch_amd.note_creation import frames_to_time_at

    notes, note, onset = _golden()
    n_frames = len(note)
    assert len(notes) == 28 and n_frames == 787
    states, first, after = align.states_from_notes(notes, n_frames)
    bounds = np.unique(notes[:, :2])
    assert len(states) == len(bounds) + 1 and not states["active"][0].any() and not states["active"][-1].any()
    act, beg = AC.rolls(states)
    for i, (s, e, q) in enumerate(notes):
        col = int(q) - 21
        assert act[first[i]:after[i], col].all() and beg[first[i], col] == 1 and after[i] > first[i]
        assert bounds[first[i] - 1] == s and bounds[after[i] - 1] == e
    assert act.sum() == sum(after - first) and beg.sum() == 28  # (no two golden notes of one pitch overlap)
    assert np.all(states["earliest"] == 0) and np.all(states["latest"] == align.FREE)
    # the events' own boundaries are frame times: the frames nearest to them give the events back exactly
    ff = np.concatenate([[0], align.nearest_frame(bounds, n_frames)])
    assert np.array_equal(frames_to_time_at(ff[1:]), bounds)
    back = align.notes_from_frames(notes, first, after, ff, n_frames)
    assert back.tobytes() == notes.tobytes()
    # without the silence states the indices move by one and the last note ends at n_frames itself
    bare, first0, after0 = align.states_from_notes(notes, n_frames, lead=False, tail=False)
    assert len(bare) == len(bounds) - 1 and np.array_equal(first0, first - 1) and bare.tobytes() == states[1:-1].tobytes()
    ends = align.notes_from_frames(notes, first0, after0, ff[1:-1], n_frames)[:, 1]
    assert ends[after0 == len(bare)].tolist() == [float(frames_to_time_at(np.array([n_frames]))[0])] * int((after0 == len(bare)).sum())
    # windows: the boundary's own frame -+ the frames of the shift, clipped; a zero shift is the frame itself
    held = align.states_from_notes(notes, n_frames, max_shift_s=0.0)[0]
    assert np.array_equal(held["earliest"][1:], ff[1:]) and np.array_equal(held["latest"][1:], ff[1:])
    assert (held["earliest"][0], held["latest"][0]) == (0, align.FREE)
    wide = align.states_from_notes(notes, n_frames, max_shift_s=0.5)[0]
    assert np.all(wide["earliest"][1:] <= ff[1:]) and np.all(wide["latest"][1:] >= ff[1:]) and wide["latest"][1:].max() <= n_frames - 1
    assert np.all(ff[1:] - wide["earliest"][1:] <= 44) and np.all(wide["latest"][1:] - ff[1:] <= 44) and wide["earliest"].min() == 0
    for bad in ([[0.0, 1.0, 20.4]], [[0.0, 1.0, 108.6]]):
        with pytest.raises(ValueError, match="note 0"):
            align.states_from_notes(bad, 10)
    assert align.states_from_notes([[0.0, 1.0, 20.6], [0.5, 1.5, 108.4]], 10)[0]["active"][2].tolist() == [1, 1 << 23]


def test_the_states_do_not_depend_on_a_shift_or_stretch_of_the_reference_times(lib):
    from basic_pitch_amd import align

    notes, _, _ = _golden()
    base = align.states_from_notes(notes, 787)
    for scale, shift in ((1.0, 3.0), (2.0, 0.0), (0.5, -1.0), (4.0, 100.0)):  # (powers of two: distinct times stay distinct)
        moved = notes.copy()
        moved[:, :2] = moved[:, :2] * scale + shift
        got = align.states_from_notes(moved, 787)
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), (scale, shift)


def test_aligning_the_golden_maps_to_the_golden_events_runs_to_status_0(lib):
    """The decoder's boundaries are no ground truth, so how near the aligned onsets land is information (profiles/align.md),
    not a gate: the gate is status 0, a monotone path, and the checker equal to the restatement."""
    from basic_pitch_amd import align

    notes, note, onset = _golden()
    order = np.argsort(notes[:, 0], kind="stable")
    states, first, after = align.states_from_notes(notes, len(note))
    got = align.align_rows(note, onset, states)
    _check(got, AC.restate(note, onset, states), "golden")
    ff, total, status = got
    assert status == 0 and ff[0] == 0 and np.all(np.diff(ff) > 0) and total > 0
    aligned = align.notes_from_frames(notes, first, after, ff, len(note))
    assert np.all(aligned[:, 1] > aligned[:, 0]) and np.array_equal(aligned[:, 2], notes[:, 2])
    assert np.all(np.diff(aligned[order, 0]) >= 0)
    near = int((np.abs(aligned[:, 0] - notes[:, 0]) <= 4.3 * 256 / 22050).sum())
    print(f"golden clip: {near} of 28 aligned onsets within 4.3 frames of the decoder's own")


# ---- the source alone, under the host sanitizers
def test_the_checker_links_without_a_device_and_runs_clean_under_the_sanitizers(tmp_path):
    """tests/test_melody_cpu.py's pattern: the checker's source and tools/sanitize/align_host.cpp, plain g++, once with
    -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "align_host.cpp"), os.path.join(ROOT, "basic_pitch_amd", "csrc", "align_host.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"align_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("align 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["aligned"]) > 80 and int(sums["flagged"]) > 0 and int(sums["infeasible"]) > 0 and int(sums["refused"]) >= 200
    assert int(sums["states"]) > 1000
