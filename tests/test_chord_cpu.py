"""Chords and key, the part that needs no GPU (include/basic_pitch_amd_chord.h): the header's symbols are exported by both
libraries with the prototypes it declares, the structures are the bytes it says, the host checker bp_chord_rows gives what an
independent restatement gives (tests/chord_cases.py: numpy int64) on seeded maps under every parameter set and boundary list,
boundaries at every frame give the result without boundaries, the best of ALL state sequences of small problems, planted triads
and scales; the three default tables; the statuses and the refusals; the checker's source under the host sanitizers as a program
of its own.  The calls that take a handle are in tests/test_gpu_chord.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import chord_cases as CC
from conftest import ROOT

NEW = ("bp_chord_params_default", "bp_chord_templates", "bp_chord_key_profiles", "bp_chord_rows", "bp_chords_from_maps", "bp_infer_clips_chords")
SHORTEST_RUN = 22  # the header's notes: planted triads come back exactly from this run length on


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, chord

    build.build_library()
    return chord.bind(_native.load_library())


_SCALAR = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "bp_handle": C.c_void_p, "void": None}


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
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_chord.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _same(got, want, where):
    """(summary, labels) of the checker against the restatement's, as bytes."""
    assert got[0].dtype == CC.SUMMARY and got[0].tobytes() == want[0].tobytes(), (where, got[0], want[0])
    assert got[1].dtype == np.uint8 and got[1].tobytes() == want[1].tobytes(), (where, got[1][:16], want[1][:16])


# ---- header and ABI
def test_every_symbol_of_the_chord_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, chord
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_beat.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(chord.PROTOTYPES) == set(_native.CHORD_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert chord.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["p", "bound_offsets", "bounds", "summaries", "labels", "max_labels"]
    assert names("bp_chord_rows") == ["note", "rows", "p", "bounds", "n_bounds", "labels", "max_labels", "summary"]
    assert names("bp_chords_from_maps") == ["h", "n_segments", "row_offsets", "note", "mem_kind"] + tail
    assert names("bp_infer_clips_chords") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert names("bp_chord_templates") == ["vocabulary", "p"] and names("bp_chord_key_profiles") == ["p"]
    # the statements the header owes: unpinned, the definition line by line, the tie rules, the bounds, the known limits
    flat = " ".join(text.replace("*", " ").split())
    for said in ("UNPINNED against any third-party chord or key estimator", "EXACT INTEGER ARITHMETIC", "its pitch class is (p + 9) % 12, C = 0",
                 "c[t][k] = sum over p in min_pitch ... max_pitch with class k of max(q(note[t][p]) - threshold_q, 0)", "8 x 1024 = 2^13",
                 "[0, B_0), [B_0, B_1), ..., [B_{n-1}, rows)", "0 < B < rows", "cu[u][k] = sum of c[t][k] over the unit's frames", "below 2^32",
                 "m = floor(sum of c^2 / sum of c)", "contraharmonic mean", "m <= 2^13", "each in -1024 ... 1024", "are DATA",
                 "the library knows no chord names", "state 0 of a table is \"no chord\"",
                 "e[u][s] = len(u) bias[s] m + sum over k of weights[s][k] cu[u][k]", "below len(u) 2^28",
                 "pen[u] = len(u) switch_penalty m", "D[0][s] = e[0][s]", "first maximum of D[u-1][.] in ascending state order",
                 "STRICTLY GREATER", "Ties stay", "D[u][s] = e[u][s] + best", "2^19 2^28 = 2^47", "first maximum of D[last][.]",
                 "there is no capacity protocol", "Ctot[k] = sum over t of c[t][k]",
                 "K[j] = sum over k of key_profile[j / 12][(k - j % 12 + 12) % 12] Ctot[k]", "first maximum of K in ascending j",
                 "this is decided first", "sum of c = 0", "every label 0, key -1", "are not tuned", "ONE KEY per segment",
                 "no bass and no inversion", "octave-folded energy only", f"AT LEAST {SHORTEST_RUN} FRAMES", "(D + 2^48, 63 - s)",
                 "weight 12 - n on its tones and -n elsewhere", "6.35 2.23 3.48 2.33 4.38 4.09 2.52 5.19 2.39 3.66 2.29 2.88",
                 "6.33 2.68 3.52 5.38 2.60 3.53 2.54 4.75 3.98 2.69 3.34 3.17", "rounded by lrint", "NO BARRIER", "nothing is written",
                 "the layout of beats / beat_offsets of bp_beats_from_maps", "the segment is named"):
        assert said in flat, said
    for macro, value in (("BP_CHORD_MAX_STATES", chord.MAX_STATES), ("BP_CHORD_CLASSES", chord.CLASSES), ("BP_CHORD_PITCHES", chord.PITCHES),
                         ("BP_CHORD_Q_ONE", chord.Q_ONE), ("BP_CHORD_MAX_WEIGHT", chord.MAX_WEIGHT), ("BP_CHORD_MAX_PENALTY", chord.MAX_PENALTY),
                         ("BP_CHORD_MAX_ROWS", chord.MAX_ROWS), ("BP_CHORD_CHROMA_ROWS", chord.CHROMA_ROWS), ("BP_CHORD_TRACE_TILE", chord.TRACE_TILE),
                         ("BP_CHORD_PATH_WAVES", chord.PATH_WAVES), ("BP_CHORD_VOCAB_MAJMIN", 0), ("BP_CHORD_VOCAB_TRIADS", 1),
                         ("BP_CHORD_VOCAB_SEVENTHS", 2)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert [v[0] for v in chord.VOCABULARIES.values()] == [0, 1, 2] and chord.CHORD_SUMMARY == CC.SUMMARY
    # the bounds the header states
    assert 8 * 1024 == 2 ** 13 and 2 ** 13 * (2 ** 19 - 1) < 2 ** 32 and 12 * 2 ** 26 * 2 ** 19 < 2 ** 49
    assert 2 ** 23 + 12 * 2 ** 10 * 2 ** 13 < 2 ** 28 and 2 ** 19 * 2 ** 28 == 2 ** 47 and 12 * 2 ** 10 * 2 ** 13 * 2 ** 19 < 2 ** 46
    assert ((2 ** 47 + 2 ** 48) << 6) + 63 < 2 ** 64
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.BEAT_SYMBOLS) | set(_native.ALIGN_SYMBOLS) | set(_native.MELODY_SYMBOLS) | set(_native.MULTIPITCH_SYMBOLS) | \
        set(_native.FRAME_SCORE_SYMBOLS) | set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | \
        set(_native.EXPORTED_SYMBOLS) | set(_native.FLAC_CLIPS_SYMBOLS) | set(_native.CONTAINERS_SYMBOLS) | set(_native.ADPCM_SYMBOLS)
    assert not set(NEW) & old and len(_native.BEAT_SYMBOLS) == 6 and len(_native.ALIGN_SYMBOLS) == 4
    assert os.path.basename(build.CHORD_HEADER) == "basic_pitch_amd_chord.h" and build.CHORD_HEADER in build.HEADERS
    assert {"chord.hip", "chord_host.cpp", "clips_chord.hip"} <= set(build.SOURCES)
    for entry in ("chords", "transcribe_clips_chords"):
        assert hasattr(Model, entry), entry
    unpinned = open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()
    assert "basic_pitch_amd_chord.h" in unpinned and "third-party chord or key estimator" in unpinned
    assert "basic_pitch_amd_chord.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "write_lab" in chord.__doc__


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, chord

    text, header = _header()
    sizes = {"BP_CHORD_MAX_STATES": 64, "BP_CHORD_CLASSES": 12}
    for name, size in (("bp_chord_params", 3456), ("bp_chord_summary", 32)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = []
        for t, decl in re.findall(r"\b(int32_t|int64_t)\s+([a-zA-Z_0-9, \[\]]+);", body):
            for n in decl.split(","):
                field, dims = re.fullmatch(r"\s*([a-z_]+)((?:\[[A-Z_0-9]+\])*)\s*", n).groups()
                ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}[t]
                for d in reversed(re.findall(r"\[([A-Z_0-9]+)\]", dims)):
                    ctype = ctype * int(sizes.get(d, d))
                fields.append((field, ctype))
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, (name, fields)
        assert f"/* {size} bytes */" in text
    assert chord.CHORD_SUMMARY.itemsize == 32 and [chord.CHORD_SUMMARY.fields[n][1] for n in chord.CHORD_SUMMARY.names] == [0, 4, 8, 12, 16, 24]
    p = chord.chord_params()
    assert (p.threshold_q, p.min_pitch, p.max_pitch, p.n_states, p.switch_penalty, list(p.reserved)) == (307, 0, 87, 25, 128, [0, 0, 0])
    assert chord.chord_params(switch_penalty=9).switch_penalty == 9 and chord.chord_params(dict(threshold_q=5)).threshold_q == 5
    assert chord.chord_params(vocabulary="sevenths").n_states == 61 and chord.chord_params(vocabulary="sevenths").names[-1] == "B:min7"
    own = chord.chord_params(CC.PARAM_SETS["two_states"])
    assert own.n_states == 2 and list(own.bias)[:3] == CC.PARAM_SETS["two_states"]["bias"][:3].tolist() and own.names[:3] == ["N", "1", "2"]
    assert [list(r) for r in own.weights][:2] == CC.PARAM_SETS["two_states"]["weights"][:2].tolist() and not any(list(own.weights[2]))
    with pytest.raises(TypeError):
        chord.chord_params(threshold=1)
    with pytest.raises(TypeError):
        chord.chord_params(vocabulary="triads", n_states=3)
    with pytest.raises(ValueError):
        chord.chord_params(vocabulary="jazz")


# ---- the three default tables and the profiles
def test_the_three_default_tables_and_the_key_profiles(lib):
    from basic_pitch_amd import _native, chord

    for vocabulary, n in (("majmin", 25), ("triads", 49), ("sevenths", 61)):
        p = chord.chord_params(vocabulary=vocabulary)
        want_n, bias, weights, names = CC.templates(vocabulary)
        assert p.n_states == n == want_n and len(names) == n and chord.chord_names(vocabulary) == names == p.names
        assert list(p.bias) == bias.tolist() and [list(r) for r in p.weights] == weights.tolist()
        table = np.array([list(r) for r in p.weights])
        assert not table.sum(axis=1).any() and not table[0].any() and not table[n:].any() and p.bias[0] == 12 and not any(list(p.bias)[1:])
        assert names[0] == "N" and names[1] == "C:maj" and names[12] == "B:maj" and names[13] == "C:min" and names[22] == "A:min"
    names = chord.chord_names("sevenths")
    assert names[1 + 24 + 7] == "G:7" and names[1 + 36] == "C:maj7" and names[60] == "B:min7" and chord.chord_names("triads")[25] == "C:dim"
    c_major = [list(r) for r in chord.chord_params().weights][1]
    assert c_major == [9, -3, -3, -3, 9, -3, -3, 9, -3, -3, -3, -3]
    g7 = [list(r) for r in chord.chord_params(vocabulary="sevenths").weights][1 + 24 + 7]
    assert [k for k, w in enumerate(g7) if w == 8] == [2, 5, 7, 11] and sorted(set(g7)) == [-4, 8]
    profile = np.array([list(r) for r in chord.chord_params().key_profile])
    want = CC.key_profiles()
    assert np.abs(profile - want).max() <= 1 and np.abs(profile.sum(axis=1)).max() <= 6  # (mean removed, then rounded)
    assert abs(float((profile[0].astype(float) ** 2).sum()) ** 0.5 - 1024) < 2 and profile[0].argmax() == 0 and profile[1].argmax() == 0
    assert len(chord.KEY_NAMES) == 24 and chord.KEY_NAMES[0] == "C major" and chord.KEY_NAMES[21] == "A minor"
    q = _native.bp_chord_params()
    assert lib.bp_chord_templates(3, C.addressof(q)) == lib.bp_chord_templates(-1, C.addressof(q)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_chord_templates(0, None) == lib.bp_chord_key_profiles(None) == _native.BP_ERR_INVALID_ARG


# ---- the checker against the restatement
@pytest.mark.parametrize("name", list(CC.PARAM_SETS))
def test_the_checker_equals_the_numpy_restatement_on_seeded_maps(lib, name):
    from basic_pitch_amd import chord

    fields = CC.PARAM_SETS[name]
    rng = np.random.default_rng(sorted(CC.PARAM_SETS).index(name))
    seen = {0: 0, 1: 0, 2: 0}
    changes = 0
    for kind, make in CC.KINDS.items():
        for rows in (1, 2, 33, 150):
            note = make(rng, rows)
            for how, bounds in (("none", None), ("one", [rows // 2] if rows > 1 else None), ("irregular", CC.irregular(rng, rows))):
                want = CC.restate(note, bounds, **fields)
                _same(chord.chord_rows_raw(note, fields, bounds), want, (name, kind, rows, how))
                seen[int(want[0]["status"][0])] += 1
                changes += int(want[0]["n_changes"][0])
    note = CC.noise(rng, 90)
    note[57, 3] = np.nan  # (a pitch outside the band of one_pitch: whatever pitch)
    _same(chord.chord_rows_raw(note, fields, [10, 57]), CC.restate(note, [10, 57], **fields), (name, "a NaN"))
    assert CC.restate(note, **fields)[0]["status"][0] == 1
    if name == "threshold_1024":
        assert seen[0] == 0 and seen[2] == 72
    else:
        assert seen[0] >= 30 and seen[2] >= 12, seen  # (of 72: silence is 12, everything under the default threshold 12 more)
        assert changes > 0 or name in ("one_state", "penalty_1024"), name


def test_the_plateaux_meet_every_tie_rule(lib):
    """Count the ties in the restatement's own numbers, so the comparison is known to have met each rule: equal D at the first
    maximum, D[a] - pen equal to D[s] (ties stay), and an equal last maximum."""
    from basic_pitch_amd import chord

    rng = np.random.default_rng(5)
    top_ties = stay_ties = end_ties = 0
    for case in range(24):
        note = CC.plateaux(rng, 120) if case % 6 != 5 else CC.major_minor_tie(case % 12, 120)  # (four maps whose last maximum ties)
        fields = dict(switch_penalty=(0, 1, 8, 128)[case % 4], threshold_q=128 * (case % 3))
        bounds = CC.irregular(rng, 120) if case % 2 else None
        p = CC.full(fields)
        found = CC.emissions(note, bounds, p)
        if found is None:
            continue
        e, pen = found[0], found[1]
        D = e[0].copy()
        for u in range(1, len(e)):
            top_ties += int((D == D.max()).sum() > 1)
            over = D.max() - pen[u]
            stay_ties += int(((over == D) & (np.arange(len(D)) != int(np.argmax(D)))).any())
            D = e[u] + np.where(over > D, over, D)
        end_ties += int((D == D.max()).sum() > 1)
        _same(chord.chord_rows_raw(note, fields, bounds), CC.restate(note, bounds, **fields), case)
    assert top_ties >= 100 and stay_ties >= 20 and end_ties >= 4, (top_ties, stay_ties, end_ties)


def test_the_quantisation_clamps_and_rounds_as_the_header_says(lib):
    """One pitch in the band, threshold 0, one state of weight 1 on the pitch's class: the score is q(x)."""
    from basic_pitch_amd import chord

    weights = np.zeros((1, 12), np.int64)
    weights[0, (40 + 9) % 12] = 1
    table = dict(n_states=1, bias=[0], weights=weights, threshold_q=0, min_pitch=40, max_pitch=40)
    for x, q in ((1.0, 1024), (7.5, 1024), (0.5, 512), (0.00048828125, 1), (0.3, 307), (np.inf, 1024), (1023.5 / 1024.0, 1024),
                 (1023.4 / 1024.0, 1023)):
        note = np.zeros((1, 88), np.float32)
        note[0, 40] = x
        s, labels = chord.chord_rows_raw(note, table)
        assert (int(s["status"][0]), int(s["score"][0]), int(s["n_units"][0])) == (0, q, 1) and int(CC.quantise(np.float32(x))) == q, x
    for x in (0.0, -3.0, 0.000487, -np.inf):  # q(x) = 0: nothing sounds
        note = np.zeros((1, 88), np.float32)
        note[0, 40] = x
        assert int(chord.chord_rows_raw(note, table)[0]["status"][0]) == 2, x
    # the pitch classes: pitch p is MIDI 21 + p, class (p + 9) % 12 — pitch 39 is MIDI 60, a C
    for pitch in (0, 3, 39, 50, 87):
        note = np.zeros((2, 88), np.float32)
        note[:, pitch] = 1.0
        weights = np.zeros((12, 12), np.int64)
        weights[np.arange(12), np.arange(12)] = 1
        s, labels = chord.chord_rows_raw(note, dict(n_states=12, bias=np.zeros(12), weights=weights, threshold_q=0))
        assert labels.tolist() == [(pitch + 21) % 12] * 2, pitch


# ---- boundaries at every frame are no boundaries
@pytest.mark.parametrize("name", ["default", "penalty_0", "random_64", "two_states"])
def test_boundaries_at_every_frame_give_the_result_without_boundaries(lib, name):
    from basic_pitch_amd import chord

    fields = CC.PARAM_SETS[name]
    rng = np.random.default_rng(17)
    for kind in ("noise", "plateaux", "triads", "infinities"):
        for rows in (2, 3, 64, 200):
            note = CC.KINDS[kind](rng, rows)
            plain = chord.chord_rows_raw(note, fields)
            every = chord.chord_rows_raw(note, fields, list(range(1, rows)))
            assert plain[0].tobytes() == every[0].tobytes() and plain[1].tobytes() == every[1].tobytes(), (name, kind, rows)
            assert int(plain[0]["n_units"][0]) == rows


# ---- every state sequence of small problems
def test_the_best_of_all_state_sequences_of_small_problems(lib):
    """At most 5 states and 7 units, with and without boundaries: the checker's path is THE best sequence — the inputs are
    random levels, and the uniqueness of the maximum is asserted, so no tie rule takes part."""
    from basic_pitch_amd import chord

    rng = np.random.default_rng(21)
    with_bounds = switched = 0
    for case in range(60):
        n = int(rng.integers(2, 6))
        fields = dict(CC.random_table(100 + case, n), switch_penalty=int(rng.choice([0, 3, 40, 300])), threshold_q=int(rng.choice([0, 128, 307])))
        fields["bias"] = fields["bias"] // 64  # (so that the emissions, not the biases, decide)
        if case % 2:
            units = int(rng.integers(2, 8))
            lens = rng.integers(1, 5, units)
            rows, bounds = int(lens.sum()), np.cumsum(lens)[:-1].tolist()
            with_bounds += 1
        else:
            rows, bounds = int(rng.integers(1, 8)), None
        note = rng.uniform(0.0, 1.0, (rows, 88)).astype(np.float32)
        want = CC.best_by_enumeration(note, bounds, **fields)
        assert want is not None and len(want[1]) == 1, (case, "the best sequence is not unique")
        summary, labels = chord.chord_rows_raw(note, fields, bounds)
        _same((summary, labels), CC.restate(note, bounds, **fields), ("the restatement", case))
        edges = CC.unit_edges(rows, bounds)
        assert int(summary["score"][0]) == want[0] and labels[edges[:-1]].tolist() == want[1][0], (case, labels, want)
        assert int(summary["n_changes"][0]) == int((np.diff(want[1][0]) != 0).sum())
        switched += int(summary["n_changes"][0]) > 0
    assert with_bounds == 30 and switched >= 15, (with_bounds, switched)


# ---- planted chords and keys
@pytest.mark.parametrize("seed", range(20))
def test_planted_triads_come_back_exactly_from_the_shortest_run_on(lib, seed):
    from basic_pitch_amd import chord

    for run in (SHORTEST_RUN, SHORTEST_RUN + 1, 40):
        note, states = CC.planted(seed, run)
        got = chord.chord_rows(note)
        assert got.status == 0 and got.labels.tolist() == states.tolist(), (seed, run)
        assert (got.labels[states == 0] == 0).all() and (states == 0).any()  # silence reads as state 0
        names = chord.chord_names()
        assert [r[2] for r in got.runs] == [names[s] for s in states[::run]] and got.n_changes == len(got.runs) - 1
        _same(chord.chord_rows_raw(note), CC.restate(note), (seed, run))
    note, states = CC.planted(seed, SHORTEST_RUN - 1)  # one frame less: the silence between the two equal chords is passed over
    assert chord.chord_rows(note).labels.tolist() != states.tolist(), seed


@pytest.mark.parametrize("key", range(24))
def test_planted_scales_give_their_key(lib, key):
    from basic_pitch_amd import chord

    note = CC.planted_scale(key)
    got = chord.chord_rows(note)
    assert got.status == 0 and got.key_index == key and got.key == chord.KEY_NAMES[key], (key, got.key)
    _same(chord.chord_rows_raw(note), CC.restate(note), key)
    with_beats = chord.chord_rows(note, bounds=[4, 5, 8])
    assert with_beats.key_index == key and with_beats.key_score == got.key_score  # the key does not depend on the units


# ---- statuses and refusals
def test_status_1_a_nan_in_whatever_pitch_and_status_2_nothing_sounds(lib, tmp_path):
    from basic_pitch_amd import chord
    from basic_pitch_amd.note_creation import frames_to_time_at

    rng = np.random.default_rng(31)
    note = CC.triads(rng, 120, 30)
    ok = chord.chord_rows(note)
    assert ok.status == 0 and ok.key is not None and ok.n_units == 120
    gone = lambda status: (status, -1, 0, 0, 0, 0)  # noqa: E731
    for row, pitch in ((0, 87), (57, 0), (119, 50)):
        bad = note.copy()
        bad[row, pitch] = np.nan
        for fields in (dict(), dict(min_pitch=10, max_pitch=20)):  # in the band or outside it
            s, labels = chord.chord_rows_raw(bad, fields, [60])
            assert s[0].tolist() == gone(1) and len(labels) == 120 and not labels.any(), (row, pitch, fields)
    # a NaN decides before silence does; an infinity is a value
    quiet = np.zeros((10, 88), np.float32)
    assert chord.chord_rows(quiet).status == 2
    quiet[3, 3] = np.nan
    assert chord.chord_rows(quiet).status == 1
    note[5, 5] = np.inf
    assert chord.chord_rows(note).status == 0
    for name, silent in (("no rows", note[:0]), ("silence", np.zeros((200, 88), np.float32)), ("under the threshold", np.full((200, 88), 0.29, np.float32))):
        s, labels = chord.chord_rows_raw(silent)
        assert s[0].tolist() == gone(2) and len(labels) == len(silent) and not labels.any(), name
    res = chord.chord_rows(note[:0])
    assert (res.status, res.key, res.runs, len(res.times_s), len(res.labels)) == (2, None, [], 0, 0)
    # the result object: runs, times and the .lab file
    assert ok.runs[0][0] == 0 and ok.runs[-1][1] == 120 and all(a[1] == b[0] for a, b in zip(ok.runs, ok.runs[1:]))
    assert np.array_equal(ok.times_s[:, 0], frames_to_time_at([r[0] for r in ok.runs])) and np.array_equal(ok.times_s[:, 1], frames_to_time_at([r[1] for r in ok.runs]))
    path = tmp_path / "a.lab"
    chord.write_lab(str(path), ok)
    lines = [line.split() for line in path.read_text().splitlines()]
    assert [line[2] for line in lines] == [r[2] for r in ok.runs] and all(len(line) == 3 and float(line[0]) < float(line[1]) for line in lines)
    # a beat at frame 0 is dropped in Python, a Beats object's frames are taken
    from basic_pitch_amd.beat import Beats

    beats = Beats(np.array([0, 30, 60, 90], np.int32), np.zeros(4), 30.0, 172.0, 0, 30, 1)
    assert chord.chord_rows(note, bounds=beats).n_units == 4 and chord.chord_rows(note, bounds=[30, 60, 90]).labels.tolist() == chord.chord_rows(note, bounds=beats).labels.tolist()


def test_every_malformed_argument_is_refused(lib):
    from basic_pitch_amd import _native, chord

    rng = np.random.default_rng(33)
    note = CC.triads(rng, 100, 30)
    labels = np.full(128, 77, np.uint8)
    summary = np.zeros(1, CC.SUMMARY)
    summary["status"] = 77
    good_bounds = np.array([10, 50], np.int32)

    def call(p, rows=100, note_p=note.ctypes.data, bounds=good_bounds, n_bounds=None, labels_p=labels.ctypes.data, room=100,
             summary_p=summary.ctypes.data):
        return lib.bp_chord_rows(note_p, rows, C.addressof(p) if p is not None else None, bounds.ctypes.data if bounds is not None else None,
                                 (len(bounds) if bounds is not None else 0) if n_bounds is None else n_bounds, labels_p, room, summary_p)

    ok = chord.chord_params()
    bad_sets = [("threshold_q", -1), ("threshold_q", 1025), ("min_pitch", -1), ("max_pitch", 88), ("n_states", 0), ("n_states", 65),
                ("switch_penalty", -1), ("switch_penalty", 1025), ("reserved", 1), ("reserved", (0, 1, 0)), ("reserved", (0, 0, 1))]
    for field, value in bad_sets:
        assert call(chord.chord_params(**{field: value})) == _native.BP_ERR_INVALID_ARG, (field, value)
        with pytest.raises(ValueError):
            chord.chord_rows(note, **{field: value})
    assert call(chord.chord_params(min_pitch=50, max_pitch=49)) == _native.BP_ERR_INVALID_ARG
    for value in (-1025, 1025):
        for s, k in ((0, 0), (24, 11), (63, 5)):  # (also beyond n_states: the whole table is held to the bound)
            table = np.zeros((64, 12), np.int64)
            table[s, k] = value
            assert call(chord.chord_params(weights=table, n_states=25)) == _native.BP_ERR_INVALID_ARG, (s, k, value)
            bias = np.zeros(64, np.int64)
            bias[s] = value
            assert call(chord.chord_params(bias=bias, n_states=25)) == _native.BP_ERR_INVALID_ARG, (s, value)
        profile = np.zeros((2, 12), np.int64)
        profile[1, 7] = value
        assert call(chord.chord_params(key_profile=profile)) == _native.BP_ERR_INVALID_ARG, value
    assert call(None) == call(ok, rows=-1) == call(ok, rows=chord.MAX_ROWS + 1) == call(ok, note_p=None) == _native.BP_ERR_INVALID_ARG
    assert call(ok, summary_p=None) == call(ok, labels_p=None) == call(ok, room=99) == call(ok, room=-1) == _native.BP_ERR_INVALID_ARG
    assert call(ok, n_bounds=-1) == call(ok, bounds=None, n_bounds=2) == _native.BP_ERR_INVALID_ARG
    for bad in ([0, 50], [10, 10], [50, 10], [10, 100], [-1, 10], [10, 50, 101]):
        assert call(ok, bounds=np.array(bad, np.int32)) == _native.BP_ERR_INVALID_ARG, bad
        with pytest.raises(ValueError):
            chord.chord_rows_raw(note, None, bad)
    assert np.all(labels == 77) and summary["status"][0] == 77, "a refused call wrote to its outputs"
    for field, value in (("threshold_q", 0), ("threshold_q", 1024), ("switch_penalty", 0), ("switch_penalty", 1024), ("n_states", 1),
                         ("n_states", 64), ("min_pitch", 87), ("max_pitch", 0)):
        assert call(chord.chord_params(**{field: value})) == _native.BP_OK, (field, value)
    for good in ([1], [99], [1, 2, 3], list(range(1, 100))):
        assert call(ok, bounds=np.array(good, np.int32)) == _native.BP_OK, good
    labels[:] = 77
    assert call(ok) == _native.BP_OK and summary["status"][0] == 0 and summary["n_units"][0] == 3 and np.all(labels[100:] == 77)
    assert lib.bp_chord_rows(None, 0, C.addressof(ok), None, 0, None, 0, summary.ctypes.data) == _native.BP_OK and summary["status"][0] == 2
    # the reason a device call gives names the field
    lib.bp_internal_chord_bad_params.restype = C.c_char_p
    lib.bp_internal_chord_bad_params.argtypes = [C.c_void_p]
    for field, value in bad_sets:
        bad = chord.chord_params(**{field: value})
        why = lib.bp_internal_chord_bad_params(C.addressof(bad)).decode()
        assert field.split("_")[0] in why, (field, why)
    assert lib.bp_internal_chord_bad_params(C.addressof(ok)) is None
    with pytest.raises(ValueError):
        chord.chord_rows(np.zeros((4, 87), np.float32))


# ---- the source alone, under the host sanitizers
def test_the_checker_links_without_a_device_and_runs_clean_under_the_sanitizers(tmp_path):
    """tests/test_beat_cpu.py's pattern: the checker's source and tools/sanitize/chord_host.cpp, plain g++, once with
    -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "chord_host.cpp"), os.path.join(ROOT, "basic_pitch_amd", "csrc", "chord_host.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"chord_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("chord 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["decoded"]) > 60 and int(sums["flagged"]) > 0 and int(sums["silent"]) > 20 and int(sums["refused"]) >= 400
    assert int(sums["changes"]) > 500 and int(sums["units"]) > 5000
