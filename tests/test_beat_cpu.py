"""Tempo and beats, the part that needs no GPU (include/basic_pitch_amd_beat.h): the header's symbols are exported by both
libraries with the prototypes it declares, the structures are the bytes it says, the host checker bp_beat_rows gives what an
independent restatement gives (tests/beat_cases.py: numpy int64) on seeded maps under several parameter sets, the best of ALL
beat sequences of small problems under the header's tie rule, and the planted beats of planted problems; the invariants on
the golden clip; the prior helper; the statuses and the refusals; the checker's source under the host sanitizers as a program of
its own.  The calls that take a handle are in tests/test_gpu_beat.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import beat_cases as BC
from conftest import GOLDEN, ROOT

NEW = ("bp_beat_params_default", "bp_beat_prior", "bp_beats_capacity", "bp_beat_rows", "bp_beats_from_maps", "bp_infer_clips_beats")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, beat, build

    build.build_library()
    return beat.bind(_native.load_library())


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
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_beat.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _same(got, want, where):
    """(summary, beats) of the checker against the restatement's: the summaries as bytes, the beats as lists."""
    assert got[0].dtype == BC.SUMMARY and got[0].tobytes() == want[0].tobytes(), (where, got[0], want[0])
    assert got[1].dtype == np.int32 and got[1].tolist() == list(want[1]), (where, got[1][:8], want[1][:8])


# ---- header and ABI
def test_every_symbol_of_the_beat_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, beat, build
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_align.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(beat.PROTOTYPES) == set(_native.BEAT_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert beat.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["p", "summaries", "beats", "max_beats", "beat_offsets"]
    assert names("bp_beat_rows") == ["onset", "rows", "p", "beats", "max_beats", "summary"]
    assert names("bp_beats_from_maps") == ["h", "n_segments", "row_offsets", "onset", "mem_kind"] + tail
    assert names("bp_infer_clips_beats") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    assert names("bp_beat_prior") == ["start_bpm", "sd_octaves", "prior"] and names("bp_beats_capacity") == ["rows", "lag_min"]
    # the statements the header owes: unpinned, the definition line by line, the tie rules, the bounds, the known limits
    flat = " ".join(text.replace("*", " ").split())
    for said in ("UNPINNED against librosa and mir_eval", "Ellis 2007", "EXACT INTEGER ARITHMETIC",
                 "o[t] = sum over p in min_pitch ... max_pitch of max(q(onset[t][p]) - threshold_q, 0)", "88 x 1024 = 90,112",
                 "L = lag_min ... min(lag_max, rows - 1)", "A[L] = sum over t = 0 ... rows-1-L of o[t] o[t+L]", "S[L] = A[L] prior[L]",
                 "ties go to the smallest lag", "lrint(1024 exp(-0.5 (log2(L / L0) / sd)^2))", "L0 = 60 22050 / 256 / start_bpm",
                 "entry 0 is 0", "m = floor(sum of o[t]^2 / sum of o[t])", "contraharmonic mean", "dmin = max(1, P / 2) and dmax = 2 P",
                 "pen[d] = floor(tightness m (d - P)^2 / (P P))", "C[t] = o[t] + best", "STRICTLY GREATER", "ties go to the start",
                 "[max(0, rows - P), rows)", "period_refined = P + 0.5 (l - r) / ((l - 2c) + r)", "lag_min < P < the last admissible lag",
                 "this is decided first", "rows - 1 < lag_min", "A[L] 1024 < 90,112^2 2^19 2^10 < 2^62", "< 2^40", "< 2^44",
                 "are not tuned", "ONE GLOBAL TEMPO", "are not trimmed", "lag 29 reads as period 58", "ONCE PER BLOCK",
                 "rows <= lag_min ? 0 : (rows - 1) / max(1, lag_min / 2) + 1", "nothing is written"):
        assert said in flat, said
    for macro, value in (("BP_BEAT_MAX_LAG", beat.MAX_LAG), ("BP_BEAT_PITCHES", beat.PITCHES), ("BP_BEAT_Q_ONE", beat.Q_ONE),
                         ("BP_BEAT_MAX_TIGHTNESS", beat.MAX_TIGHTNESS), ("BP_BEAT_MAX_ROWS", beat.MAX_ROWS), ("BP_BEAT_RING", beat.RING),
                         ("BP_BEAT_TEMPO_ROWS", beat.TEMPO_ROWS), ("BP_BEAT_TEMPO_LAGS", beat.TEMPO_LAGS), ("BP_BEAT_PATH_WAVES", beat.PATH_WAVES)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert beat.MAX_LAG == 256 == BC.MAX_LAG and beat.MAX_ROWS == 2 ** 19 and beat.RING >= 2 * beat.MAX_LAG + beat.MAX_LAG // 2
    assert 90112 ** 2 * 2 ** 19 * 2 ** 10 < 2 ** 62 and 2 ** 19 * 90112 < 2 ** 40 and 1024 * 90112 * beat.MAX_LAG ** 2 < 2 ** 44
    assert 2 * beat.MAX_LAG - beat.MAX_LAG // 2 + 1 == 385 <= 7 * 64 and beat.BEAT_SUMMARY == BC.SUMMARY
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.ALIGN_SYMBOLS) | set(_native.MELODY_SYMBOLS) | set(_native.MULTIPITCH_SYMBOLS) | set(_native.FRAME_SCORE_SYMBOLS) | \
        set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | set(_native.EXPORTED_SYMBOLS) | \
        set(_native.FLAC_CLIPS_SYMBOLS) | set(_native.CONTAINERS_SYMBOLS) | set(_native.ADPCM_SYMBOLS)
    assert not set(NEW) & old and len(_native.ALIGN_SYMBOLS) == 4 and len(_native.MELODY_SYMBOLS) == 7
    assert os.path.basename(build.BEAT_HEADER) == "basic_pitch_amd_beat.h" and build.BEAT_HEADER in build.HEADERS
    assert {"beat.hip", "beat_host.cpp"} <= set(build.SOURCES)
    for entry in ("beats", "transcribe_clips_beats"):
        assert hasattr(Model, entry), entry
    unpinned = open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()
    assert "basic_pitch_amd_beat.h" in unpinned and "librosa" in unpinned
    assert "basic_pitch_amd_beat.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "midi_tempo" in beat.__doc__


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, beat

    text, header = _header()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name, size in (("bp_beat_params", 1064), ("bp_beat_summary", 32)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = []
        for t, decl in re.findall(r"\b(int32_t|int64_t|double)\s+([a-zA-Z_0-9, +\[\]]+);", body):
            for n in decl.split(","):
                arr = re.fullmatch(r"\s*([a-z_]+)\[([A-Z_0-9 +]+)\]\s*", n)
                count = eval(arr.group(2).replace("BP_BEAT_MAX_LAG", "256")) if arr else 0
                fields.append((arr.group(1), ctype[t] * count) if arr else (n.strip(), ctype[t]))
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, (name, fields)
        assert f"/* {size} bytes */" in text
    assert beat.BEAT_SUMMARY.itemsize == 32 and [beat.BEAT_SUMMARY.fields[n][1] for n in beat.BEAT_SUMMARY.names] == [0, 4, 8, 16, 24]
    p = beat.beat_params()
    assert (p.threshold_q, p.min_pitch, p.max_pitch, p.lag_min, p.lag_max, p.tightness, list(p.reserved), p.reserved_tail) == \
        (307, 0, 87, 21, 172, 4, [0, 0], 0)
    assert beat.beat_params(tightness=9).tightness == 9 and beat.beat_params(dict(lag_min=5)).lag_min == 5
    assert list(beat.beat_params(prior=BC.FLAT).prior) == BC.FLAT.tolist()
    assert list(beat.beat_params(start_bpm=90.0).prior) == beat.beat_prior(90.0, 1.0).tolist()
    with pytest.raises(TypeError):
        beat.beat_params(threshold=1)
    with pytest.raises(TypeError):
        beat.beat_params(prior=BC.FLAT, start_bpm=100.0)


# ---- the prior helper
def test_the_prior_helper_is_the_formula_and_the_defaults_carry_the_default_table(lib):
    from basic_pitch_amd import _native, beat

    for bpm, sd in ((120.0, 1.0), (60.0, 0.5), (200.0, 2.0), (97.3, 0.25)):
        got, want = beat.beat_prior(bpm, sd), BC.prior_table(bpm, sd)
        assert got.dtype == np.int32 and got[0] == 0 and np.abs(got.astype(np.int64) - want).max() <= 1, (bpm, sd)
        assert got.min() >= 0 and got.max() <= 1024
    table = beat.beat_prior()
    assert list(beat.beat_params().prior) == table.tolist()
    assert int(np.argmax(table)) == 43 and table[43] == 1024 and table[29] < table[58]  # 120 a minute is 43.07 frames; the octave rule
    for bad in ((0.0, 1.0), (-1.0, 1.0), (120.0, 0.0), (np.nan, 1.0), (120.0, np.inf)):
        with pytest.raises(ValueError):
            beat.beat_prior(*bad)
    assert lib.bp_beat_prior(120.0, 1.0, None) == _native.BP_ERR_INVALID_ARG
    # the room: from the rows and lag_min alone
    for rows, lag_min, cap in ((0, 21, 0), (21, 21, 0), (22, 21, 3), (787, 21, 79), (5, 2, 5), (5, 3, 5), (12, 2, 12), (100, 256, 0), (300, 256, 3)):
        assert beat.beats_capacity(rows, lag_min) == cap == (0 if rows <= lag_min else (rows - 1) // max(1, lag_min // 2) + 1), (rows, lag_min)
    for bad in ((-1, 21), (10, 1), (10, 257)):
        with pytest.raises(ValueError):
            beat.beats_capacity(*bad)


# ---- the checker against the restatement
@pytest.mark.parametrize("name", list(BC.PARAM_SETS))
def test_the_checker_equals_the_numpy_restatement_on_seeded_maps(lib, name):
    from basic_pitch_amd import beat

    fields = BC.PARAM_SETS[name]
    rng = np.random.default_rng(sorted(BC.PARAM_SETS).index(name))
    seen = {0: 0, 1: 0, 2: 0}
    refined = 0
    for kind, make in BC.KINDS.items():
        for rows in (1, 20, 22, 44, 130, 300, 433):
            onset = make(rng, rows)
            want = BC.restate(onset, **fields)
            _same(beat.beat_rows_raw(onset, **fields), want, (name, kind, rows))
            seen[int(want[0]["status"][0])] += 1
            refined += float(want[0]["period_refined"][0]) != float(want[0]["period"][0])
    onset = BC.noise(rng, 90)
    onset[57, 3] = np.nan  # (a pitch outside the narrow band: whatever pitch)
    _same(beat.beat_rows_raw(onset, **fields), BC.restate(onset, **fields), (name, "a NaN"))
    assert BC.restate(onset, **fields)[0]["status"][0] == 1
    assert seen[0] >= 10 and seen[2] >= 7, seen  # (of 35 maps: 7 are silence, and the short ones lie under lag_min)
    assert refined > 0 or name == "one_lag", name


def test_the_quantised_maps_tie_in_the_lags_the_candidates_and_the_ending(lib):
    """The eighths maps are there for the ties: count them in the restatement's own numbers, so the comparison above is known
    to have met each rule."""
    from basic_pitch_amd import beat

    rng = np.random.default_rng(5)
    lag_ties = cand_ties = end_ties = 0
    for case in range(12):
        onset = BC.eighths(rng, 433, 1 + case % 3)
        fields = dict(tightness=case % 2 * 4, prior=BC.FLAT)  # (a flat prior: equal A are equal S)
        p = BC.full(fields)
        o = BC.strength(onset, p)
        P, S, last = BC.tempo(o, p)
        lag_ties += int(len(np.unique(S[p["lag_min"] : last + 1])) < last + 1 - p["lag_min"])
        summary, beats = BC.restate(onset, **fields)
        dmin, dmax, pen = BC.penalties(o, P, p)
        cand_ties += len(set(pen.values())) < len(pen)  # equal penalties at distinct gaps: equal candidates wherever C ties too
        end_ties += int((o[max(0, 433 - P):] == 0).any())
        assert summary["status"][0] == 0 and len(beats) >= 2
        _same(beat.beat_rows_raw(onset, **fields), (summary, beats), case)
    assert lag_ties >= 3 and cand_ties >= 6 and end_ties >= 6, (lag_ties, cand_ties, end_ties)  # (of 12 maps)
    # a tie AT the maximum: three equal pulses at 0, 30 and 70 make A[30] = A[40] = A[70], and the smallest lag is the period
    onset = np.zeros((90, 88), np.float32)
    onset[[0, 30, 70], 10] = 0.75
    summary, beats = beat.beat_rows_raw(onset, prior=BC.FLAT)
    assert (int(summary["period"][0]), int(summary["score"][0]), float(summary["period_refined"][0])) == (30, (768 - 307) ** 2 * 1024, 30.0)
    _same((summary, beats), BC.restate(onset, prior=BC.FLAT), "three pulses")
    assert beats.tolist() == [0, 30, 70]
    onset[[75, 80], 10] = 0.75  # two more equal pulses in the ending window, under the stiffest penalty
    summary, beats = beat.beat_rows_raw(onset, prior=BC.FLAT, tightness=1024)
    _same((summary, beats), BC.restate(onset, prior=BC.FLAT, tightness=1024), "five pulses")


def test_the_quantisation_clamps_and_rounds_as_the_header_says(lib):
    """One pitch in the band, threshold 0, a flat prior, two equal pulses one lag apart: the score is q(x)^2 * 1024."""
    from basic_pitch_amd import beat

    for x, q in ((1.0, 1024), (7.5, 1024), (0.5, 512), (0.00048828125, 1), (0.3, 307), (np.inf, 1024), (1023.5 / 1024.0, 1024),
                 (1023.4 / 1024.0, 1023)):
        onset = np.zeros((5, 88), np.float32)
        onset[1, 40] = onset[3, 40] = x
        s, b = beat.beat_rows_raw(onset, prior=BC.FLAT, threshold_q=0, lag_min=2, lag_max=3, min_pitch=40, max_pitch=40)
        assert (int(s["status"][0]), int(s["period"][0]), int(s["score"][0])) == (0, 2, q * q * 1024), x
        assert int(BC.quantise(np.float32(x))) == q and b.tolist() == [1, 3]
    for x in (0.0, -3.0, 0.000487, -np.inf):  # q(x) = 0: no pulse
        onset = np.zeros((5, 88), np.float32)
        onset[1, 40] = onset[3, 40] = x
        assert int(beat.beat_rows_raw(onset, prior=BC.FLAT, threshold_q=0, lag_min=2, lag_max=3)[0]["status"][0]) == 2, x


# ---- every beat sequence of small problems
def test_the_best_of_all_beat_sequences_under_the_tie_rule(lib):
    from basic_pitch_amd import beat

    rng = np.random.default_rng(21)
    shared = silent = 0
    for case in range(90):
        rows = int(rng.integers(3, 13))
        fields = dict(lag_min=2, lag_max=3, prior=BC.FLAT, threshold_q=int(rng.choice([0, 128, 256])), tightness=int(rng.choice([0, 1, 4, 64])))
        onset = BC.eighths(rng, rows, 2) if case % 5 else np.full((rows, 88), rng.integers(0, 9) / 8.0, np.float32)  # (all-equal maps too)
        want = BC.best_by_enumeration(onset, **fields)
        summary, beats = beat.beat_rows_raw(onset, **fields)
        _same((summary, beats), BC.restate(onset, **fields), ("the restatement", case))
        if want is None:
            assert summary["status"][0] == 2
            silent += 1
            continue
        top, chosen, n_ties = want
        p = BC.full(fields)
        o = BC.strength(onset, p)
        _, _, pen = BC.penalties(o, int(summary["period"][0]), p)
        value = int(o[beats].sum()) - sum(pen[int(g)] for g in np.diff(beats))  # the checker's C at its last beat
        assert value == top and beats.tolist() == chosen, (case, rows, beats, chosen)
        shared += n_ties > 1
    assert shared >= 10 and silent >= 2, (shared, silent)


# ---- planted beats
@pytest.mark.parametrize("seed", range(30))
def test_planted_beats_come_back_exactly_with_the_defaults(lib, seed):
    from basic_pitch_amd import beat

    onset, period, beats = BC.planted(seed)
    got = beat.beat_rows(onset)
    assert got.status == 0 and got.period == period, (seed, period, got.period)  # first: the period found is the planted one
    assert got.frames.tolist() == beats, (seed, period, len(onset))
    assert abs(got.period_frames - period) < 0.5 and abs(got.bpm - 60 * 22050 / 256 / got.period_frames) < 1e-9
    _same(beat.beat_rows_raw(onset), BC.restate(onset), seed)


def test_the_planted_problems_cover_their_range():
    sizes = [(BC.planted(s)[1], len(BC.planted(s)[0])) for s in range(30)]
    assert min(p for p, _ in sizes) <= 38 and max(p for p, _ in sizes) >= 57 and min(r for _, r in sizes) < 400 < 600 < max(r for _, r in sizes)


# ---- the golden clip
def test_the_invariants_hold_on_the_golden_clips_onset_map(lib):
    """A solo voice: no number is pinned."""
    from basic_pitch_amd import beat
    from basic_pitch_amd.note_creation import frames_to_time_at

    onset = np.load(os.path.join(GOLDEN, "vocadito_10_model_output.npz"))["onset"]
    got = beat.beat_rows(onset)
    p = beat.beat_params()
    assert got.status == 0 and p.lag_min <= got.period <= min(p.lag_max, len(onset) - 1)
    gaps = np.diff(got.frames)
    assert len(got.frames) >= 2 and np.all(gaps >= max(1, got.period // 2)) and np.all(gaps <= 2 * got.period)
    assert got.frames[0] >= 0 and len(onset) - got.period <= got.frames[-1] < len(onset)
    assert got.frames.dtype == np.int32 and np.array_equal(got.times_s, frames_to_time_at(got.frames))
    assert abs(got.period_frames - got.period) < 1.0 and got.bpm == 60 * 22050 / 256 / got.period_frames and got.score > 0
    _same(beat.beat_rows_raw(onset), BC.restate(onset), "golden")
    print(f"golden clip: period {got.period} frames ({got.bpm:.1f} a minute), {len(got.frames)} beats")


# ---- statuses and refusals
def test_status_1_a_nan_in_whatever_pitch_and_status_2_no_pulse(lib):
    from basic_pitch_amd import beat

    rng = np.random.default_rng(31)
    onset = BC.pulses(rng, 120, 40)
    assert beat.beat_rows(onset).status == 0
    gone = lambda status: (status, 0, 0, 0, 0.0)  # noqa: E731
    for row, pitch in ((0, 87), (57, 0), (119, 50)):
        bad = onset.copy()
        bad[row, pitch] = np.nan
        for fields in (dict(), dict(min_pitch=10, max_pitch=20)):  # in the band or outside it
            s, b = beat.beat_rows_raw(bad, **fields)
            assert s[0].tolist() == gone(1) and len(b) == 0, (row, pitch, fields)
    # a NaN decides before "too few rows" does; an infinity is a value
    short = onset[:10].copy()
    assert beat.beat_rows(short).status == 2
    short[3, 3] = np.nan
    assert beat.beat_rows(short).status == 1
    onset[5, 5] = np.inf
    assert beat.beat_rows(onset).status == 0
    # no pulse: no rows, rows - 1 < lag_min, silence, everything under the threshold; one row more than lag_min admits one lag
    for name, quiet in (("no rows", onset[:0]), ("lag_min rows", onset[:21]), ("silence", np.zeros((200, 88), np.float32)),
                        ("under the threshold", np.full((200, 88), 0.29, np.float32))):
        s, b = beat.beat_rows_raw(quiet)
        assert s[0].tolist() == gone(2) and len(b) == 0, name
    loud = np.full((22, 88), 0.5, np.float32)
    got = beat.beat_rows(loud)
    assert (got.status, got.period, got.period_frames) == (0, 21, 21.0)
    res = beat.Beats.of(beat.beat_rows_raw(onset[:0])[0][0], np.zeros(0, np.int32))
    assert (res.status, res.bpm, res.period_frames, len(res.times_s)) == (2, 0.0, 0.0, 0)


def test_every_malformed_argument_is_refused(lib):
    from basic_pitch_amd import _native, beat

    rng = np.random.default_rng(33)
    onset = BC.pulses(rng, 100, 30)
    beats = np.full(128, 77, np.int32)
    summary = np.zeros(1, BC.SUMMARY)
    summary["status"] = 77
    cap = beat.beats_capacity(100, 21)
    assert cap == 10

    def call(p, rows=100, onset_p=onset.ctypes.data, beats_p=beats.ctypes.data, room=None, summary_p=summary.ctypes.data):
        if room is None:  # what the set itself asks for (a malformed lag_min asks for nothing)
            room = max(0, lib.bp_beats_capacity(100, p.lag_min)) if p is not None else cap
        return lib.bp_beat_rows(onset_p, rows, C.addressof(p) if p is not None else None, beats_p, room, summary_p)

    ok = beat.beat_params()
    bad_sets = [("threshold_q", -1), ("threshold_q", 1025), ("min_pitch", -1), ("max_pitch", 88), ("lag_min", 1), ("lag_max", 257),
                ("tightness", -1), ("tightness", 1025), ("reserved", 1), ("reserved", (0, 1)), ("reserved_tail", 1)]
    for field, value in bad_sets:
        assert call(beat.beat_params(**{field: value})) == _native.BP_ERR_INVALID_ARG, (field, value)
        with pytest.raises(ValueError):
            beat.beat_rows(onset, **{field: value})
    assert call(beat.beat_params(min_pitch=50, max_pitch=49)) == call(beat.beat_params(lag_min=60, lag_max=59)) == _native.BP_ERR_INVALID_ARG
    for L in (0, 1, 100, 256):
        for value in (-1, 1025):
            table = BC.FLAT.copy()
            table[L] = value
            assert call(beat.beat_params(prior=table)) == _native.BP_ERR_INVALID_ARG, (L, value)
    assert call(None) == call(ok, rows=-1) == call(ok, rows=beat.MAX_ROWS + 1) == call(ok, onset_p=None) == _native.BP_ERR_INVALID_ARG
    assert call(ok, summary_p=None) == call(ok, beats_p=None) == call(ok, room=cap - 1) == call(ok, room=-1) == _native.BP_ERR_INVALID_ARG
    assert np.all(beats == 77) and summary["status"][0] == 77, "a refused call wrote to its outputs"
    for field, value in (("threshold_q", 0), ("threshold_q", 1024), ("tightness", 0), ("tightness", 1024), ("lag_min", 2), ("lag_max", 256),
                         ("min_pitch", 87), ("max_pitch", 0)):
        assert call(beat.beat_params(**{field: value})) == _native.BP_OK, (field, value)
    beats[:] = 77
    assert call(ok) == _native.BP_OK and summary["status"][0] == 0 and np.all(beats[int(summary["n_beats"][0]):] == 77)
    assert lib.bp_beat_rows(None, 0, C.addressof(ok), None, 0, summary.ctypes.data) == _native.BP_OK and summary["status"][0] == 2
    # the reason a device call gives names the field
    lib.bp_internal_beat_bad_params.restype = C.c_char_p
    lib.bp_internal_beat_bad_params.argtypes = [C.c_void_p]
    for field, value in bad_sets:
        bad = beat.beat_params(**{field: value})
        why = lib.bp_internal_beat_bad_params(C.addressof(bad)).decode()
        assert field.split("_")[0] in why, (field, why)
    assert lib.bp_internal_beat_bad_params(C.addressof(ok)) is None
    with pytest.raises(ValueError):
        beat.beat_rows(np.zeros((4, 87), np.float32))


# ---- the source alone, under the host sanitizers
def test_the_checker_links_without_a_device_and_runs_clean_under_the_sanitizers(tmp_path):
    """tests/test_align_cpu.py's pattern: the checker's source and tools/sanitize/beat_host.cpp, plain g++, once with
    -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "beat_host.cpp"), os.path.join(ROOT, "basic_pitch_amd", "csrc", "beat_host.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"beat_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("beat 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["decoded"]) > 60 and int(sums["flagged"]) > 0 and int(sums["silent"]) > 20 and int(sums["refused"]) >= 200
    assert int(sums["beats"]) > 500
