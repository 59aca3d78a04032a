"""Two recordings against each other, the part that needs no GPU (include/basic_pitch_amd_sync.h): the header's symbols are
exported by both libraries with the prototypes it declares, the structures are the bytes it says, the header says its
definition line by line, the host checker bp_sync_rows gives what an independent restatement gives (tests/sync_cases.py: numpy
int64 and Python integers) on seeded pairs under every hop, band and pitch band, the best of ALL monotone paths of small
problems and the path the tie order selects among the optimal ones, planted warps in both roles, a segment against itself, the
extremes of the feature, the statuses, the refusals, and the checker's source under the host sanitizers as a program of its
own.  The calls that take a handle are in tests/test_gpu_sync.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sync_cases as SC
from conftest import ROOT

NEW = ("bp_sync_params_default", "bp_sync_rows", "bp_sync_from_maps", "bp_infer_clips_sync")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, sync

    build.build_library()
    return sync.bind(_native.load_library())


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
    text = open(os.path.join(ROOT, "include", "basic_pitch_amd_sync.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _same(got, want, where):
    """(summary, path region) of the checker against the restatement's, as bytes."""
    assert got[0].dtype == SC.SUMMARY and got[0].tobytes() == want[0].tobytes(), (where, got[0], want[0])
    assert got[1].dtype == np.int32 and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), (where, got[1][:8], want[1][:8])


# ---- header and ABI
def test_every_symbol_of_the_sync_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, sync
    from basic_pitch_amd.inference import Model

    text, header = _header()
    assert '#include "basic_pitch_amd_chord.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(sync.PROTOTYPES) == set(_native.SYNC_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert sync.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    tail = ["n_pairs", "pairs", "p", "summaries", "path", "max_path"]
    assert names("bp_sync_rows") == ["note_a", "rows_a", "note_b", "rows_b", "p", "path", "max_path", "summary"]
    assert names("bp_sync_from_maps") == ["h", "n_segments", "row_offsets", "note", "mem_kind"] + tail
    assert names("bp_infer_clips_sync") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind"] + tail
    # the statements the header owes: unpinned, the definition line by line, the tie order, the bounds, the room, the limits
    flat = " ".join(text.replace("*", " ").split())
    for said in ("UNPINNED against any third-party alignment or time-warping implementation", "EXACT INTEGER ARITHMETIC",
                 "a == b is allowed", "exactly as basic_pitch_amd_chord.h defines it", "class (p + 9) % 12", "at most 2^13",
                 "Unit u is the frames [u hop, min((u + 1) hop, rows))", "U = ceil(rows / hop)", "at most 64 2^13 = 2^19",
                 "THE SMALLEST INTEGER WITH r r >= s, the ceiling root", "x[u][k] = floor(255 cu[u][k] / r)", "With s = 0 the unit is all zero",
                 "The ceiling root, not the floor root", "sum over k of x[u][k]^2 <= 255^2", "become (255, 255)", "they are (127, 127)",
                 "g(i, j) = sum over k of xa[i][k] xb[j][k]", "0 <= g <= 255^2 = 65,025", "Every cell when band == 0",
                 "|i (M - 1) - j (N - 1)| <= band max(N - 1, M - 1)", "in int64", "D[0][0] = 2 g(0, 0)",
                 "D[i][j] = max(D[i-1][j-1] + 2 g(i, j), D[i-1][j] + g(i, j), D[i][j-1] + g(i, j))",
                 "exist, are admissible and are reachable", "An inadmissible cell is unreachable", "the same total weight N + M",
                 "16,384 x 65,025 = 1,065,369,600 < 2^31", "D is int32", "Diagonal before (i-1, j) before (i, j-1)", "STRICTLY GREATER",
                 "From (N-1, M-1) back to (0, 0)", "in ascending order as int32 pairs", "max(N, M) <= n_path <= N + M - 1",
                 "in whatever pitch", "this is decided first", "a segment has no rows", "n_path and total are 0", "A silent unit is not a status",
                 "A BAND NEVER CUTS THE END OFF", "status 2 has no second cause", "There is no capacity protocol",
                 "Pair p owns N_p + M_p - 1 entries of path (0 when either segment has no rows)", "summary.path_first says where its region starts",
                 "past n_path are (-1, -1)", "max_path is checked against the sum before anything is queued",
                 "Both ends are fixed: there is no subsequence search", "ONE WORKGROUP A PAIR", "Octave-folded energy only", "are not tuned",
                 "A segment against ITSELF gives the pure diagonal when every unit has the same self-gain", "It is not a theorem of the definition",
                 "total (N + M) 65,025", "1024 lanes x 8 columns a lane", "no scratch and no spills", "nothing is written",
                 "Zero pairs is a call that does nothing", "the pair is named", "A segment that no pair names costs no device work",
                 "one barrier a step", "N + lanes in use - 1 steps", "three v_dot4_u32_u8", "[step][lane]", "12 feature bytes and 4 zero bytes"):
        assert said in flat, said
    for macro, value in (("BP_SYNC_MAX_UNITS", sync.MAX_UNITS), ("BP_SYNC_MAX_HOP", sync.MAX_HOP), ("BP_SYNC_MAX_GAIN", sync.MAX_GAIN),
                         ("BP_SYNC_MAX_CELLS", sync.MAX_CELLS), ("BP_SYNC_MAX_PRED_BYTES", sync.MAX_PRED_BYTES), ("BP_SYNC_CLASSES", sync.CLASSES),
                         ("BP_SYNC_PITCHES", sync.PITCHES), ("BP_SYNC_TRACE_TILE", sync.TRACE_TILE)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert sync.SYNC_SUMMARY == SC.SUMMARY and sync.MAX_UNITS == 8192 == 1024 * 8 and sync.MAX_GAIN == 255 ** 2 and sync.MAX_CELLS == 2 ** 28
    # the bounds the header states
    assert 64 * 2 ** 13 == 2 ** 19 and 12 * 2 ** 38 < 2 ** 42 and 16384 * 65025 == 1065369600 < 2 ** 31 and 8191 * 8192 < 2 ** 26
    assert (8192 + 1024 - 1) * 1024 * 2 < sync.MAX_PRED_BYTES  # the largest pair's predecessors fit the store
    # the existing lists are what they were and share nothing with the new one; the build watches the new files
    old = set(_native.CHORD_SYMBOLS) | set(_native.BEAT_SYMBOLS) | set(_native.ALIGN_SYMBOLS) | set(_native.MELODY_SYMBOLS) | \
        set(_native.MULTIPITCH_SYMBOLS) | set(_native.FRAME_SCORE_SYMBOLS) | set(_native.SCORE_SYMBOLS) | set(_native.SWEEP_SYMBOLS) | \
        set(_native.EVENTS_SYMBOLS) | set(_native.EXPORTED_SYMBOLS) | set(_native.FLAC_CLIPS_SYMBOLS) | set(_native.CONTAINERS_SYMBOLS) | \
        set(_native.ADPCM_SYMBOLS) | set(_native.LIVE_SYMBOLS) | set(_native.ROLLING_SYMBOLS) | set(_native.UPDATE_SYMBOLS) | \
        set(_native.STREAM_EVENTS_SYMBOLS) | set(_native.CLIPS_SYMBOLS)
    assert not set(NEW) & old and len(_native.CHORD_SYMBOLS) == 6 and len(_native.BEAT_SYMBOLS) == 6 and len(_native.ALIGN_SYMBOLS) == 4
    assert os.path.basename(build.SYNC_HEADER) == "basic_pitch_amd_sync.h" and build.SYNC_HEADER in build.HEADERS
    assert {"sync.hip", "sync_host.cpp", "clips_sync.hip"} <= set(build.SOURCES)
    for entry in ("sync", "sync_pairs", "transcribe_clips_sync"):
        assert hasattr(Model, entry), entry
    for method in ("map_times", "transfer_notes"):
        assert hasattr(sync.Sync, method), method
    unpinned = open(os.path.join(ROOT, "README.md")).read().split("Unpinned")[1].lower()
    assert "basic_pitch_amd_sync.h" in unpinned and "third-party alignment or time-warping implementation" in unpinned
    assert "basic_pitch_amd_sync.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "transfer_notes" in sync.__doc__


def test_the_symbols_are_exported_by_both_libraries(lib):
    from basic_pitch_amd import build

    for path in (build.build_library(), build.build_library(ab=True)):
        defined = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(rf"\bT {name}\b", defined), (path, name)


def test_the_structures_are_the_bytes_the_header_declares(lib):
    from basic_pitch_amd import _native, sync

    text, header = _header()
    for name, size in (("bp_sync_params", 32), ("bp_sync_pair", 8), ("bp_sync_summary", 32)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, flags=re.S).group(1)
        fields = []
        for t, decl in re.findall(r"\b(int32_t|int64_t)\s+([a-zA-Z_0-9, \[\]]+);", body):
            for n in decl.split(","):
                field, dims = re.fullmatch(r"\s*([a-z_]+)((?:\[[0-9]+\])*)\s*", n).groups()
                ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}[t]
                for d in reversed(re.findall(r"\[([0-9]+)\]", dims)):
                    ctype = ctype * int(d)
                fields.append((field, ctype))
        struct = getattr(_native, name)
        assert fields == list(struct._fields_) and C.sizeof(struct) == size, (name, fields)
        assert f"/* {size} bytes */" in text
    assert sync.SYNC_SUMMARY.itemsize == 32 and [sync.SYNC_SUMMARY.fields[n][1] for n in sync.SYNC_SUMMARY.names] == [0, 4, 8, 12, 16, 24]
    assert sync.SYNC_PAIR.itemsize == 8 and sync.pair_table([(3, 5), (0, 0)]).tobytes() == np.array([3, 5, 0, 0], np.int32).tobytes()
    p = sync.sync_params()
    assert (p.threshold_q, p.min_pitch, p.max_pitch, p.hop, p.band, list(p.reserved)) == (307, 0, 87, 4, 0, [0, 0, 0])
    assert sync.sync_params(hop=9).hop == 9 and sync.sync_params(dict(band=5)).band == 5 and sync.sync_params(p) is p
    with pytest.raises(TypeError):
        sync.sync_params(threshold=1)


# ---- the checker against the restatement
@pytest.mark.parametrize("kind", list(SC.KINDS))
def test_the_checker_equals_the_numpy_restatement_on_seeded_pairs(lib, kind):
    from basic_pitch_amd import sync

    rng = np.random.default_rng(sorted(SC.KINDS).index(kind))
    bands_seen, cut, ragged = set(), 0, 0
    for case in range(64):
        hop = (1, 3, 4, 64)[case % 4]
        band = (0, 1, 3, 20)[(case // 4) % 4]
        N, M = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        if hop == 64:
            N, M = min(N, 12), min(M, 12)
        rows_a, rows_b = N * hop - int(rng.integers(0, hop)), M * hop - int(rng.integers(0, hop))  # rows not a multiple of hop
        ragged += rows_a % hop != 0
        fields = dict(hop=hop, band=band, threshold_q=int(rng.choice([0, 128, 307, 700])))
        if case % 3 == 2:
            lo = int(rng.integers(0, 60))
            fields.update(min_pitch=lo, max_pitch=lo + int(rng.integers(0, 88 - lo)))  # pitch bands
        a, b = SC.random_maps(1000 * case + 7, rows_a, rows_b, kind)
        want = SC.restate(a, b, **fields)
        _same(sync.sync_rows(a, b, fields), want, (kind, case, fields, N, M))
        assert want[0]["status"][0] == 0 and want[0]["units_a"][0] == N and want[0]["units_b"][0] == M
        if band:
            path = want[1][: want[0]["n_path"][0]]
            ok = SC.admissible(N, M, band)
            assert ok[path[:, 0], path[:, 1]].all()
            cut += int(not ok.all())
            bands_seen.add(band)
    assert bands_seen == {1, 3, 20} and cut >= 10 and ragged >= 20, (bands_seen, cut, ragged)


def test_the_quantiser_the_classes_and_the_ceiling_root(lib):
    """The feature's extremes: a one-hot unit is 255 in its class and reaches g = 65,025 in every cell; (1, 1) energies give
    (127, 127); a map of ones gives twelve nearly equal classes whose floors stay under 255^2; the floor root would not."""
    from basic_pitch_amd import sync

    for pitch in (0, 3, 39, 50, 87):
        note = np.zeros((8, 88), np.float32)
        note[:, pitch] = 1.0
        x = SC.features(note, hop=4)
        assert x.shape == (2, 12) and x[0].tolist() == [255 * int(k == (pitch + 21) % 12) for k in range(12)]
        s, path = sync.sync_rows(note, note)
        assert (s["status"][0], s["total"][0], s["n_path"][0]) == (0, 4 * 65025, 2) and path.tolist() == [[0, 0], [1, 1], [-1, -1]]
    two = np.zeros((1, 88), np.float32)
    two[0, 39] = two[0, 40] = (307 + 1) / 1024.0  # one above the threshold each: energies (1, 1)
    assert SC.features(two, hop=1)[0].tolist() == [127, 127] + [0] * 10 and 255 // 1 == 255  # (floor root of 2 is 1: (255, 255))
    s, _ = sync.sync_rows(two, two, hop=1)
    assert s["total"][0] == 2 * (127 * 127 * 2)
    ones = np.ones((6, 88), np.float32)
    g = SC.gains(SC.features(ones, hop=3), SC.features(ones, hop=3))
    assert g.min() == g.max() == 64800 <= SC.MAX_GAIN  # eight pitches in four classes, seven in eight: floors of 255 c / r
    s, path = sync.sync_rows(ones, ones, hop=3)
    assert s["total"][0] == 4 * 64800 and path[:2].tolist() == [[0, 0], [1, 1]]
    rng = np.random.default_rng(1)
    worst = 0
    for _ in range(300):
        cu = rng.integers(0, 2 ** 19 + 1, 12) * (rng.integers(0, 3, 12) > 0)
        s = int((cu.astype(object) ** 2).sum())
        if s:
            r = SC.ceil_root(s)
            assert r * r >= s > (r - 1) * (r - 1)
            worst = max(worst, int(((255 * cu // r) ** 2).sum()))
    assert 60000 < worst <= 255 ** 2


# ---- all monotone paths
def test_the_best_of_all_monotone_paths_and_the_one_the_tie_order_selects(lib):
    from basic_pitch_amd import sync

    several = cases = 0
    for N in range(1, 6):
        for M in range(1, 6):
            paths = SC.all_paths(N, M)
            for seed in range(3):
                a, b = SC.random_maps(97 * N + 13 * M + seed, N, M, "eighths")
                fields = dict(hop=1, threshold_q=0)
                g = SC.gains(SC.features(a, **fields), SC.features(b, **fields))
                totals = [SC.path_total(g, p) for p in paths]
                best = [p for p, t in zip(paths, totals) if t == max(totals)]
                s, region = sync.sync_rows(a, b, fields)
                assert s["status"][0] == 0 and s["total"][0] == max(totals), (N, M, seed)
                assert region[: s["n_path"][0]].tolist() == [list(c) for c in SC.selected_by_ties(best)], (N, M, seed, len(best))
                several += len(best) > 1
                cases += 1
    assert cases == 75 and several >= 10, several  # (at least one case must have more than one optimal path)
    assert len(SC.all_paths(5, 5)) == 321  # the central Delannoy number D(4, 4)


# ---- planted warps and a segment against itself
@pytest.mark.parametrize("seed", range(12))
def test_planted_warps_come_back_exactly_in_both_roles(lib, seed):
    from basic_pitch_amd import sync

    N, M = (40, 65) if seed == 0 else (5 + 3 * seed, 5 + 3 * seed + 7 * (seed % 4))
    for hop in (4, 1):
        a, b, w = SC.planted_warp(seed, N, M, hop)
        want = np.stack([w, np.arange(M)], axis=1).astype(np.int32)
        s, region = sync.sync_rows(a, b, hop=hop)
        assert s["status"][0] == 0 and s["n_path"][0] == M and np.array_equal(region[:M], want), (seed, hop)
        assert s["total"][0] == (N + M) * 65025 and np.all(region[M:] == -1)
        _same((s, region), SC.restate(a, b, hop=hop), (seed, hop))
        s, region = sync.sync_rows(b, a, hop=hop)  # the roles swapped
        assert s["n_path"][0] == M and np.array_equal(region[:M], want[:, ::-1]) and s["total"][0] == (N + M) * 65025


@pytest.mark.parametrize("seed", range(5))
def test_a_chord_map_against_itself_gives_the_diagonal(lib, seed):
    """The header's condition: every unit of these maps has the same self-gain, and the restatement itself returns the
    diagonal."""
    from basic_pitch_amd import sync

    note = SC.chord_map(seed, 60)
    x = SC.features(note)
    assert len({int(v @ v) for v in x}) == 1  # the same self-gain everywhere
    want = SC.restate(note, note)
    diagonal = np.stack([np.arange(60)] * 2, axis=1)
    assert np.array_equal(want[1][:60], diagonal) and want[0]["n_path"][0] == 60
    _same(sync.sync_rows(note, note), want, seed)


# ---- silence
def test_silent_units_earn_nothing_and_the_ties_decide(lib):
    from basic_pitch_amd import sync

    rng = np.random.default_rng(4)
    for where in ("middle", "start", "end", "both ends"):
        a, b = SC.thousand(rng, 48), SC.eighths(rng, 60)
        for note in (a, b):
            if where == "middle":
                note[16:28] = 0.0
            if where in ("start", "both ends"):
                note[:9] = 0.0
            if where in ("end", "both ends"):
                note[-9:] = 0.0
        want = SC.restate(a, b)
        assert want[0]["status"][0] == 0
        _same(sync.sync_rows(a, b), want, where)
    quiet_a, quiet_b = np.zeros((20, 88), np.float32), np.full((33, 88), 0.29, np.float32)  # silence, and everything under the threshold
    s, region = sync.sync_rows(quiet_a, quiet_b)
    _same((s, region), SC.restate(quiet_a, quiet_b), "all silent")
    # status 0, total 0, and the path by ties alone: the diagonal first, then (i, j-1) along the last row
    assert (s["status"][0], s["total"][0], s["n_path"][0]) == (0, 0, 9)
    assert region[:9].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4], [1, 5], [2, 6], [3, 7], [4, 8]]


# ---- statuses and independence
def test_the_statuses_and_that_a_pair_does_not_depend_on_the_others(lib):
    from basic_pitch_amd import sync

    rng = np.random.default_rng(6)
    a, b = SC.thousand(rng, 40), SC.eighths(rng, 52)
    clean = sync.sync_rows(a, b)
    assert clean[0]["status"][0] == 0
    for row, pitch in ((0, 87), (39, 0), (17, 50)):
        bad = a.copy()
        bad[row, pitch] = np.nan
        for fields in (dict(), dict(min_pitch=10, max_pitch=20)):  # in the band or outside it: whatever pitch
            for pair in ((bad, b), (b, bad), (bad, bad)):
                s, region = sync.sync_rows(*pair, fields)
                _same((s, region), SC.restate(*pair, **fields), (row, pitch))
                assert (s["status"][0], s["n_path"][0], s["total"][0]) == (1, 0, 0) and np.all(region == -1) and len(region) > 0
    a[5, 5] = np.inf  # an infinity is a value
    assert sync.sync_rows(a, b)[0]["status"][0] == 0
    none = a[:0]
    for pair in ((none, b), (a, none), (none, none)):
        s, region = sync.sync_rows(*pair)
        _same((s, region), SC.restate(*pair), "no rows")
        assert s["status"][0] == 2 and len(region) == 0 and s["units_a"][0] == (len(pair[0]) + 3) // 4
    bad = b.copy()
    bad[0, 0] = np.nan
    assert sync.sync_rows(bad, none)[0]["status"][0] == 1  # a NaN is decided first
    # no band cuts the end off: the header's staircase, tried on every shape up to 14 x 14
    flat = np.ones((14, 88), np.float32)
    for N in range(1, 15):
        for M in range(1, 15):
            for band in (1, 2, 5):
                ok = SC.admissible(N, M, band)
                assert SC.warp(np.ones((N, M), np.int64), ok)[2] is not None, (N, M, band)
        assert sync.sync_rows(flat[:N], flat, hop=1, band=1)[0]["status"][0] == 0
    # the same pair gives the same bytes whatever pair was computed before it (the checker keeps nothing between calls)
    again = sync.sync_rows(a, b)
    sync.sync_rows(b, b, hop=1, band=3)
    assert sync.sync_rows(a, b)[0].tobytes() == again[0].tobytes() and sync.sync_rows(a, b)[1].tobytes() == again[1].tobytes()
    s = sync.Sync.of(again[0][0], again[1], 4)
    assert (s.status, s.total, s.units_a, s.units_b, s.hop) == (0, int(again[0]["total"][0]), 10, 13, 4) and s.path.shape == (int(again[0]["n_path"][0]), 2)
    assert np.all(np.diff(s.map_times(np.linspace(0, 1, 50))) >= 0) and np.all(np.diff(s.map_times(np.linspace(0, 1, 50), to="a")) >= 0)


# ---- refusals
def test_every_malformed_argument_is_refused(lib):
    from basic_pitch_amd import _native, sync

    rng = np.random.default_rng(33)
    a, b = SC.thousand(rng, 100), SC.eighths(rng, 60)
    room = 25 + 15 - 1
    path = np.full((256, 2), 77, np.int32)  # room for the 100 + 60 - 1 entries of hop 1 below, and more
    summary = np.zeros(1, SC.SUMMARY)
    summary["status"] = 77

    def call(p, rows_a=100, rows_b=60, a_p=a.ctypes.data, b_p=b.ctypes.data, path_p=path.ctypes.data, room=room, summary_p=summary.ctypes.data):
        return lib.bp_sync_rows(a_p, rows_a, b_p, rows_b, C.addressof(p) if p is not None else None, path_p, room, summary_p)

    ok = sync.sync_params()
    bad_sets = [("threshold_q", -1), ("threshold_q", 1025), ("min_pitch", -1), ("max_pitch", 88), ("hop", 0), ("hop", 65), ("hop", -4),
                ("band", -1), ("band", 8193), ("reserved", 1), ("reserved", (0, 1, 0)), ("reserved", (0, 0, 1))]
    for field, value in bad_sets:
        assert call(sync.sync_params(**{field: value})) == _native.BP_ERR_INVALID_ARG, (field, value)
        with pytest.raises(ValueError):
            sync.sync_rows(a, b, **{field: value})
    assert call(sync.sync_params(min_pitch=50, max_pitch=49)) == _native.BP_ERR_INVALID_ARG
    assert call(None) == call(ok, rows_a=-1) == call(ok, rows_b=-1) == call(ok, a_p=None) == call(ok, b_p=None) == _native.BP_ERR_INVALID_ARG
    assert call(ok, summary_p=None) == call(ok, path_p=None) == call(ok, room=room - 1) == call(ok, room=-1) == _native.BP_ERR_INVALID_ARG
    # a segment above BP_SYNC_MAX_UNITS, refused from the row count alone (nothing is read)
    assert call(ok, rows_a=4 * sync.MAX_UNITS + 1, room=10 ** 6) == call(ok, rows_b=4 * sync.MAX_UNITS + 1, room=10 ** 6) == _native.BP_ERR_INVALID_ARG
    assert np.all(path == 77) and summary["status"][0] == 77, "a refused call wrote to its outputs"
    for field, value in (("threshold_q", 0), ("threshold_q", 1024), ("hop", 1), ("hop", 64), ("band", 8192), ("min_pitch", 87), ("max_pitch", 0)):
        assert call(sync.sync_params(**{field: value}), room=len(path)) == _native.BP_OK, (field, value)
    path[:] = 77
    assert call(ok) == _native.BP_OK and summary["status"][0] == 0 and summary["units_a"][0] == 25 and np.all(path[room:] == 77)
    assert lib.bp_sync_rows(None, 0, None, 0, C.addressof(ok), None, 0, summary.ctypes.data) == _native.BP_OK and summary["status"][0] == 2
    # the reason a device call gives names the field
    lib.bp_internal_sync_bad_params.restype = C.c_char_p
    lib.bp_internal_sync_bad_params.argtypes = [C.c_void_p]
    for field, value in bad_sets:
        bad = sync.sync_params(**{field: value})
        why = lib.bp_internal_sync_bad_params(C.addressof(bad)).decode()
        assert field.split("_")[0] in why, (field, why)
    assert lib.bp_internal_sync_bad_params(C.addressof(ok)) is None
    with pytest.raises(ValueError):
        sync.sync_rows(np.zeros((4, 87), np.float32), b)


# ---- the source alone, under the host sanitizers
def test_the_checker_links_without_a_device_and_runs_clean_under_the_sanitizers(tmp_path):
    """tests/test_chord_cpu.py's pattern: the checker's source and tools/sanitize/sync_host.cpp, plain g++, once with
    -fsanitize=address,undefined; both print the same line."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "sync_host.cpp"), os.path.join(ROOT, "basic_pitch_amd", "csrc", "sync_host.cpp")]
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / f"sync_host_{name}")
        res = subprocess.run([cxx, "-std=c++17", "-O1", "-w"] + extra + srcs + ["-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        if extra:
            syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
            assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
        res = subprocess.run([exe, "200"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        outs.append(res.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("sync 200 cases: ")
    words = outs[0].split()
    sums = {k: v for k, v in zip(words[3::2], words[4::2])}
    assert int(sums["paths"]) > 80 and int(sums["flagged"]) > 0 and int(sums["empty"]) > 20 and int(sums["refused"]) >= 600
    assert int(sums["cells"]) > 10000 and int(sums["steps"]) > 1000
