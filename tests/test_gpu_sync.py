"""Two recordings against each other on the device (include/basic_pitch_amd_sync.h; csrc/sync.hip): the summaries and the
whole path regions, tails included, of bp_sync_from_maps are byte for byte those of the host checker bp_sync_rows, pair by
pair — every shape where the kernels can go wrong as a call of its own, so that it picks its own launch variant (units of 1 and
2, a wave's edge, the capacities of the small and the large workgroup and every step from one number of columns a lane to the
next, a shorter than the lanes in use, the backtrace tile -+ 1, the two sizes of the LDS staging of a, the largest segments),
the band on and off, hop 1 and 64; a mixed job with a segment without rows, one with a NaN, (a, a), shared segments and a
segment no pair names, in host and in device memory; the pools and the other calls of the handle; every refusal; planted warps;
clips through the model and the Python entries; the Sync methods; the non-default handles."""
import ctypes as C
import functools

import numpy as np
import pytest

import sync_cases as SC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

INV = -1
MAX_UNITS, TRACE_TILE = 8192, 64  # BP_SYNC_* (compared with the binding's and the header's below)
SMALL_LANES, LANES, SMALL_ROWS = 256, 1024, 2048  # csrc/bp_kernels.h: kSyncSmallLanes, kSyncLanes, kSyncSmallRows


@pytest.fixture(scope="module")
def model():
    import os
    import re

    from basic_pitch_amd import sync as SY
    from basic_pitch_amd.inference import Model
    from conftest import ROOT

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_sync.h")).read()
    for macro, ours, theirs in (("BP_SYNC_MAX_UNITS", MAX_UNITS, SY.MAX_UNITS), ("BP_SYNC_TRACE_TILE", TRACE_TILE, SY.TRACE_TILE)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == ours == theirs, macro
    kernels = open(os.path.join(ROOT, "basic_pitch_amd", "csrc", "bp_kernels.h")).read()
    for constant, ours in (("kSyncSmallLanes", SMALL_LANES), ("kSyncLanes", LANES), ("kSyncSmallRows", SMALL_ROWS)):
        assert int(re.search(rf"\b{constant}\s*=\s*(\d+)", kernels).group(1)) == ours, constant
    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host(maps, pairs, prm=None):
    """The host checker on every pair: (summaries with path_first as the device counts it, the path of all pairs)."""
    from basic_pitch_amd import sync as SY

    summaries, regions, first = [], [], 0
    for a, b in pairs:
        s, region = SY.sync_rows(maps[a], maps[b], prm)
        s["path_first"] = first
        first += len(region)
        summaries.append(s)
        regions.append(region)
    return np.concatenate(summaries + [np.zeros(0, SC.SUMMARY)]), np.concatenate(regions + [np.zeros((0, 2), np.int32)]).astype(np.int32)


def _device(model, maps, pairs, prm=None, where="host"):
    import torch

    from basic_pitch_amd import _native, sync as SY

    offs, note = SC.stack(maps)
    if where == "host":
        before = note.copy()
        got = SY.sync_from_maps(model, offs, note.ctypes.data if note.size else None, _native.BP_MEM_HOST, pairs, prm)
        after = note
    else:
        before = note
        shift = 1 if where == "device_unaligned" else 0  # one float: 4 bytes off a 16-byte boundary
        dev = torch.empty(note.size + 4, dtype=torch.float32, device="cuda")
        view = dev[shift : shift + note.size]
        view.copy_(torch.from_numpy(note.reshape(-1)))
        torch.cuda.synchronize()
        assert (view.data_ptr() % 16 != 0) == bool(shift)
        got = SY.sync_from_maps(model, offs, view.data_ptr(), _native.BP_MEM_DEVICE, pairs, prm)
        after = view.cpu().numpy().reshape(note.shape)
    assert after.tobytes() == before.tobytes(), "the map is left untouched"
    return got


def _assert_equal(got, want, where):
    for g, w, name in zip(got, want, ("summaries", "path")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (where, name, g[:6], w[:6])


@functools.lru_cache(maxsize=None)
def _segment(seed, units, kind="eighths"):
    """A seeded map of `units` rows (a unit a row under hop 1), shared and left alone."""
    note = SC.KINDS[kind](np.random.default_rng(seed), units)
    note.setflags(write=False)
    return note


# ---- the shapes where the kernels can go wrong, each a call of its own
C_OF = lambda m: 1 if m <= 256 else 2 if m <= 512 else 4 if m <= 1024 else 8 if m <= 2048 else 4 if m <= 4096 else 8  # noqa: E731
SHAPES = {
    "units of 1 and 2": [(1, 1), (1, 2), (2, 1), (2, 2), (1, 70), (70, 1), (2, 300), (300, 2)],
    "a wave's edge": [(40, 63), (40, 65), (40, 2 * 192 - 1), (40, 2 * 192 + 1), (40, 4 * 192 - 1), (40, 4 * 192 + 1), (40, 8 * 192 - 1),
                      (40, 8 * 192 + 1), (40, 4 * 640 - 1), (40, 4 * 640 + 1), (40, 8 * 576 - 1), (40, 8 * 576 + 1)],
    "capacities and the steps between columns": [(37, m) for m in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095,
                                                                   4096, 4097, 8191)],
    "a shorter than the lanes in use": [(3, 200), (3, 1000), (5, 2048), (3, 4000), (2, 8192), (100, 1500)],
    "the backtrace tile": [(TRACE_TILE - 1, 1), (TRACE_TILE, 1), (TRACE_TILE + 1, 1), (2 * TRACE_TILE + 1, 1), (TRACE_TILE, 100),
                           (2 * TRACE_TILE + 1, 130), (200, 200), (300, 700)],
    "the staging of a": [(SMALL_ROWS - 1, 70), (SMALL_ROWS, 70), (SMALL_ROWS + 1, 70), (SMALL_ROWS + 1, 300)],
    "the largest segments": [(MAX_UNITS, 70), (70, MAX_UNITS)],
}


def test_the_shapes_cover_every_launch_variant():
    ms = [m for group in SHAPES.values() for _, m in group]
    assert {(SMALL_LANES if m <= 8 * SMALL_LANES else LANES, C_OF(m)) for m in ms} == {(256, 1), (256, 2), (256, 4), (256, 8), (1024, 4), (1024, 8)}
    for cap in (256, 512, 1024, 2048, 4096):
        assert {cap - 1, cap, cap + 1} <= set(ms)
    assert any(n < (m + C_OF(m) - 1) // C_OF(m) for group in SHAPES.values() for n, m in group)


@pytest.mark.parametrize("group", list(SHAPES))
def test_the_shapes_where_the_kernels_can_go_wrong(model, group):
    for k, (n, m) in enumerate(SHAPES[group]):
        kind = "eighths" if k % 2 == 0 else "thousand"
        maps = [_segment(100 + k, n, kind), _segment(200 + k, m, kind)]
        got = _device(model, maps, [(0, 1)], dict(hop=1), "device" if k % 3 == 0 else "host")
        _assert_equal(got, _host(maps, [(0, 1)], dict(hop=1)), (group, n, m))
        assert got[0]["status"][0] == 0 and max(n, m) <= got[0]["n_path"][0] <= n + m - 1


def test_the_largest_pairs_on_constant_maps_reach_the_largest_total(model):
    """BP_SYNC_MAX_UNITS x BP_SYNC_MAX_UNITS twice in one call, against the checker only: a map of ones (every gain the same,
    64,800: twelve floored classes do not reach 255^2) and a one-hot map (every gain 65,025: the largest total there is)."""
    ones = np.ones((MAX_UNITS, 88), np.float32)
    one_hot = SC.one_hot_units([0] * MAX_UNITS, 1)
    got = _device(model, [ones, one_hot], [(0, 0), (1, 1)], dict(hop=1), "device")
    _assert_equal(got, _host([ones, one_hot], [(0, 0), (1, 1)], dict(hop=1)), "constant maps")
    assert got[0]["total"].tolist() == [2 * MAX_UNITS * 64800, 2 * MAX_UNITS * 65025] and 2 * MAX_UNITS * 65025 == 1065369600 < 2 ** 31
    diagonal = np.stack([np.arange(MAX_UNITS)] * 2, axis=1)
    for p in range(2):
        region = got[1][p * (2 * MAX_UNITS - 1) : (p + 1) * (2 * MAX_UNITS - 1)]
        assert got[0]["n_path"][p] == MAX_UNITS and np.array_equal(region[:MAX_UNITS], diagonal) and np.all(region[MAX_UNITS:] == -1)


@pytest.mark.parametrize("band", [0, 1, 3, 20])
def test_the_band_on_and_off_and_hop_1_and_64(model, band):
    for n, m in ((40, 65), (300, 700), (90, 2049)):
        for hop in (1, 64) if m < 2049 else (1,):  # (the longest at hop 1 alone: 2049 units of 64 rows are 46 MB)
            rows = lambda u, cut: u * hop - (cut % hop)  # noqa: E731  (rows that are no multiple of hop)
            maps = [SC.eighths(np.random.default_rng(n + hop), rows(n, 3)), SC.thousand(np.random.default_rng(m + hop), rows(m, 5))]
            prm = dict(hop=hop, band=band, threshold_q=200)
            got = _device(model, maps, [(0, 1), (1, 0)], prm)
            _assert_equal(got, _host(maps, [(0, 1), (1, 0)], prm), (band, n, m, hop))
            assert got[0]["units_a"].tolist() == [n, m] and got[0]["status"].tolist() == [0, 0]
            if band:
                i, j = got[1][: got[0]["n_path"][0]].astype(np.int64).T
                assert np.all(np.abs(i * (m - 1) - j * (n - 1)) <= band * max(n - 1, m - 1))


# ---- a mixed job in one call
@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(11)
    rows = [90, 0, 300, 41, 130, 7, 610, 55, 200, 33]
    maps = [SC.KINDS[("eighths", "thousand", "sparse")[i % 3]](rng, r) for i, r in enumerate(rows)]
    maps[4][-1, 87] = np.nan  # a NaN in its last row
    pairs = [(0, 2), (2, 2), (0, 3), (3, 0), (1, 5), (4, 0), (6, 8), (8, 6), (5, 1), (1, 1), (4, 1), (9, 6)]  # segment 7: no pair names it
    return maps, pairs


@pytest.mark.parametrize("where", ["host", "device", "device_unaligned"])
def test_a_mixed_job_in_one_call(model, where):
    maps, pairs = _mixed()
    for prm in (None, dict(hop=3, band=2, min_pitch=20, max_pitch=70)):
        want = _host(maps, pairs, prm)
        got = _device(model, maps, pairs, prm, where)
        _assert_equal(got, want, (where, prm))
        assert got[0]["status"].tolist() == [0, 0, 0, 0, 2, 1, 0, 0, 2, 2, 1, 0]
        for p in (1, 6, 11):  # three pairs alone give the bytes they give inside the job
            alone = _device(model, maps, [pairs[p]], prm, where)
            first, n = int(got[0]["path_first"][p]), len(alone[1])
            assert alone[1].tobytes() == got[1][first : first + n].tobytes()
            assert alone[0][["status", "units_a", "units_b", "n_path", "total"]].tolist() == got[0][p : p + 1][["status", "units_a", "units_b", "n_path", "total"]].tolist()


# ---- pools and neighbours
def test_a_smaller_call_after_a_larger_one_and_the_other_calls_undisturbed(model):
    """Events, a sweep, the melody and an alignment of one segment give the bytes they gave before the sync calls between
    them (a larger one, then smaller ones, which also shows the grow-only pools reused)."""
    import align_cases as AC
    from basic_pitch_amd import _native, align as AL, melody as ME

    rng = np.random.default_rng(3)
    out = TS._segment(rng, 142)
    note_prm = TS._prm(TS.BASE)
    sets = [TS._prm(dict(TS.BASE, **v)) for v in TS.VARIED[:3]]
    note, onset, contour = (np.ascontiguousarray(out[k], np.float32) for k in ("note", "onset", "contour"))
    states = AC.random_states(rng, 11, 142)

    def others():
        ev = TS._single(model, out, note_prm)
        sw = TS._sweep(model, [out], sets)
        mel = ME.melody_from_maps(model, [0, 142], contour.ctypes.data, _native.BP_MEM_HOST)
        al = AL.align_from_maps(model, [0, 142], note.ctypes.data, onset.ctypes.data, _native.BP_MEM_HOST, [0, len(states)], states)
        return (ev, sw, mel[0].tobytes(), mel[1].tolist(), al[0].tobytes(), al[1].tolist(), al[2].tolist())

    before = others()
    assert len(before[0][0]) > 0 and len(before[1]) == 3
    ff, total, status = AL.align_rows(note, onset, states)  # the alignment has a path, and it is the checker's
    assert (before[4], before[5], before[6]) == (ff.tobytes(), [total], [status]) and status == 0 and total != 0
    large = [SC.thousand(rng, 3000), SC.eighths(rng, 2200)]
    small = [SC.eighths(rng, 60), SC.sparse(rng, 30)]
    _assert_equal(_device(model, large, [(0, 1)]), _host(large, [(0, 1)]), "large")
    for where in ("host", "device"):
        _assert_equal(_device(model, small, [(0, 1), (1, 1)], None, where), _host(small, [(0, 1), (1, 1)]), ("small after large", where))
    own = [np.asarray(out["note"], np.float32)]
    _assert_equal(_device(model, own, [(0, 0)]), _host(own, [(0, 0)]), "the segment of the other calls")
    assert others() == before


# ---- refusals
def test_nothing_to_do_the_refusals_and_too_little_room(model):
    from basic_pitch_amd import _native, sync as SY

    lib = SY.bind(model._lib)
    h = model._handle
    rng = np.random.default_rng(70)
    maps = [SC.eighths(rng, 200), SC.thousand(rng, 90)]
    offs, note = SC.stack(maps)
    pair_list = [(0, 1), (1, 1)]
    want = _host(maps, pair_list)
    room_needed = len(want[1])
    assert room_needed == (50 + 23 - 1) + (23 + 23 - 1)
    p = SY.sync_params()
    tab = SY.pair_table(pair_list)
    summaries = np.zeros(4, SC.SUMMARY)
    path = np.full((room_needed + 8, 2), 77, np.int32)
    zero = np.zeros(4, np.int64)

    def fresh():
        summaries.view(np.uint8)[:] = 77
        path[:] = 77

    def call(n=2, offs=offs, note_p=note.ctypes.data, kind=_native.BP_MEM_HOST, n_pairs=2, tab=tab, p=p, summaries_p=summaries.ctypes.data,
             path_p=path.ctypes.data, room=room_needed):
        return lib.bp_sync_from_maps(h, n, _p64(offs), note_p, kind, n_pairs, tab.ctypes.data if tab is not None else None,
                                     C.addressof(p) if p is not None else None, summaries_p, path_p, room)

    def refused(rc, *words):
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and "bp_sync_from_maps" in msg and all(w in msg for w in words), (rc, msg)
        assert np.all(summaries.view(np.uint8) == 77) and np.all(path == 77), "a refused call wrote to its outputs"

    fresh()
    # zero pairs: a call that does nothing; pairs of segments without rows: no device work, status 2
    assert call(n_pairs=0, tab=None, summaries_p=None, path_p=None, room=0) == 0
    assert call(n=0, offs=zero, note_p=None, n_pairs=0, tab=None, summaries_p=None, path_p=None, room=0) == 0
    assert np.all(summaries.view(np.uint8) == 77) and np.all(path == 77)
    assert call(n=3, offs=zero, note_p=None, path_p=None, room=0) == 0
    assert summaries[:2].tolist() == [(2, 0, 0, 0, 0, 0)] * 2 and np.all(path == 77)
    fresh()
    # the refusals, each before anything is queued or written
    refused(call(n=-1), "negative")
    refused(call(n_pairs=-1), "negative")
    refused(call(offs=np.array([1, 200, 290], np.int64)), "row_offsets")
    refused(call(offs=np.array([0, 200, 199], np.int64)), "row_offsets")
    refused(call(kind=7), "mem_kind")
    refused(call(note_p=None), "null input")
    refused(call(summaries_p=None), "summaries")
    refused(call(tab=None), "pairs")
    refused(call(p=None), "params")
    refused(call(room=room_needed - 1), f"room for {room_needed - 1}", str(room_needed), "nothing has been written")
    refused(call(room=-1), "max_path")
    refused(call(path_p=None), "without a buffer")
    for bad, at in (([(0, 2), (1, 1)], 0), ([(0, 1), (-1, 1)], 1), ([(0, 1), (1, 2)], 1)):
        refused(call(tab=SY.pair_table(bad)), f"pair {at}", "outside 0 ... 1")
    for field, value, word in (("threshold_q", 1025, "threshold_q"), ("hop", 0, "hop"), ("hop", 65, "hop"), ("band", -1, "band"),
                               ("band", MAX_UNITS + 1, "band"), ("max_pitch", 88, "max_pitch"), ("min_pitch", -1, "min_pitch"),
                               ("reserved", 1, "reserved"), ("reserved", (0, 0, 1), "reserved")):
        refused(call(p=SY.sync_params(**{field: value})), "params", word)
    # the bounds, refused from the offsets alone (nothing is read): the pair and the segment are named
    long_offs = np.array([0, 10, 10 + 4 * MAX_UNITS + 1], np.int64)
    refused(call(offs=long_offs, room=10 ** 6), "pair 0", "segment 1", "BP_SYNC_MAX_UNITS")
    many = SY.pair_table([(1, 1)] * 5)  # five pairs of 8192 x 8192 units: 2^28 cells are passed at the fifth
    full = np.array([0, 10, 10 + 4 * MAX_UNITS], np.int64)
    big = np.zeros(8, SC.SUMMARY)
    big.view(np.uint8)[:] = 77
    rc = call(offs=full, n_pairs=5, tab=many, summaries_p=big.ctypes.data, room=10 ** 6)
    refused(rc, "pair 4", "BP_SYNC_MAX_CELLS")
    assert np.all(big.view(np.uint8) == 77)
    # pairs of a one-unit a against the longest b: few cells, but their skewed predecessors pass the store's bound
    skew = np.array([0, 1, 1 + 4 * MAX_UNITS], np.int64)
    n_skew = 200
    big = np.zeros(n_skew, SC.SUMMARY)
    big.view(np.uint8)[:] = 77
    rc = call(offs=skew, n_pairs=n_skew, tab=SY.pair_table([(0, 1)] * n_skew), summaries_p=big.ctypes.data, room=10 ** 7)
    refused(rc, "pair 128", "BP_SYNC_MAX_PRED_BYTES")
    assert np.all(big.view(np.uint8) == 77)
    rows_in_all = np.array([0, 4 * MAX_UNITS, 2 ** 23 + 1], np.int64)
    refused(call(offs=rows_in_all, tab=SY.pair_table([(0, 0), (0, 0)]), room=10 ** 6), "BP_SWEEP_MAX_ROWS")
    # and the handle is usable: the same arguments, unbroken, with exactly the room the pairs ask for
    assert call() == 0
    assert summaries[:2].tobytes() == want[0].tobytes() and path[:room_needed].tobytes() == want[1].tobytes() and np.all(path[room_needed:] == 77)
    assert np.all(summaries[2:].view(np.uint8) == 77)


# ---- planted warps
def test_planted_warps_are_recovered_exactly_on_the_device(model):
    maps, pairs, ws = [], [], []
    for seed in range(24):
        n = 20 + seed
        a, b, w = SC.planted_warp(seed, n, n + 5 + 2 * seed)
        swap = seed % 2  # the roles swapped on every other pair
        pairs.append((len(maps) + 1, len(maps)) if swap else (len(maps), len(maps) + 1))
        maps += [a, b]
        ws.append((w, swap))
    summaries, path = _device(model, maps, pairs, None, "device")
    for (w, swap), s in zip(ws, summaries):
        got = path[int(s["path_first"]) : int(s["path_first"]) + int(s["n_path"])]
        want = np.stack([w, np.arange(len(w))], axis=1)
        assert s["status"] == 0 and np.array_equal(got, want[:, ::-1] if swap else want)
        assert s["total"] == (int(s["units_a"]) + int(s["units_b"])) * 65025
    _assert_equal((summaries, path), _host(maps, pairs), "planted")


# ---- clips and the Python entries
def _float_clips(model, sr):
    return [(c.astype(np.float32) / np.float32(32768.0)).reshape(-1, 1) for c in TS._clips_at(model, sr)]


def test_clips_through_the_model_and_the_python_entries(model):
    import torch

    from basic_pitch_amd import clips as CL, sync as SY

    clips = _float_clips(model, 22050) + [_float_clips(model, 22050)[1][::-1].copy()]
    arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
    outs = [model.predict_pcm(c, 22050) for c in clips]
    rows = [len(o["note"]) for o in outs]
    assert rows[0] == 0 and min(rows[1:]) > 100
    pairs = [(1, 2), (2, 3), (3, 3), (0, 1), (2, 1)]
    got = SY.infer_clips_sync(model, arrays, 22050, pairs)
    notes = [np.asarray(o["note"], np.float32).reshape(-1, 88) for o in outs]
    _assert_equal(got, _device(model, notes, pairs), "bp_infer_clips_sync against bp_sync_from_maps")
    _assert_equal(got, _host(notes, pairs), "bp_infer_clips_sync against the checker")
    assert got[0]["status"].tolist() == [0, 0, 0, 2, 0]
    # the Python entries, across two sample rates
    mixed = clips[1:3] + _float_clips(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    m_outs = [model.predict_pcm(c, r) for c, r in zip(mixed, rates)]
    m_pairs = [(2, 3), (0, 1), (1, 1), (3, 2)]
    for how in (dict(), dict(hop=2, band=10, threshold_q=200)):
        via_clips = model.transcribe_clips_sync(mixed, rates, m_pairs, **how)
        via_maps = model.sync_pairs(m_outs, m_pairs, **how)
        via_dev = model.sync_pairs([{k: torch.from_numpy(np.asarray(v)).cuda() for k, v in o.items()} for o in m_outs], m_pairs, **how)
        for (a, b), x, y, z in zip(m_pairs, via_clips, via_maps, via_dev):
            s, region = SY.sync_rows(m_outs[a]["note"], m_outs[b]["note"], how)
            host = SY.Sync.of(s[0], region, how.get("hop", 4))
            for r in (x, y, z):
                assert (r.status, r.total, r.units_a, r.units_b, r.hop) == (host.status, host.total, host.units_a, host.units_b, host.hop)
                assert r.path.dtype == np.int32 and r.path.tobytes() == host.path.tobytes() and r.status == 0
    both = model.sync(m_outs[:2], m_outs[2:])
    assert [(r.status, r.total) for r in both] == [(r.status, r.total) for r in model.sync_pairs(m_outs, [(0, 2), (1, 3)])]
    with pytest.raises(ValueError, match=r"pair 1 = \(1, 2\).*Model.sync"):
        model.transcribe_clips_sync(mixed, rates, [(0, 1), (1, 2)])
    with pytest.raises(ValueError):
        model.sync(m_outs[:2], m_outs[:1])
    with pytest.raises(TypeError):
        model.sync_pairs(m_outs, m_pairs, threshold=0.3)
    assert model.sync([], []) == [] and model.sync_pairs(m_outs, []) == []


def test_map_times_and_transfer_notes(model):
    from basic_pitch_amd import sync as SY

    a, b, w = SC.planted_warp(5, 30, 47)
    s = model.sync([{"note": a}], [{"note": b}])[0]
    assert s.status == 0 and np.array_equal(s.path[:, 0], w)
    t = np.linspace(-0.5, 2.0, 400)
    for to in ("b", "a"):
        mapped = s.map_times(t, to)
        assert mapped.dtype == np.float64 and np.all(np.diff(mapped) >= 0), to  # monotone
    # unit 3 of a is matched with the run of b's units where w == 3: its centre goes to the mean of theirs
    centre = lambda u: float(SY._frame_time(np.array([(u + 0.5) * 4]))[0])  # noqa: E731
    run = np.flatnonzero(w == 3)
    assert abs(float(s.map_times([centre(3)])[0]) - np.mean([centre(j) for j in run])) < 1e-12
    # the identity within half a unit on a pair whose path is the diagonal
    chords = SC.chord_map(1, 40)
    same = model.sync_pairs([{"note": chords}], [(0, 0)])[0]
    assert np.array_equal(same.path, np.stack([np.arange(40)] * 2, axis=1))
    half_unit = centre(1) - centre(0.5)
    t = np.linspace(0.0, centre(39.5), 300)
    assert np.all(np.abs(same.map_times(t) - t) <= half_unit + 1e-12)
    inside = t[(t >= centre(0)) & (t <= centre(39))]
    assert np.all(np.abs(same.map_times(inside) - inside) < 1e-9)
    notes = np.array([[0.05, 0.30, 60.0], [0.30, 0.31, 64.5], [0.2, 1.0, 33.0], [1.4, 1.4, 72.0]])
    moved = s.transfer_notes(notes)
    assert moved.shape == (4, 3) and np.array_equal(moved[:, 2], notes[:, 2]) and np.all(moved[:, 1] >= moved[:, 0])
    back = s.transfer_notes(moved, to="a")
    assert np.all(back[:, 1] >= back[:, 0]) and np.array_equal(back[:, 2], notes[:, 2])
    with pytest.raises(ValueError):
        s.map_times(t, to="c")


# ---- the non-default handles
@pytest.mark.parametrize("mode", ["bf16_weights", "ext_cqt_44k"])
def test_on_the_non_default_handles_the_call_equals_the_checker_on_that_handles_own_maps(mode):
    from basic_pitch_amd import clips as CL, sync as SY
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8, **{mode: True}) as m:
        sr = m.sample_rate
        clips = _float_clips(m, sr)[1:]
        arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
        notes = [np.asarray(m.predict_pcm(c, sr)["note"], np.float32) for c in clips]
        pairs = [(0, 1), (1, 0), (1, 1)]
        want = _host(notes, pairs)
        _assert_equal(SY.infer_clips_sync(m, arrays, sr, pairs), want, (mode, "clips"))
        _assert_equal(_device(m, notes, pairs), want, (mode, "maps"))
        assert want[0]["status"].tolist() == [0, 0, 0] and min(len(n) for n in notes) > 100
