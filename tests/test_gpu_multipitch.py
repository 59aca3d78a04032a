"""Multi-pitch estimates on the device (include/basic_pitch_amd_multipitch.h; csrc/multipitch.hip): the points of
bp_multipitch_from_maps are byte for byte those of the host checker bp_multipitch_rows, segment by segment — maps in host and
in device memory, several sets, a job that takes more than one pass of the scan with a dense segment across the pass's end —,
the capacity protocol writes nothing past the caller's room, clips through the model give the points of their own contour
rows, and every decode of a threshold / band sweep has the frame counts bp_score_f0_frames gives on the points of its
segment under its set, with statuses 1 and 3, the refusals, and the Python entries."""
import ctypes as C

import numpy as np
import pytest

import multipitch_cases as MC
import score_cases as SC
import test_gpu_score as TG
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

FIELDS = ("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub")
INV = -1
SETS = [dict(threshold=t, min_bin=lo, max_bin=hi) for t, lo, hi in
        ((0.3, 1, 262), (0.5, 1, 262), (0.1, 1, 262), (0.8, 1, 262), (0.3, 60, 200), (0.3, 144, 144), (-1.0, 1, 262), (0.6, 2, 100))]
POINT_SETS = [MC.DEFAULT, dict(threshold=0.3, min_bin=100, max_bin=100), dict(threshold=10.0, min_bin=1, max_bin=262),
              dict(threshold=-1.0, min_bin=1, max_bin=262)]  # the default, a narrow band, above every cell, negative


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host_points(segs, prm):
    """The host checker on every segment: (points of all, point_offsets, statuses)."""
    from basic_pitch_amd import multipitch as MP

    parts, status = [], []
    for c in segs:
        pts, st = MP.multipitch_rows(c, prm)
        parts.append(pts)
        status.append(st)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts) if parts else np.zeros(0, MC.POINT), offs, np.array(status, np.int32)


def _assert_equal(got, want, where):
    (pts, offs, st), (w_pts, w_offs, w_st) = got, want
    assert offs.tolist() == w_offs.tolist(), where
    assert st.tolist() == w_st.tolist(), where
    assert pts.tobytes() == w_pts.tobytes(), where  # the point records as raw bytes


@pytest.fixture(scope="module")
def job():
    """The segment job (rows 0, 1, 2, 63, 64, 65, 142, 173, 433: bumps and dense noise alternating, the crafted rows in the
    segment of 65) and the host checker's points under POINT_SETS, computed once."""
    segs = MC.segment_job()
    offs, cat = MC.stack(segs)
    assert np.diff(offs).tolist() == list(MC.SEGMENT_ROWS)
    return dict(segs=segs, offs=offs, cat=cat, want=[_host_points(segs, prm) for prm in POINT_SETS])


# ---- the points
@pytest.mark.parametrize("where", ["host", "device"])
def test_the_points_are_the_host_checkers_byte_for_byte(model, job, where):
    import torch

    from basic_pitch_amd import _native, multipitch as MP

    if where == "host":
        ptr, kind, before = job["cat"].ctypes.data, _native.BP_MEM_HOST, job["cat"].copy()
    else:
        dev = torch.from_numpy(job["cat"]).cuda()
        torch.cuda.synchronize()
        ptr, kind = dev.data_ptr(), _native.BP_MEM_DEVICE
    n_points = []
    for prm, want in zip(POINT_SETS, job["want"]):
        _assert_equal(MP.multipitch_from_maps(model, job["offs"], ptr, kind, prm), want, (where, prm))
        n_points.append(len(want[0]))
    assert n_points[0] > 1000 and n_points[1] > 0 and n_points[2] == 0 and n_points[3] > 50000, n_points
    # the map is left untouched
    after = job["cat"] if where == "host" else dev.cpu().numpy()
    assert after.tobytes() == (before if where == "host" else job["cat"]).tobytes()


def test_a_job_of_more_than_one_scan_pass_carries_the_sum_across_a_dense_segment(model):
    """Total rows above BP_MP_SCAN_TILE_ROWS (1,024, imported from the binding): a segment boundary inside the first pass (at
    500 and 900) and a dense-noise segment over rows 900 ... 1,199, across the pass's end."""
    from basic_pitch_amd import _native, multipitch as MP

    tile = MP.SCAN_TILE_ROWS
    assert tile == 1024
    rng = np.random.default_rng(11)
    segs = [MC.bumps(rng, 500), MC.dense(rng, 400), MC.dense(rng, 300), MC.bumps(rng, 0), MC.bumps(rng, 7)]
    offs, cat = MC.stack(segs)
    assert offs[2] < tile < offs[3] and offs[-1] >= tile + 1
    for prm in (MC.DEFAULT, POINT_SETS[3]):
        _assert_equal(MP.multipitch_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, prm), _host_points(segs, prm), prm)
    # exactly one pass and one row more, as one segment
    for rows in (tile, tile + 1):
        c = MC.dense(rng, rows)
        _assert_equal(MP.multipitch_from_maps(model, [0, rows], c.ctypes.data, _native.BP_MEM_HOST, None), _host_points([c], None), rows)


def test_a_segment_with_a_cell_that_is_not_finite_has_no_points_and_its_neighbours_theirs(model, job):
    from basic_pitch_amd import _native, multipitch as MP

    segs = [c.copy() for c in job["segs"]]
    segs[4] = MC.with_nonfinite(segs[4], np.nan, 63, 263)    # outside every band, the last cell of the segment
    segs[7] = MC.with_nonfinite(segs[7], -np.inf, 0, 0)      # the first cell of the segment
    offs, cat = MC.stack(segs)
    prm = dict(threshold=0.3, min_bin=50, max_bin=200)
    got = MP.multipitch_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, prm)
    want = _host_points(segs, prm)
    assert want[2].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0]
    _assert_equal(got, want, "status 1")
    assert got[1][5] == got[1][4] and got[1][8] == got[1][7] and len(got[0]) > 0


def test_too_little_room_writes_nothing_and_the_repeat_succeeds(model, job):
    from basic_pitch_amd import _native, events as EV, multipitch as MP

    lib = MP.bind(model._lib)
    h, offs, cat = model._handle, job["offs"], job["cat"]
    want_pts, want_offs, want_st = job["want"][0]
    need = len(want_pts)
    # a small events job on the same handle, before and after
    rng = np.random.default_rng(3)
    seg_cat, seg_offs = TS._cat([TS._segment(rng, 142)])
    note_prm = TS._prm(TS.BASE)
    events_before = EV.note_events_from_maps(model, seg_offs, *TG._ptrs(seg_cat, seg_offs), _native.BP_MEM_HOST, note_prm)
    p = MP.mp_params()
    canary = 64
    buf = np.zeros(need + canary, MC.POINT)
    buf.view(np.uint8)[:] = 0xA5
    p_offs, st = np.full(len(offs), -1, np.int64), np.full(len(offs) - 1, -1, np.int32)
    args = (h, len(offs) - 1, _p64(offs), cat.ctypes.data, _native.BP_MEM_HOST, C.addressof(p))
    rc = lib.bp_multipitch_from_maps(*args, buf.ctypes.data, need - 1, _p64(p_offs), st.ctypes.data)
    msg = lib.bp_last_error(h).decode()
    assert rc == INV and f"{need} points are needed" in msg and "bp_multipitch_from_maps" in msg, msg
    assert p_offs.tolist() == want_offs.tolist() and st.tolist() == want_st.tolist()  # complete
    assert np.all(buf.view(np.uint8) == 0xA5), "a refused call wrote to points"
    rc = lib.bp_multipitch_from_maps(*args, buf.ctypes.data, need, _p64(p_offs), st.ctypes.data)
    assert rc == 0 and buf[:need].tobytes() == want_pts.tobytes()
    assert np.all(buf[need:].view(np.uint8) == 0xA5), "the canary behind points"
    events_after = EV.note_events_from_maps(model, seg_offs, *TG._ptrs(seg_cat, seg_offs), _native.BP_MEM_HOST, note_prm)
    n_ev = int(events_before[2][-1])
    assert n_ev > 0 and events_after[2].tolist() == events_before[2].tolist() and events_after[3].tolist() == events_before[3].tolist()
    assert bytes(events_after[0])[: n_ev * C.sizeof(_native.bp_note_event)] == bytes(events_before[0])[: n_ev * C.sizeof(_native.bp_note_event)]


def test_nothing_to_do_and_the_refusals(model, job):
    from basic_pitch_amd import _native, multipitch as MP

    lib = MP.bind(model._lib)
    h, offs, cat = model._handle, job["offs"], job["cat"]
    p = MP.mp_params()
    p_offs, st = np.full(len(offs), -1, np.int64), np.full(len(offs), -1, np.int32)
    buf = np.zeros(10, MC.POINT)
    zero = np.zeros(4, np.int64)
    # zero segments, and segments without rows: BP_OK, zeroed offsets
    assert lib.bp_multipitch_from_maps(h, 0, _p64(zero), None, 0, C.addressof(p), None, 0, _p64(p_offs), None) == 0 and p_offs[0] == 0
    assert lib.bp_multipitch_from_maps(h, 3, _p64(zero), None, 0, C.addressof(p), None, 0, _p64(p_offs), st.ctypes.data) == 0
    assert p_offs[:4].tolist() == [0, 0, 0, 0] and st[:3].tolist() == [0, 0, 0]

    def refused(said, n=len(offs) - 1, o=offs, c=cat.ctypes.data, kind=0, prm=p, pts=buf.ctypes.data, room=10, po=p_offs, s=st):
        rc = lib.bp_multipitch_from_maps(h, n, _p64(o) if o is not None else None, c, kind, C.addressof(prm) if prm is not None else None,
                                         pts, room, _p64(po) if po is not None else None, s.ctypes.data if s is not None else None)
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and said in msg, (said, rc, msg)

    refused("negative n_segments", n=-1)
    refused("null point_offsets or status", po=None)
    refused("null point_offsets or status", s=None)
    refused("room without a buffer", pts=None)
    refused("negative max_points", room=-1)
    refused("row_offsets must start at 0", o=np.array([1, 2] + [3] * 8, np.int64))
    refused("row_offsets must start at 0", o=np.array([0, 5, 4] + [6] * 7, np.int64))
    refused("mem_kind", kind=7)
    refused("null input pointer", c=None)
    refused("null params", prm=None)
    for fields, named in ((dict(threshold=np.nan), "threshold"), (dict(min_bin=0), "min_bin"), (dict(max_bin=263), "max_bin"),
                          (dict(min_bin=9, max_bin=8), "min_bin"), (dict(reserved=2), "reserved")):
        refused(named, prm=MP.mp_params(**fields))
    big = np.array([0, 8388608 + 1], np.int64)
    refused("BP_SWEEP_MAX_ROWS", n=1, o=big)
    # the handle is usable
    _assert_equal(MP.multipitch_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, None), job["want"][0], "after the refusals")


# ---- clips through the model
def test_clips_through_the_model_give_the_points_of_their_own_contour_rows(model):
    """One- and two-window PCM clips (and one of 100 samples) at two sample rates through bp_infer_clips_multipitch against
    bp_multipitch_from_maps on the contour rows of each clip ALONE through Model.predict_pcm_raw (bp_infer_pcm_raw): the route
    the clips tests compare the batched candidates with, whose maps equal the clips driver's bit for bit."""
    from basic_pitch_amd import _native, clips as CL, multipitch as MP

    n_points = 0
    for sr in (22050, 44100):
        arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(model, sr))]
        rows = np.diff(CL.clips_row_offsets(model, arrays, sr))
        contours = [model.predict_pcm_raw(a.tobytes(), CL.FORMATS[a.dtype], a.shape[0], a.shape[1], sr)["contour"] for a in arrays]
        assert [len(c) for c in contours] == rows.tolist() and rows[0] == 0 and 0 < rows[1] < rows[2]
        offs, cat = MC.stack(contours)
        for prm in (None, dict(threshold=0.15, min_bin=30, max_bin=230)):
            got = MP.infer_clips_multipitch(model, arrays, sr, prm)
            _assert_equal(got, MP.multipitch_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, prm), (sr, prm))
            _assert_equal(got, _host_points(contours, prm), (sr, prm, "host checker"))
            n_points += len(got[0])
    assert n_points > 500


# ---- sweeps scored where the peaks are
def _want_scores(segs, sets, refs, pairs, **tolerances):
    """bp_multipitch_rows + bp_score_f0_frames per decode: the five counts and the status."""
    from basic_pitch_amd import multipitch as MP

    out, cache = [], {}
    for s, p in pairs:
        if (s, p) not in cache:
            pts, st = MP.multipitch_rows(segs[s], sets[p])
            if st:
                cache[(s, p)] = (len(segs[s]), 0, 0, 0, 0, st)
            else:
                c = MP.score_f0_frames(pts, refs[s], len(segs[s]), **tolerances)
                cache[(s, p)] = tuple(int(c[f]) for f in FIELDS) + (0,)
        out.append(cache[(s, p)])
    return out


def _tuples(counts):
    return [tuple(int(c[f]) for f in FIELDS + ("status",)) for c in np.asarray(counts).reshape(-1)]


@pytest.fixture(scope="module")
def sweep_job(job):
    from basic_pitch_amd import sweep as SW

    rng = np.random.default_rng(21)
    refs = [MC.refs_for(rng, c, MC.DEFAULT, n=14) if len(c) else SC.notes([(0.0, 1.0, 60.0)]) for c in job["segs"]]
    pairs = SW.cross_product(len(SETS), len(job["segs"]))
    return dict(refs=refs, pairs=pairs, want=_want_scores(job["segs"], SETS, refs, pairs))


def test_the_reference_of_the_sweep_is_not_trivial(sweep_job):
    want = sweep_job["want"]
    assert len(want) == 8 * 9 and all(w[5] == 0 for w in want), "a decode of the main job without status 0: the test is built wrong"
    tp, sub = [w[3] for w in want], [w[4] for w in want]
    miss = [w[1] - w[3] - w[4] for w in want]
    fa = [w[2] - w[3] - w[4] for w in want]
    assert max(tp) > 0 and max(sub) > 0 and max(miss) > 0 and max(fa) > 0
    assert len({w[:5] for w in want}) >= 30


@pytest.mark.parametrize("where", ["host", "device"])
def test_the_cross_product_equals_from_maps_plus_the_frame_checker(model, job, sweep_job, where):
    import torch

    from basic_pitch_amd import _native, multipitch as MP

    if where == "host":
        ptr, kind = job["cat"].ctypes.data, _native.BP_MEM_HOST
    else:
        dev = torch.from_numpy(job["cat"]).cuda()
        torch.cuda.synchronize()
        ptr, kind = dev.data_ptr(), _native.BP_MEM_DEVICE
    got = MP.multipitch_sweep_frame_score(model, job["offs"], ptr, kind, SETS, sweep_job["refs"])
    assert _tuples(got) == sweep_job["want"]
    # ... and the points those counts are of are bp_multipitch_from_maps' own
    for p in (0, 5):
        pts, offs, st = MP.multipitch_from_maps(model, job["offs"], ptr, kind, SETS[p])
        _assert_equal((pts, offs, st), _host_points(job["segs"], SETS[p]), p)
    # another tolerance, strict
    tol = dict(pitch_tolerance_cents=70.0, strict=1)
    got = MP.multipitch_sweep_frame_score(model, job["offs"], ptr, kind, SETS[:3], sweep_job["refs"], **tol)
    assert _tuples(got) == _want_scores(job["segs"], SETS, sweep_job["refs"], [q for q in sweep_job["pairs"] if q[1] < 3], **tol)


def test_an_explicit_table_with_repeated_pairs_equals_its_own_permutation(model, job, sweep_job):
    from basic_pitch_amd import _native, multipitch as MP

    rng = np.random.default_rng(5)
    pairs = sweep_job["pairs"]
    order = list(rng.permutation(len(pairs))[:40]) + [17, 17, 40, len(pairs) - 1, len(pairs) - 1]
    got = MP.multipitch_sweep_frame_score(model, job["offs"], job["cat"].ctypes.data, _native.BP_MEM_HOST, SETS, sweep_job["refs"],
                                          [pairs[k] for k in order])
    assert _tuples(got) == [sweep_job["want"][k] for k in order]


@pytest.mark.parametrize("rows", [2048, 2049])
def test_a_job_with_a_long_decode_takes_the_wide_workgroups_and_counts_the_same(model, rows):
    """A job whose longest decode has more than 2,048 rows (csrc/bp_kernels.h kMpSweepLongRows) is scored by workgroups of 16
    waves instead of 4: the last size of the one form and the first of the other, a short segment beside the long one."""
    from basic_pitch_amd import _native, multipitch as MP

    rng = np.random.default_rng(rows)
    segs = [MC.bumps(rng, rows), MC.dense(rng, 65)]
    segs[0][1000:1040] = MC.dense(rng, 40)
    offs, cat = MC.stack(segs)
    sets = SETS[:3]
    refs = [MC.refs_for(rng, c, MC.DEFAULT, n=40) for c in segs]
    pairs = [(s, p) for p in range(3) for s in range(2)]
    want = _want_scores(segs, sets, refs, pairs)
    assert all(w[5] == 0 for w in want) and sum(w[3] for w in want) > 0 and sum(w[4] for w in want) > 0
    assert _tuples(MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, refs)) == want


def test_a_ref_at_the_exact_tolerance_and_a_chain(model):
    """A row with peaks whose refined pitches are exactly 60.0 and 61.0 (symmetric neighbours: delta 0) against refs 60.5
    (hits both at exactly 50 cents) and 60.4 (hits 60 alone): 2 when not strict — only by giving 60.5 the higher peak —,
    1 when strict."""
    from basic_pitch_amd import _native, multipitch as MP

    c = np.zeros((3, 264), np.float32)
    for b in (117, 120):  # MIDI 60 and 61
        c[1, b - 1 : b + 2] = (0.2, 0.7, 0.2)
    refs = [SC.notes([(SC.frame_time(1), SC.frame_time(2), 60.5), (SC.frame_time(1), SC.frame_time(2), 60.4)])]
    for strict, tp in ((0, 2), (1, 1)):
        got = MP.multipitch_sweep_frame_score(model, [0, 3], c.ctypes.data, _native.BP_MEM_HOST, [MC.DEFAULT], refs, strict=strict)
        assert _tuples(got) == [(3, 2, 2, tp, 2 - tp, 0)] == _want_scores([c], [MC.DEFAULT], refs, [(0, 0)], strict=strict)


def test_statuses_1_and_3_leave_the_zero_record_and_their_neighbours_alone(model, job, sweep_job):
    from basic_pitch_amd import _native, multipitch as MP

    segs = [c.copy() for c in job["segs"]]
    segs[5] = MC.with_nonfinite(segs[5], np.inf, 30, 0)
    offs, cat = MC.stack(segs)
    refs = list(sweep_job["refs"])
    many = np.tile(SC.notes([(0.0, 0.5, 60.0)]), (16384 + 1, 1))  # one more than BP_SCORE_MAX_NOTES
    refs[7] = many
    sets = SETS[:2]
    got = _tuples(MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, refs))
    for j, (s, p) in enumerate((s, p) for p in range(2) for s in range(9)):
        if s == 5:
            assert got[j] == (65, 0, 0, 0, 0, 1)
        elif s == 7:
            assert got[j] == (173, 0, 0, 0, 0, 3)
        else:
            assert got[j] == sweep_job["want"][p * 9 + s], (s, p)
    # the Python entry finishes status 3 on the host, and reports status 1 as it is
    outputs = [{"contour": c} for c in segs]
    counts = model.sweep_multipitch_frame_scores(outputs, sets, refs)
    assert counts.shape == (2, 9)
    for p in range(2):
        pts, _ = MP.multipitch_rows(segs[7], sets[p])
        host = MP.score_f0_frames(pts, many, 173)
        rec = counts[p, 7]
        assert rec["status"] == 3 and tuple(int(rec[f]) for f in FIELDS) == tuple(int(host[f]) for f in FIELDS) and rec["ref_frames"] > 0
        assert tuple(int(counts[p, 5][f]) for f in FIELDS + ("status",)) == (65, 0, 0, 0, 0, 1)
        assert _tuples(counts[p, [0, 1, 2, 3, 4, 6, 8]]) == [sweep_job["want"][p * 9 + s] for s in (0, 1, 2, 3, 4, 6, 8)]


def test_clips_through_the_model_are_scored_as_their_maps_are(model):
    from basic_pitch_amd import _native, clips as CL, multipitch as MP

    rng = np.random.default_rng(8)
    for sr in (22050, 44100):
        arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(model, sr))]
        contours = [model.predict_pcm_raw(a.tobytes(), CL.FORMATS[a.dtype], a.shape[0], a.shape[1], sr)["contour"] for a in arrays]
        sets = [dict(threshold=t, min_bin=1, max_bin=262) for t in (0.1, 0.3, 0.5)]
        refs = [MC.refs_for(rng, c, sets[0], n=10) if len(c) else SC.notes([]) for c in contours]
        pairs = [(s, p) for p in range(3) for s in range(3)]
        want = _want_scores(contours, sets, refs, pairs)
        assert sum(w[3] for w in want) > 0 and all(w[5] == 0 for w in want)
        assert _tuples(MP.infer_clips_multipitch_sweep_frame_score(model, arrays, sr, sets, refs)) == want
        offs, cat = MC.stack(contours)
        assert _tuples(MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, refs)) == want
    mixed = TS._clips_at(model, 22050)[1:] + TS._clips_at(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    counts = model.transcribe_clips_sweep_multipitch_frame_scores(mixed, rates, [MC.DEFAULT], [SC.notes([])] * 4)
    rows = [int(np.diff(CL.clips_row_offsets(model, [CL.as_clip(c, 0)], r))[0]) for c, r in zip(mixed, rates)]
    assert counts.shape == (1, 4) and counts["n_frames"].tolist() == [rows] and min(rows) > 0 and np.all(counts["est_frames"] > 0)


def test_the_refusals_of_the_sweep_name_the_index_and_leave_the_handle_usable(model, job, sweep_job):
    from basic_pitch_amd import _native, multipitch as MP, score, sweep as SW

    lib = MP.bind(model._lib)
    h, offs, cat = model._handle, job["offs"], job["cat"]
    ref_offs, flat = score.refs_table(sweep_job["refs"])
    prm = score.score_params()
    n_seg = len(offs) - 1
    frames, st = np.zeros((64, 5), np.int64), np.zeros(64, np.int32)

    def refused(said, sets=SETS[:2], n_decodes=2 * n_seg, pairs=None, ro=ref_offs, refs=flat, sp=prm, fr=frames):
        arr = MP.sets_array(sets)
        tab = SW.decode_table(pairs) if pairs is not None else None
        rc = lib.bp_multipitch_sweep_frame_score(h, n_seg, _p64(offs), cat.ctypes.data, _native.BP_MEM_HOST, len(sets), C.addressof(arr),
                                                 n_decodes, C.addressof(tab) if tab is not None else None, _p64(ro) if ro is not None else None,
                                                 refs.ctypes.data, C.addressof(sp), fr.ctypes.data if fr is not None else None, st.ctypes.data)
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and said in msg and "bp_multipitch_sweep_frame_score" in msg, (said, rc, msg)

    refused("set 1: max_bin", sets=[MC.DEFAULT, dict(threshold=0.3, min_bin=1, max_bin=263)])
    refused("set 0: the threshold", sets=[dict(threshold=np.inf, min_bin=1, max_bin=262), MC.DEFAULT])
    refused("n_decodes is not n_sets * n_segments", n_decodes=2 * n_seg - 1)
    refused("decode 1: params 2", n_decodes=2, pairs=[(0, 0), (1, 2)])
    refused("decode 1: segment 9", n_decodes=2, pairs=[(0, 0), (9, 1)])
    refused("BP_SWEEP_MAX_DECODES", n_decodes=65537)
    refused("null ref_offsets or frames", fr=None)
    refused("null ref_offsets or frames", ro=None)
    bad = flat.copy()
    bad[3, 2] = np.nan
    refused("ref 3:", refs=bad)
    dec = ref_offs.copy()
    dec[2] = dec[1] - 1 if dec[1] > 0 else dec[3] + 1
    refused("segment 1: ref_offsets decrease" if dec[1] > 0 else "ref_offsets decrease", ro=dec)
    refused("tolerance", sp=score.score_params(pitch_tolerance_cents=-1.0))
    got = MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, SETS[:2], sweep_job["refs"])
    assert _tuples(got) == sweep_job["want"][: 2 * n_seg]
    # nothing to do is no error: no decodes; decodes of segments without rows alone
    assert len(MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, SETS[:2], sweep_job["refs"], [])) == 0
    empty = MP.multipitch_sweep_frame_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, SETS[:2], sweep_job["refs"], [(0, 0), (0, 1)])
    assert _tuples(empty) == [(0, 0, 0, 0, 0, 0)] * 2


# ---- the Python entries
def test_model_multipitch_takes_host_and_device_outputs(model, job):
    import torch

    from basic_pitch_amd.note_creation import model_frames_to_time

    outputs = [{"contour": c} for c in job["segs"]]
    want_pts, want_offs, _ = job["want"][0]
    for outs in (outputs, [{"contour": torch.from_numpy(c).cuda()} for c in job["segs"]]):
        ests = model.multipitch(outs)
        assert len(ests) == 9
        for i, est in enumerate(ests):
            w = want_pts[int(want_offs[i]) : int(want_offs[i + 1])]
            assert est.status == 0 and est.frames.tolist() == w["frame"].tolist()
            assert est.pitch_midi.tobytes() == w["pitch_midi"].tobytes() and est.salience.tobytes() == w["salience"].tobytes()
            assert np.array_equal(est.times_s, model_frames_to_time(max(1, len(job["segs"][i])))[est.frames])
            assert np.array_equal(est.freqs_hz, 440.0 * np.exp2((est.pitch_midi - 69.0) / 12.0))
    assert model.multipitch([]) == []
    narrow = model.multipitch(outputs, dict(threshold=0.3, min_bin=100, max_bin=100))
    assert sum(len(e.frames) for e in narrow) == len(job["want"][1][0])


def test_transcribe_clips_multipitch_groups_the_rates(model):
    from basic_pitch_amd import clips as CL, multipitch as MP

    clips = TS._clips_at(model, 22050)[1:] + TS._clips_at(model, 44100)[1:]
    rates = [22050, 44100, 22050, 44100]
    clips = [clips[0], clips[2], clips[1], clips[3]]
    ests = model.transcribe_clips_multipitch(clips, rates)
    for c, r, est in zip(clips, rates, ests):
        a = CL.as_clip(c, 0)
        pts, offs, st = MP.infer_clips_multipitch(model, [a], r)
        assert est.status == 0 and len(est.frames) > 0 and est.pitch_midi.tobytes() == pts["pitch_midi"].tobytes()


def test_a_440_hz_sine_has_its_strongest_peak_at_the_bin_of_midi_69(model):
    """A pure 440 Hz sine (amplitude 0.5, one window) through Model.predict + Model.multipitch: on the frames of its steady
    part (20 ... 149) the peak with the largest salience of its frame is at bin 144 +- 1 (MIDI 69 is bin 144).

    MEASURED, not fixed in advance: the same window through the CPU oracle (oracle/bp_oracle.py forward, float64) and
    bp_multipitch_rows has that peak at bin 145 on every one of those frames, its refined pitch 0.3497 semitones above MIDI
    69 at worst (0.3498 with the float32 oracle).  The oracle itself strays by more than a third of a semitone — one bin —
    so a margin in semitones is not what the model supports; the gate is "the peak's bin is 144 +- 1" alone."""
    from basic_pitch_amd.constants import AUDIO_N_SAMPLES

    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(AUDIO_N_SAMPLES) / 22050.0)).astype(np.float32)[None, :]
    out = model.predict(x)
    est = model.multipitch([{"contour": np.asarray(out["contour"]).reshape(-1, 264)}])[0]
    assert est.status == 0
    for fr in range(20, 150):
        on = np.flatnonzero(est.frames == fr)
        assert len(on), fr
        top = on[np.argmax(est.salience[on])]
        bin_ = int(np.rint((est.pitch_midi[top] - 21.0) * 3.0))
        assert abs(bin_ - 144) <= 1, (fr, bin_, est.pitch_midi[top])
