"""The melody decode on the device (include/basic_pitch_amd_melody.h; csrc/melody.hip): the records of bp_melody_from_maps are
byte for byte those of the host checker bp_melody_rows, segment by segment — maps in host and in device memory, every case map,
every set of melody_cases.SETS, segment lengths around the read-ahead depth and the tile seams of the backtrace —, too little
room writes nothing, clips through the model give the records of their own contour rows, and every decode of a scored sweep has
the counts bp_score_melody_frames gives on the records of its segment under its set, with status 1, the refusals, and the
Python entries."""
import ctypes as C

import numpy as np
import pytest

import melody_cases as MC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

FIELDS = ("n_frames", "ref_voiced", "est_voiced", "both_voiced", "pitch_ok", "chroma_ok")
INV = -1
DEPTH, TILE = 8, 128  # BP_MELODY_READ_AHEAD, BP_MELODY_TILE_ROWS (compared with the binding's below)
# 0, 1, 2; one below / at / one above the read-ahead depth; TILE - 1, TILE, TILE + 1; 2 TILE + 1; 433 — the smallest shapes at
# which the pipeline fill, the tile seam of the backtrace and the last partial tile can go wrong — and 433 rows of the other kinds
SEGMENT_ROWS = (0, 1, 2, DEPTH - 1, DEPTH, DEPTH + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 433, 433, 433)
KINDS = ("glide", "noise", "quantised") * 3 + ("glide", "noise", "glide", "quantised")


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host_records(segs, prm):
    """The host checker on every segment: (records of all rows, statuses)."""
    from basic_pitch_amd import melody as ME

    parts, status = [], []
    for c in segs:
        pts, st = ME.melody_rows(c, MC.params(**prm) if prm is not None else None)
        parts.append(pts)
        status.append(st)
    return np.concatenate(parts) if parts else np.zeros(0, MC.POINT), np.array(status, np.int32)


def _assert_equal(got, want, where):
    (pts, st), (w_pts, w_st) = got, want
    assert st.tolist() == w_st.tolist(), where
    assert len(pts) == len(w_pts) and pts.tobytes() == w_pts.tobytes(), where  # the records as raw bytes


@pytest.fixture(scope="module")
def job():
    """The segment job and the host checker's records under every set of MC.SETS, computed once."""
    from basic_pitch_amd import melody as ME

    assert (ME.READ_AHEAD, ME.TILE_ROWS) == (DEPTH, TILE)
    segs = [dict(MC.case_maps(r, seed=i))[kind] for i, (r, kind) in enumerate(zip(SEGMENT_ROWS, KINDS))]
    offs, cat = MC.stack(segs)
    assert np.diff(offs).tolist() == list(SEGMENT_ROWS)
    return dict(segs=segs, offs=offs, cat=cat, want=[_host_records(segs, prm) for prm in MC.SETS])


def _where(job, where):
    import torch

    from basic_pitch_amd import _native

    if where == "host":
        return job["cat"].ctypes.data, _native.BP_MEM_HOST, None
    dev = torch.from_numpy(job["cat"]).cuda()
    torch.cuda.synchronize()
    return dev.data_ptr(), _native.BP_MEM_DEVICE, dev


# ---- the records
@pytest.mark.parametrize("where", ["host", "device"])
def test_the_records_are_the_host_checkers_byte_for_byte(model, job, where):
    from basic_pitch_amd import melody as ME

    ptr, kind, dev = _where(job, where)
    before = job["cat"].copy()
    voiced = []
    for prm, want in zip(MC.SETS, job["want"]):
        _assert_equal(ME.melody_from_maps(model, job["offs"], ptr, kind, MC.params(**prm)), want, (where, prm))
        voiced.append(int((want[0]["bin"] >= 0).sum()))
        assert want[1].tolist() == [0] * len(SEGMENT_ROWS)
    assert min(voiced) > 100 and max(voiced) < len(job["cat"]), voiced
    # the map is left untouched
    after = job["cat"] if where == "host" else dev.cpu().numpy()
    assert after.tobytes() == before.tobytes()


def test_both_window_widths_of_the_kernel_give_the_checkers_records(model):
    """A call whose sets all have max_jump <= 4 reads windows of 4 bins on either side, any other of 16 (csrc/bp_kernels.h
    kMelodyNarrowJump): the last set of the one form and the first of the other on a voice that moves by up to 6 bins a row,
    alone (each its own call) and together in one scored sweep, where both decodes take the wide form."""
    from basic_pitch_amd import _native, melody as ME

    segs = [dict(MC.case_maps(257, seed=5))["glide"], dict(MC.case_maps(129, seed=6))["noise"]]
    offs, cat = MC.stack(segs)
    sets = [dict(max_jump=4, jump_penalty=0.01), dict(max_jump=5, jump_penalty=0.01)]
    most = []
    for prm in sets:
        want = _host_records(segs, prm)
        _assert_equal(ME.melody_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, MC.params(**prm)), want, prm)
        widest = 0
        for i in range(2):  # (jumps within a segment: the records of the two lie one after the other)
            b = want[0]["bin"][int(offs[i]) : int(offs[i + 1])]
            v = b >= 0
            widest = max(widest, int(np.abs(np.diff(b))[v[1:] & v[:-1]].max()))
        most.append(widest)
    assert most == [4, 5]
    rng = np.random.default_rng(2)
    refs = [MC.ref_for(rng, _host_records([c], sets[1])[0]) for c in segs]
    pairs = [(s, p) for p in range(2) for s in range(2)]
    want = _want_scores(segs, sets, refs, pairs)
    assert _tuples(ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, np.concatenate(refs))) == want
    assert want[0] != want[2]


def test_the_reference_of_the_job_meets_its_conditions(job):
    """On the job's own segments: jumps of every size 0 ... max_jump in the checker's paths, and every set has a segment with
    at least 10 % voiced and at least 10 % unvoiced frames."""
    for k, (prm, (pts, _)) in enumerate(zip(MC.SETS, job["want"])):
        p = MC.params(**prm)
        jumps, mixed = set(), False
        for i in range(len(SEGMENT_ROWS)):
            b = pts["bin"][int(job["offs"][i]) : int(job["offs"][i + 1])]
            v = b >= 0
            jumps |= set(np.abs(np.diff(b))[v[1:] & v[:-1]].tolist())
            mixed = mixed or (len(b) >= 100 and 0.1 <= v.mean() <= 0.9)
        assert jumps == set(range(min(p["max_jump"], p["max_bin"] - p["min_bin"]) + 1)) and mixed, (k, sorted(jumps), mixed)


def test_a_segment_with_a_cell_out_of_range_is_unvoiced_and_its_neighbours_keep_theirs(model, job):
    from basic_pitch_amd import _native, melody as ME

    segs = [c.copy() for c in job["segs"]]
    segs[7] = MC.with_cell(segs[7], np.nan, TILE - 1, 263)   # outside the band, the last cell of the segment
    segs[9] = MC.with_cell(segs[9], -65537.0, 0, 0)          # the first cell of the segment
    segs[4] = MC.with_cell(segs[4], 65536.0, 3, 5)           # the largest magnitude that is taken
    offs, cat = MC.stack(segs)
    prm = MC.params(min_bin=50, max_bin=200)
    got = ME.melody_from_maps(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, prm)
    want = _host_records(segs, prm)
    assert want[1].tolist() == [0] * 7 + [1, 0, 1, 0, 0, 0]
    _assert_equal(got, want, "status 1")
    for i in (7, 9):
        assert np.all(got[0]["bin"][int(offs[i]) : int(offs[i + 1])] == -1)
    for i in (6, 8, 10):
        assert np.any(got[0]["bin"][int(offs[i]) : int(offs[i + 1])] >= 0)


def test_nothing_to_do_the_refusals_and_one_record_short(model, job):
    from basic_pitch_amd import _native, melody as ME

    lib = ME.bind(model._lib)
    h, offs, cat = model._handle, job["offs"], job["cat"]
    total = int(offs[-1])
    p = ME.melody_params()
    st = np.full(len(offs), -1, np.int32)
    buf = np.zeros(total + 4, MC.POINT)
    buf.view(np.uint8)[:] = 0xA5
    zero = np.zeros(4, np.int64)
    # zero segments, and segments without rows: BP_OK, statuses 0
    assert lib.bp_melody_from_maps(h, 0, _p64(zero), None, 0, C.addressof(p), None, 0, None) == 0
    assert lib.bp_melody_from_maps(h, 3, _p64(zero), None, 0, C.addressof(p), None, 0, st.ctypes.data) == 0 and st[:4].tolist() == [0, 0, 0, -1]

    def refused(said, n=len(offs) - 1, o=offs, c=cat.ctypes.data, kind=0, prm=p, pts=buf.ctypes.data, room=total, s=st):
        rc = lib.bp_melody_from_maps(h, n, _p64(o) if o is not None else None, c, kind, C.addressof(prm) if prm is not None else None,
                                     pts, room, s.ctypes.data if s is not None else None)
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and said in msg and "bp_melody_from_maps" in msg, (said, rc, msg)
        assert np.all(buf.view(np.uint8) == 0xA5), "a refused call wrote to points"

    refused(f"room for {total - 1} records, but the segments have {total} rows", room=total - 1)  # one short of the total
    refused("negative n_segments", n=-1)
    refused("null status", s=None)
    refused("room without a buffer", pts=None)
    refused("negative max_points", room=-1)
    refused("row_offsets must start at 0", o=np.array([1, 2] + [3] * 12, np.int64))
    refused("row_offsets must start at 0", o=np.array([0, 5, 4] + [6] * 11, np.int64))
    refused("mem_kind", kind=7)
    refused("null input pointer", c=None)
    refused("null params", prm=None)
    for fields, named in ((dict(threshold=np.nan), "threshold"), (dict(jump_penalty=-1.0), "jump_penalty"), (dict(voicing_penalty=np.inf), "voicing_penalty"),
                          (dict(max_jump=17), "max_jump"), (dict(min_bin=-1), "min_bin"), (dict(max_bin=264), "max_bin"),
                          (dict(min_bin=9, max_bin=8), "min_bin"), (dict(reserved=2), "reserved")):
        refused("params: ", prm=ME.melody_params(**fields))
        refused(named, prm=ME.melody_params(**fields))
    refused("BP_SWEEP_MAX_ROWS", n=1, o=np.array([0, 8388608 + 1], np.int64), room=8388608 + 1)
    # the handle is usable, and exactly the room of the rows is enough: the canary behind the records stands
    rc = lib.bp_melody_from_maps(h, len(offs) - 1, _p64(offs), cat.ctypes.data, 0, C.addressof(p), buf.ctypes.data, total, st.ctypes.data)
    assert rc == 0 and buf[:total].tobytes() == job["want"][0][0].tobytes() and np.all(buf[total:].view(np.uint8) == 0xA5)
    assert st[: len(offs) - 1].tolist() == [0] * (len(offs) - 1)


# ---- clips through the model
def _float_clips(model, sr):
    return [(c.astype(np.float32) / np.float32(32768.0)).reshape(-1, 1) for c in TS._clips_at(model, sr)]


def test_clips_through_the_model_give_the_records_of_their_own_contour_rows(model):
    """PCM clips of 100 samples, one window and two windows at two sample rates IN ONE CALL of Model.transcribe_clips_melody
    against the host checker on Model.predict_pcm(...)["contour"] of each clip alone."""
    from basic_pitch_amd import clips as CL, melody as ME

    clips = _float_clips(model, 22050) + _float_clips(model, 44100)
    rates = [22050] * 3 + [44100] * 3
    order = [0, 3, 1, 4, 2, 5]
    clips, rates = [clips[i] for i in order], [rates[i] for i in order]
    contours = [model.predict_pcm(c, r)["contour"] for c, r in zip(clips, rates)]
    assert [len(c) for c in contours][:2] == [0, 0] and all(len(c) > 0 for c in contours[2:])
    voiced = 0
    for prm in (None, dict(threshold=0.15, min_bin=30, max_bin=230, max_jump=2)):
        ests = model.transcribe_clips_melody(clips, rates, prm)
        want, status = _host_records(contours, prm)
        assert [e.status for e in ests] == status.tolist() == [0] * 6
        assert np.concatenate([e.bins for e in ests]).tobytes() == want["bin"].tobytes()
        assert np.concatenate([e.pitch_midi for e in ests]).tobytes() == want["pitch_midi"].tobytes()
        assert np.concatenate([e.salience for e in ests]).tobytes() == want["salience"].tobytes()
        voiced += int((want["bin"] >= 0).sum())
    assert voiced > 200
    # the native call of one rate, record for record
    arrays = [CL.as_clip(c, i) for i, c in enumerate(clips[1::2])]
    pts, st, offs = ME.infer_clips_melody(model, arrays, 44100)
    _assert_equal((pts, st), _host_records(contours[1::2], None), "bp_infer_clips_melody")
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in contours[1::2]])]).tolist()


# ---- sweeps scored where the track is
def _want_scores(segs, sets, refs, pairs, **tolerances):
    """bp_melody_rows + bp_score_melody_frames per decode: the six counts and the status."""
    from basic_pitch_amd import melody as ME

    out, cache = [], {}
    for s, p in pairs:
        if (s, p) not in cache:
            pts, st = ME.melody_rows(segs[s], MC.params(**sets[p]))
            if st:
                cache[(s, p)] = (len(segs[s]), 0, 0, 0, 0, 0, st)
            else:
                c = ME.score_melody_frames(pts, refs[s], **tolerances)
                cache[(s, p)] = tuple(int(c[f]) for f in FIELDS) + (0,)
        out.append(cache[(s, p)])
    return out


def _tuples(counts):
    return [tuple(int(c[f]) for f in FIELDS + ("status",)) for c in np.asarray(counts).reshape(-1)]


@pytest.fixture(scope="module")
def sweep_job(job):
    from basic_pitch_amd import sweep as SW

    rng = np.random.default_rng(21)
    pts, offs = job["want"][0][0], job["offs"]
    refs = [MC.ref_for(rng, pts[int(offs[i]) : int(offs[i + 1])]) for i in range(len(SEGMENT_ROWS))]
    pairs = SW.cross_product(len(MC.SETS), len(job["segs"]))
    return dict(refs=refs, flat=np.concatenate(refs), pairs=pairs, want=_want_scores(job["segs"], MC.SETS, refs, pairs))


def test_the_reference_of_the_sweep_is_not_trivial(sweep_job):
    want = sweep_job["want"]
    assert len(want) == 8 * len(SEGMENT_ROWS) and all(w[6] == 0 for w in want)
    for k in range(1, 6):
        assert max(w[k] for w in want) > 0, k
    assert any(w[5] > w[4] for w in want) and any(w[3] > w[5] for w in want) and any(w[2] > w[3] for w in want) and any(w[1] > w[3] for w in want)
    assert len({w[:6] for w in want}) >= 40


@pytest.mark.parametrize("where", ["host", "device"])
def test_the_cross_product_equals_from_maps_plus_the_counts_checker(model, job, sweep_job, where):
    from basic_pitch_amd import melody as ME

    ptr, kind, dev = _where(job, where)
    got = ME.melody_sweep_score(model, job["offs"], ptr, kind, MC.SETS, sweep_job["flat"])
    assert _tuples(got) == sweep_job["want"]
    # ... and the records those counts are of are bp_melody_from_maps' own
    for p in (0, 3):
        _assert_equal(ME.melody_from_maps(model, job["offs"], ptr, kind, MC.params(**MC.SETS[p])), job["want"][p], p)
    # another tolerance, strict
    tol = dict(pitch_tolerance_cents=50.0, strict=1)
    got = ME.melody_sweep_score(model, job["offs"], ptr, kind, MC.SETS[:3], sweep_job["flat"], **tol)
    want = _want_scores(job["segs"], MC.SETS, sweep_job["refs"], [q for q in sweep_job["pairs"] if q[1] < 3], **tol)
    assert _tuples(got) == want and want != sweep_job["want"][: len(want)]  # (refs sit exactly on the tolerance)


def test_an_explicit_table_with_repeated_pairs_equals_its_own_permutation(model, job, sweep_job):
    from basic_pitch_amd import _native, melody as ME

    rng = np.random.default_rng(5)
    pairs = sweep_job["pairs"]
    order = [int(k) for k in rng.permutation(len(pairs))[:40]] + [17, 17, 40, len(pairs) - 1, len(pairs) - 1]
    got = ME.melody_sweep_score(model, job["offs"], job["cat"].ctypes.data, _native.BP_MEM_HOST, MC.SETS, sweep_job["flat"],
                                [pairs[k] for k in order])
    assert _tuples(got) == [sweep_job["want"][k] for k in order]


def test_status_1_leaves_the_zero_record_and_its_neighbours_alone(model, job, sweep_job):
    from basic_pitch_amd import _native, melody as ME

    segs = [c.copy() for c in job["segs"]]
    segs[8] = MC.with_cell(segs[8], np.inf, 30, 0)
    offs, cat = MC.stack(segs)
    sets = MC.SETS[:2]
    n = len(segs)
    got = _tuples(ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, sweep_job["flat"]))
    for j, (s, p) in enumerate((s, p) for p in range(2) for s in range(n)):
        assert got[j] == ((TILE + 1, 0, 0, 0, 0, 0, 1) if s == 8 else sweep_job["want"][p * n + s]), (s, p)


def test_clips_through_the_model_are_scored_as_their_maps_are(model):
    from basic_pitch_amd import _native, clips as CL, melody as ME

    rng = np.random.default_rng(8)
    sets = [dict(), dict(threshold=0.15, max_jump=2), dict(threshold=0.5, voicing_penalty=0.25, min_bin=60, max_bin=230)]
    for sr in (22050, 44100):
        clips = _float_clips(model, sr)
        arrays = [CL.as_clip(c, i) for i, c in enumerate(clips)]
        contours = [model.predict_pcm(c, sr)["contour"] for c in clips]
        refs = [MC.ref_for(rng, _host_records([c], sets[1])[0]) for c in contours]
        pairs = [(s, p) for p in range(3) for s in range(3)]
        want = _want_scores(contours, sets, refs, pairs)
        assert sum(w[4] for w in want) > 0 and all(w[6] == 0 for w in want)
        assert _tuples(ME.infer_clips_melody_sweep_score(model, arrays, sr, sets, refs)) == want
        offs, cat = MC.stack(contours)
        assert _tuples(ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, sets, np.concatenate(refs))) == want
    mixed = _float_clips(model, 22050)[1:] + _float_clips(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    tracks = [np.zeros(len(model.predict_pcm(c, r)["contour"])) for c, r in zip(mixed, rates)]
    counts = model.transcribe_clips_sweep_melody_scores(mixed, rates, [dict()], tracks)
    assert counts.shape == (1, 4) and counts["n_frames"].tolist() == [[len(t) for t in tracks]] and np.all(counts["est_voiced"] > 0)
    assert np.all(counts["ref_voiced"] == 0)


def test_the_refusals_of_the_sweep_name_the_index_and_leave_the_handle_usable(model, job, sweep_job):
    from basic_pitch_amd import _native, melody as ME, score, sweep as SW

    lib = ME.bind(model._lib)
    h, offs, cat = model._handle, job["offs"], job["cat"]
    flat = sweep_job["flat"]
    prm = score.score_params()
    n_seg = len(offs) - 1
    scores, st = np.zeros((64, 6), np.int64), np.zeros(64, np.int32)

    def refused(said, sets=MC.SETS[:2], n_decodes=2 * n_seg, pairs=None, ref=flat, sp=prm, sc=scores):
        arr = ME.sets_array([ME.melody_params(**s) if isinstance(s, dict) else s for s in sets])
        tab = SW.decode_table(pairs) if pairs is not None else None
        rc = lib.bp_melody_sweep_score(h, n_seg, _p64(offs), cat.ctypes.data, _native.BP_MEM_HOST, len(sets), C.addressof(arr), n_decodes,
                                       C.addressof(tab) if tab is not None else None, ref.ctypes.data if ref is not None else None,
                                       C.addressof(sp), sc.ctypes.data if sc is not None else None, st.ctypes.data)
        msg = lib.bp_last_error(h).decode()
        assert rc == INV and said in msg and "bp_melody_sweep_score" in msg, (said, rc, msg)

    refused("set 1: max_bin", sets=[dict(), dict(max_bin=264)])
    refused("set 0: the threshold", sets=[dict(threshold=np.inf), dict()])
    refused("set 1: max_jump", sets=[dict(), dict(max_jump=17)])
    refused("n_decodes is not n_sets * n_segments", n_decodes=2 * n_seg - 1)
    refused("decode 1: params 2", n_decodes=2, pairs=[(0, 0), (1, 2)])
    refused(f"decode 1: segment {n_seg}", n_decodes=2, pairs=[(0, 0), (n_seg, 1)])
    refused("BP_SWEEP_MAX_DECODES", n_decodes=65537)
    refused("null sets, scores or status", sc=None)
    refused("null ref_pitch", ref=None)
    for value in (np.nan, -1.0, np.inf):
        bad = flat.copy()
        bad[137] = value
        refused("ref_pitch 137:", ref=bad)
    refused("tolerance", sp=score.score_params(pitch_tolerance_cents=-1.0))
    got = ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, MC.SETS[:2], flat)
    assert _tuples(got) == sweep_job["want"][: 2 * n_seg]
    # nothing to do is no error: no decodes; decodes of segments without rows alone
    assert len(ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, MC.SETS[:2], flat, [])) == 0
    empty = ME.melody_sweep_score(model, offs, cat.ctypes.data, _native.BP_MEM_HOST, MC.SETS[:2], flat, [(0, 0), (0, 1)])
    assert _tuples(empty) == [(0, 0, 0, 0, 0, 0, 0)] * 2


# ---- the Python entries
def test_the_model_entries_take_host_and_device_outputs(model, job, sweep_job):
    import torch

    from basic_pitch_amd import melody as ME
    from basic_pitch_amd.note_creation import model_frames_to_time

    outputs = [{"contour": c} for c in job["segs"]]
    on_device = [{"contour": torch.from_numpy(c).cuda()} for c in job["segs"]]
    want_pts, _ = job["want"][0]
    offs = job["offs"]
    n = len(SEGMENT_ROWS)
    for outs in (outputs, on_device):
        ests = model.melody(outs)
        assert len(ests) == n
        for i, est in enumerate(ests):
            w = want_pts[int(offs[i]) : int(offs[i + 1])]
            assert est.status == 0 and est.bins.tobytes() == w["bin"].tobytes()
            assert est.pitch_midi.tobytes() == w["pitch_midi"].tobytes() and est.salience.tobytes() == w["salience"].tobytes()
            assert np.array_equal(est.times_s, model_frames_to_time(len(w))) and np.array_equal(est.voiced, w["bin"] >= 0)
        counts = model.sweep_melody_scores(outs, MC.SETS, sweep_job["refs"])
        assert counts.shape == (8, n) and _tuples(counts) == sweep_job["want"]
        pairs = [(12, 7), (3, 0), (12, 7)]
        some = model.sweep_melody_scores(outs, MC.SETS, sweep_job["refs"], pairs)
        assert _tuples(some) == [sweep_job["want"][p * n + s] for s, p in pairs]
    assert model.melody([]) == []
    m = ME.measures(counts)
    assert m["overall_accuracy"].shape == (8, n) and np.all((m["overall_accuracy"] >= 0) & (m["overall_accuracy"] <= 1))
    assert np.all(m["raw_chroma_accuracy"] >= m["raw_pitch_accuracy"]) and np.any(m["raw_chroma_accuracy"] > m["raw_pitch_accuracy"])
    narrow = model.melody(outputs, MC.params(**MC.SETS[4]))
    assert np.concatenate([e.bins for e in narrow]).tobytes() == job["want"][4][0]["bin"].tobytes()
    with pytest.raises(ValueError, match="reference track"):
        model.sweep_melody_scores(outputs, MC.SETS, [r[:-1] if len(r) else r for r in sweep_job["refs"]])


def test_a_440_hz_sine_is_voiced_at_the_bin_of_midi_69(model):
    """A pure 440 Hz sine (amplitude 0.5, one window) through Model.predict + Model.melody: the frames of its steady part
    (20 ... 149) are voiced with bin 144 +- 1 (MIDI 69 is bin 144) — the gate of tests/test_gpu_multipitch.py, for the reason
    DESIGN.md 20 gives: the CPU oracle itself puts the peak a third of a semitone above MIDI 69, so there is no margin in
    semitones."""
    from basic_pitch_amd.constants import AUDIO_N_SAMPLES

    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(AUDIO_N_SAMPLES) / 22050.0)).astype(np.float32)[None, :]
    out = model.predict(x)
    est = model.melody([{"contour": np.asarray(out["contour"]).reshape(-1, 264)}])[0]
    assert est.status == 0
    for fr in range(20, 150):
        assert est.voiced[fr] and abs(int(est.bins[fr]) - 144) <= 1, (fr, int(est.bins[fr]))
