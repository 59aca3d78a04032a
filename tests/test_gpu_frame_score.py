"""The decodes of a sweep scored at the note and the frame level on the device (bp_note_events_sweep_frame_score /
bp_infer_clips_events_sweep_frame_score, include/basic_pitch_amd_frame_score.h; csrc/note_frames.hip): decode by decode the
five frame counts, the four note counts and the status are those of the host checkers bp_score_note_frames and
bp_score_note_events on the events the plain sweep call returns for that decode, with the refs and the rows of its segment —
for the cross product and an explicit table, with and without the note counts, host and device maps, segments that end on
and behind the steps of the frame time and that take more than one chunk of the kernel, chains only a maximum matching
completes, every status, PCM clips on every kind of handle, and with the other calls on the same handle undisturbed."""
import ctypes as C

import numpy as np
import pytest

import frame_score_cases as FC
import note_cases
import score_cases as SC
import test_gpu_score as TG
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

MAPS = TS.MAPS
NOTE_FIELDS = TG.FIELDS
CHUNK = 2048  # csrc/bp_kernels.h kNoteFramesChunk
ROWS = (0, 1, 5, 142, 172, 173, 345, 433, 1300, CHUNK + 1)


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _frame_tuples(counts):
    return [tuple(int(c[f]) for f in FC.FIELDS + ("status",)) for c in np.asarray(counts).reshape(-1)]


def _want_frames(got, pairs, refs, rows, **tolerances):
    """The frame checker on every decode of a plain sweep's result (events, bends, event_offsets, status): the six integers."""
    from basic_pitch_amd import frame_score

    events, _, ev_offs, status = got
    out = []
    for j, (s, _) in enumerate(pairs):
        if status[j]:
            out.append((int(rows[s]), 0, 0, 0, 0, int(status[j])))
            continue
        c = frame_score.score_note_frames(TG._rows(events, int(ev_offs[j]), int(ev_offs[j + 1])), refs[s], int(rows[s]), **tolerances)
        out.append(tuple(int(c[f]) for f in FC.FIELDS) + (0,))
    return out


def _refs_for(rng, own, rows):
    """test_gpu_score's perturbed refs, then a quarter moved by +0.5 or -0.3 in pitch, one outside 21 ... 108, one of no length."""
    refs = TG._perturbed(rng, own)
    pick = rng.random(len(refs)) < 0.25
    refs[pick, 2] += rng.choice([0.5, -0.3], int(pick.sum()))
    t = SC.frame_time(max(1, rows // 2))
    return np.concatenate([refs, [(0.0, SC.frame_time(rows + 3), 110.0 if rng.random() < 0.5 else 12.5), (t, t, 60.0)]])


def _call(model, job, pairs=None, notes=True, **tolerances):
    from basic_pitch_amd import _native, frame_score

    return frame_score.note_events_sweep_frame_score(model, job["offs"], *TG._ptrs(job["cat"], job["offs"]), _native.BP_MEM_HOST,
                                                     job["sets"], job["refs"], pairs, notes, **tolerances)


@pytest.fixture(scope="module")
def job(model):
    """The golden maps cut into one-window segments and tests/test_gpu_sweep.py's handcrafted segments at ROWS, that file's
    twelve sets, refs made from each segment's own events under set 0, and the plain sweep of the cross product with both
    checkers' counts for it — computed once."""
    from basic_pitch_amd import _native, sweep as SW

    gold = note_cases.golden_output()
    T = gold["note"].shape[0]
    segs = [{k: gold[k][t : t + 142].copy() for k, _ in MAPS} for t in range(0, T, 142)]
    rng = np.random.default_rng(2024)
    segs += [TS._segment(rng, rows) for rows in ROWS]
    sets = [TS._prm(dict(TS.BASE, **v)) for v in TS.VARIED]
    cat, offs = TS._cat(segs)
    rows = np.diff(offs)
    plain = SW.note_events_sweep(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    pairs = SW.cross_product(len(sets), len(segs))
    events, _, ev_offs, status = plain
    rng = np.random.default_rng(7)
    refs = [_refs_for(rng, TG._rows(events, int(ev_offs[i]), int(ev_offs[i + 1])), int(rows[i])) for i in range(len(segs))]
    return dict(segs=segs, sets=sets, cat=cat, offs=offs, rows=rows, refs=refs, pairs=pairs, want_notes=TG._want(plain, pairs, refs),
                want=_want_frames(plain, pairs, refs, rows))


def test_the_reference_is_not_trivial(job):
    want, n_seg = job["want"], len(job["segs"])
    assert len(job["sets"]) == 12 and len(want) == 12 * n_seg and job["rows"].tolist()[-len(ROWS):] == list(ROWS)
    ok = [w for w in want if w[5] == 0]
    assert {w[5] for w in want} == {0, 1}  # the set with no onset threshold is the host's
    assert len({w[:5] for w in ok}) >= 20
    assert sum(w[4] > 0 for w in ok) >= 10                    # substitutions
    assert sum(w[3] < min(w[1], w[2]) for w in ok) >= 10      # partial matchings
    assert sum(w[3] > 0 for w in ok) >= 50
    assert any(w[2] == 0 for w in ok) and any(w[1] == 0 for w in ok)
    assert any(w[0] == CHUNK + 1 and w[3] > 0 for w in ok) and any(w[0] == 1300 and w[3] > 0 for w in ok)


def test_the_cross_product_equals_sweep_plus_both_checkers(model, job):
    notes, frames = _call(model, job)
    assert _frame_tuples(frames) == job["want"]
    assert TG._tuples(notes) == job["want_notes"]
    assert notes["status"].tolist() == frames["status"].tolist()


def test_an_explicit_table_with_repeated_pairs_equals_its_own_permutation(model, job):
    rng = np.random.default_rng(5)
    pairs = job["pairs"]
    order = list(rng.permutation(len(pairs))[:70]) + [17, 17, 40, len(pairs) - 1, len(pairs) - 1]
    notes, frames = _call(model, job, [pairs[k] for k in order])
    assert _frame_tuples(frames) == [job["want"][k] for k in order]
    assert TG._tuples(notes) == [job["want_notes"][k] for k in order]


def test_without_scores_the_frames_and_the_statuses_are_the_same(model, job):
    notes, frames = _call(model, job, notes=False)
    assert notes is None and _frame_tuples(frames) == job["want"]
    # ... and through the C ABI itself: scores NULL, the same bytes in frames and status as with scores
    from basic_pitch_amd import _native, frame_score, score, sweep as SW

    lib = frame_score.bind(model._lib)
    offs, n = job["offs"], len(job["pairs"])
    sets = SW.sets_array(job["sets"])
    ref_offs, flat = score.refs_table(job["refs"])
    prm = score.score_params()
    out = []
    for with_scores in (True, False):
        sc, fr, st = np.full((n, 4), -1, np.int32), np.full((n, 5), -1, np.int64), np.full(n, -1, np.int32)
        rc = lib.bp_note_events_sweep_frame_score(model._handle, len(offs) - 1, offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  *TG._ptrs(job["cat"], offs), _native.BP_MEM_HOST, len(job["sets"]), C.addressof(sets), n,
                                                  None, ref_offs.ctypes.data_as(C.POINTER(C.c_int64)), flat.ctypes.data, C.addressof(prm),
                                                  sc.ctypes.data if with_scores else None, fr.ctypes.data, st.ctypes.data)
        assert rc == _native.BP_OK, lib.bp_last_error(model._handle)
        out.append((fr.tobytes(), st.tobytes()))
        assert (sc == -1).all() != with_scores
    assert out[0] == out[1]


def test_maps_in_device_memory_and_the_python_entry(model, job):
    import torch

    from basic_pitch_amd import frame_score, score

    n_seg = len(job["segs"])
    dev = [{k: torch.from_numpy(s[k]).cuda() for k, _ in MAPS} for s in job["segs"]]
    before = [{k: d[k].clone() for k in d} for d in dev]
    notes, frames = model.sweep_frame_scores(dev, job["sets"], job["refs"])
    torch.cuda.synchronize()
    for d, b in zip(dev, before):
        for k in d:
            assert torch.equal(d[k].view(torch.int32), b[k].view(torch.int32)), k
    assert notes.shape == frames.shape == (12, n_seg) and notes.dtype == score.COUNTS and frames.dtype == frame_score.FRAME_COUNTS
    flat, flat_notes = _frame_tuples(frames), TG._tuples(notes)
    for j, (w, g) in enumerate(zip(job["want"], flat)):
        if w[5] == 0:
            assert g == w and flat_notes[j] == job["want_notes"][j], j
        else:  # the decodes the device leaves are scored by the host route; the status stays
            assert g[5] == w[5] == 1 and g[0] == w[0], j
    # ... and that host route is the host decoder followed by both checkers
    p = next(i for i, v in enumerate(TS.VARIED) if v.get("onset_thresh") == 0.0)
    n_host = 0
    for i, seg in enumerate(job["segs"][:6]):  # (the golden segments: all have rows)
        ev = score._host_events_from_maps(seg, job["sets"][p])
        c = frame_score.score_note_frames(ev, job["refs"][i], seg["note"].shape[0])
        assert flat[p * n_seg + i] == tuple(int(c[f]) for f in FC.FIELDS) + (1,), i
        s = score.score_note_events(ev, job["refs"][i])
        assert flat_notes[p * n_seg + i] == tuple(int(s[f]) for f in NOTE_FIELDS[:4]) + (1,), i
        n_host += int(c["true_pos"])
    assert n_host >= 100
    # pairs: one record per pair; host maps give the same; notes=False gives the frames alone
    some = [(8, 2), (3, 0), (8, 2), (0, 1), (n_seg - 1, 4)]
    listed = model.sweep_frame_scores(job["segs"], job["sets"], job["refs"], pairs=some)
    assert _frame_tuples(listed[1]) == [flat[p * n_seg + i] for i, p in some]
    assert TG._tuples(listed[0]) == [flat_notes[p * n_seg + i] for i, p in some]
    alone = model.sweep_frame_scores(job["segs"], job["sets"], job["refs"], pairs=some, notes=False)
    assert isinstance(alone, np.ndarray) and _frame_tuples(alone) == _frame_tuples(listed[1])
    # the planted set wins by accuracy when the refs are its own events
    # (the golden segments and the handcrafted one-window segment, whose notes of 5 and 8 frames a minimum length of 7 tells apart)
    planted = 5
    segs = job["segs"][:6] + [job["segs"][9]]
    assert TS.VARIED[planted] == {"min_note_len": 7} and segs[6]["note"].shape[0] == 142
    events = model.sweep_note_events(segs, job["sets"], pairs=[(i, planted) for i in range(7)])
    own = [SC.notes([(e[0], e[1], e[2]) for e in ev]) for ev, _ in events]
    got = model.sweep_frame_scores(segs, job["sets"], own, notes=False)
    assert got.shape == (12, 7) and frame_score.best_set_by_accuracy(got) == planted
    total = {f: got[f].sum(axis=1) for f in FC.FIELDS}
    assert total["true_pos"][planted] == total["ref_frames"][planted] == total["est_frames"][planted] >= 200


def test_other_tolerances_and_strict_reach_the_kernel(model, job):
    from basic_pitch_amd import _native, frame_score, sweep as SW

    segs, refs = job["segs"][:5], job["refs"][:5]
    cat, offs = TS._cat(segs)
    sets = job["sets"][:2]
    plain = SW.note_events_sweep(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    pairs = SW.cross_product(2, 5)
    seen = set()
    for tol in (dict(strict=1), dict(pitch_tolerance_cents=0.0), dict(pitch_tolerance_cents=30.0, strict=1),
                dict(pitch_tolerance_cents=130.0), dict(pitch_tolerance_cents=1e6)):
        _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, refs, **tol)
        assert _frame_tuples(frames) == _want_frames(plain, pairs, refs, np.diff(offs), **tol), tol
        seen.add(tuple(_frame_tuples(frames)))
    assert len(seen) >= 4  # the tolerances change the counts


# ---- chains: only a maximum matching completes them
STEP = TG.STEP  # bins between simultaneous notes


def _notes_map(pitches, T=40, first=5, last=25):
    m = {"note": np.zeros((T, 88), np.float32), "onset": np.zeros((T, 88), np.float32), "contour": np.zeros((T, 264), np.float32)}
    for p in pitches:
        m["note"][first:last, p - 21] = 0.8
        m["onset"][first, p - 21] = 0.9
    return m


def test_the_minimal_chain_in_all_four_orders_through_pairs(model):
    """Ests 60 and 62, refs 61 (hits both at exactly 100 cents) and 60.8 (hits 60 alone): two segments with the notes, each
    with the refs in one order, and the pairs in both orders."""
    from basic_pitch_amd import _native, frame_score, sweep as SW

    seg = _notes_map([60, 62])
    sets = [TS._prm(dict(TS.BASE, melodia_trick=False))]
    cat, offs = TS._cat([seg, seg])
    events, _, ev_offs, status = SW.note_events_sweep(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    est = TG._rows(events, 0, int(ev_offs[1]))
    assert status.tolist() == [0, 0] and sorted(est[:, 2].tolist()) == [60, 62] and est[0, 0] == SC.frame_time(5) and est[0, 1] == SC.frame_time(25)
    a, b = (est[0, 0], est[0, 1], 61.0), (est[0, 0], est[0, 1], 60.8)
    refs = [SC.notes([a, b]), SC.notes([b, a])]
    tol = dict(pitch_tolerance_cents=100.0)
    stranded = 0
    for r in refs:
        counts, g = FC.per_frame(est, r, 40, **tol)[10]
        assert counts[:3] == (2, 2, 2)
        stranded += SC.first_fit(g.T) < 2
    assert stranded >= 1
    for pairs in ([(0, 0), (1, 0)], [(1, 0), (0, 0)]):
        _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, refs, pairs, **tol)
        assert _frame_tuples(frames) == [(40, 40, 40, 40, 0, 0)] * 2
    # strict: 61 hits neither, a substitution per frame; the default 50 cents: nothing hits
    _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, refs, strict=1, **tol)
    assert _frame_tuples(frames) == [(40, 40, 40, 20, 20, 0)] * 2
    _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, refs)
    assert _frame_tuples(frames) == [(40, 40, 40, 0, 40, 0)] * 2


@pytest.mark.parametrize("decoy_low", (True, False))
def test_the_device_matches_a_chain_of_eight_on_every_frame(model, decoy_low):
    from basic_pitch_amd import _native, frame_score, sweep as SW

    seg = TG._eight_notes()
    sets = [TS._prm(dict(TS.BASE, melodia_trick=False))]
    cat, offs = TS._cat([seg])
    events, _, ev_offs, status = SW.note_events_sweep(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    est = TG._rows(events, 0, int(ev_offs[1]))
    assert status[0] == 0 and est[:, 2].tolist() == [64, 62, 60, 58, 56, 54, 52, 50]
    _, ref = SC.long_chain(50.0, decoy_low, start=est[0, 0], end=est[0, 1])
    ref[:, 2] = 50.0 + STEP * (ref[:, 2] - 50.0)
    tol = dict(pitch_tolerance_cents=50.0 * STEP)
    counts, g = FC.per_frame(est, ref, 40, **tol)[10]
    assert counts[:3] == (8, 8, 8) and min(SC.first_fit(g.T), SC.first_fit(g[:, ::-1].T)) == 7
    _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, [ref], **tol)
    assert _frame_tuples(frames) == [(40, 160, 160, 160, 0, 0)] == _want_frames((events, None, ev_offs, status), [(0, 0)], [ref], [40], **tol)
    _, frames = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, [ref])
    assert _frame_tuples(frames) == [(40, 160, 160, 0, 160, 0)]


# ---- statuses
def test_statuses_1_2_and_3_leave_the_zero_records_and_are_redone_on_the_host_alone(model, job):
    from basic_pitch_amd import _native, frame_score, score

    clean, refs = job["segs"][:3], job["refs"][:3]
    nan = {k: v.copy() for k, v in job["segs"][1].items()}
    nan["note"][50, 40] = np.nan
    # tests/test_gpu_score.py: under a frame threshold of 0 the bends the set asks for pass the room of the decode's region
    dense = {"note": np.ones((64, 88), np.float32), "onset": np.zeros((64, 88), np.float32), "contour": np.zeros((64, 264), np.float32)}
    dense["onset"][1:62:2, ::2] = 0.9
    many = np.tile(np.array([[0.5, 1.0, 60.0]]), (score.MAX_NOTES + 1, 1))
    overflow = TS._prm(dict(onset_thresh=0.5, frame_thresh=0.0, min_note_len=0, infer_onsets=False, melodia_trick=False))
    sets = [job["sets"][0], overflow]

    def call(segs, seg_refs, notes=True):
        cat, offs = TS._cat(segs)
        n, f = frame_score.note_events_sweep_frame_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, seg_refs, None, notes)
        return (TG._tuples(n) if notes else None), _frame_tuples(f)

    alone_n, alone = call(clean, refs)
    assert [a[5] for a in alone] == [0] * 6 and sum(a[3] for a in alone) >= 100
    #         0..2   3    4      5
    segs, seg_refs = clean + [nan, dense, job["segs"][1]], refs + [refs[1], refs[0], many]
    n = len(segs)
    for notes in (True, False):
        both_n, both = call(segs, seg_refs, notes)
        for p in range(2):
            assert both[p * n : p * n + 3] == alone[p * 3 : p * 3 + 3], p                # unchanged
            assert both[p * n + 3] == (142, 0, 0, 0, 0, 1)                               # a NaN
            assert both[p * n + 5] == (142, 0, 0, 0, 0, 3)                               # too many refs
            if notes:
                assert both_n[p * n : p * n + 3] == alone_n[p * 3 : p * 3 + 3]
                assert both_n[p * n + 3] == (len(refs[1]), 0, 0, 0, 1) and both_n[p * n + 5] == (score.MAX_NOTES + 1, 0, 0, 0, 3)
        assert both[4][5] == 0 and both[4][2] > 0 and both[n + 4] == (64, 0, 0, 0, 0, 2)  # the dense segment under frame threshold 0
        if notes:
            assert both_n[n + 4] == (len(refs[0]), 0, 0, 0, 2)
    # exactly the bound is scored
    _, at_bound = call([job["segs"][1]], [many[:-1]])
    c = frame_score.score_note_frames(score._host_events_from_maps(job["segs"][1], sets[0]), many[:-1], 142)
    assert at_bound[0] == tuple(int(c[f]) for f in FC.FIELDS) + (0,) and at_bound[0][1] > score.MAX_NOTES and at_bound[0][2] > 0
    # the Python entry redoes the decodes the device left, and those alone, by the host decoder and both checkers
    todo = [(3, 0), (4, 1), (5, 0), (1, 0)]
    got_n, got = model.sweep_frame_scores(segs, sets, seg_refs, pairs=todo)
    assert got["status"].tolist() == [1, 2, 3, 0] == got_n["status"].tolist()
    assert _frame_tuples(got)[3] == alone[1] and TG._tuples(got_n)[3] == alone_n[1]
    for k, (s, p) in enumerate(todo[:3]):
        ev = score._host_events_from_maps(segs[s], sets[p])
        c = frame_score.score_note_frames(ev, seg_refs[s], segs[s]["note"].shape[0])
        assert _frame_tuples(got)[k][:5] == tuple(int(c[f]) for f in FC.FIELDS), k
        c = score.score_note_events(ev, seg_refs[s])
        assert TG._tuples(got_n)[k][:4] == tuple(int(c[f]) for f in NOTE_FIELDS[:4]), k
    assert got["est_frames"][1] > 0 and got["ref_frames"][2] > score.MAX_NOTES


# ---- PCM clips, on every kind of handle
@pytest.fixture(scope="module")
def handles(model):
    from basic_pitch_amd.inference import Model

    made = {"default": model}

    def get(mode):
        if mode not in made:
            made[mode] = Model(device=0, max_windows=8, **{mode: True})
        return made[mode]

    yield get
    for mode, m in made.items():
        if mode != "default":
            m.close()


@pytest.mark.parametrize("mode", TS.HANDLES)
def test_clips_through_the_model_equal_the_clips_sweep_plus_both_checkers(handles, mode):
    from basic_pitch_amd import clips as CL, frame_score, sweep as SW

    m = handles(mode)
    sets = [TS._prm(v) for v in TS.CLIP_SETS]
    matched = 0
    for sr in (22050, 44100) if mode == "default" else (44100,):
        arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(m, sr))]
        rows = np.diff(CL.clips_row_offsets(m, arrays, sr))
        plain = SW.infer_clips_events_sweep(m, arrays, sr, sets)
        events, _, ev_offs, status = plain
        rng = np.random.default_rng(11)
        refs = [_refs_for(rng, TG._rows(events, int(ev_offs[i]), int(ev_offs[i + 1])), int(rows[i])) for i in range(3)]
        pairs = SW.cross_product(3, 3)
        want, want_notes = _want_frames(plain, pairs, refs, rows), TG._want(plain, pairs, refs)
        notes, frames = frame_score.infer_clips_events_sweep_frame_score(m, arrays, sr, sets, refs)
        assert _frame_tuples(frames) == want and TG._tuples(notes) == want_notes, (mode, sr)
        table = [(2, 1), (1, 0), (2, 1)]
        none, frames = frame_score.infer_clips_events_sweep_frame_score(m, arrays, sr, sets, refs, table, notes=False)
        assert none is None and _frame_tuples(frames) == [want[p * 3 + i] for i, p in table]
        matched += sum(w[3] for w in want)
    assert matched >= 10


def test_transcribe_clips_sweep_frame_scores_groups_the_rates_and_finishes_on_the_host(model):
    from basic_pitch_amd import clips as CL, frame_score, note_creation as NC, score

    clips = TS._clips_at(model, 22050)[1:] + TS._clips_at(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    rows = [int(np.diff(CL.clips_row_offsets(model, [CL.as_clip(c, 0)], r))[0]) for c, r in zip(clips, rates)]
    sets = [NC._note_params(ot, 0.3, 11, True, None, None, True, NC.ENERGY_TOLERANCE, True) for ot in (0.5, 0.0, 0.6)]
    events = model.transcribe_clips_sweep(clips, rates, sets)  # [set][clip], complete: set 1 by the host route
    refs = [SC.notes([(e[0], e[1], e[2]) for e in events[2][i]]) for i in range(4)]  # set 2 is the planted one
    notes, frames = model.transcribe_clips_sweep_frame_scores(clips, rates, sets, refs)
    assert frames.shape == notes.shape == (3, 4) and frames["status"].tolist() == [[0] * 4, [1] * 4, [0] * 4] == notes["status"].tolist()
    for p in range(3):
        for i in range(4):
            c = frame_score.score_note_frames(events[p][i], refs[i], rows[i])
            assert tuple(int(frames[p, i][f]) for f in FC.FIELDS) == tuple(int(c[f]) for f in FC.FIELDS), (p, i)
            c = score.score_note_events(events[p][i], refs[i])
            assert tuple(int(notes[p, i][f]) for f in NOTE_FIELDS[:4]) == tuple(int(c[f]) for f in NOTE_FIELDS[:4]), (p, i)
    assert frame_score.frame_metrics(frames)["accuracy"][2].tolist() == [1.0] * 4 and frames["true_pos"][2].sum() >= 40
    assert frame_score.best_set_by_accuracy(frames) == 2
    listed = model.transcribe_clips_sweep_frame_scores(clips, rates, sets, refs, pairs=[(3, 2), (0, 0), (2, 1)], notes=False)
    assert _frame_tuples(listed) == [_frame_tuples(frames[2, 3])[0], _frame_tuples(frames[0, 0])[0], _frame_tuples(frames[1, 2])[0]]


# ---- refusals
def test_refusals_name_the_index_and_leave_the_handle_usable(model, job):
    from basic_pitch_amd import _native, clips as CL, frame_score, score, sweep as SW

    INV = _native.BP_ERR_INVALID_ARG
    segs = job["segs"][:3]
    cat, offs = TS._cat(segs)
    lib = frame_score.bind(model._lib)
    h = model._handle
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    sets = SW.sets_array(job["sets"][:2])
    good_offs, good = score.refs_table(job["refs"][:3])
    assert len(good) >= 6 and good_offs[1] >= 2
    what = "bp_note_events_sweep_frame_score"

    def call(ref_offs=good_offs, refs=good, n_decodes=6, table=None, scores=True, frames=True, status=True, **tol):
        prm = score.score_params(**tol)
        sc, fr, st = np.zeros((max(1, n_decodes), 4), np.int32), np.zeros((max(1, n_decodes), 5), np.int64), np.zeros(max(1, n_decodes), np.int32)
        rc = lib.bp_note_events_sweep_frame_score(h, 3, p64(offs), *TG._ptrs(cat, offs), _native.BP_MEM_HOST, 2, C.addressof(sets), n_decodes,
                                                  C.addressof(table) if table is not None else None,
                                                  p64(ref_offs) if ref_offs is not None else None, refs.ctypes.data if refs is not None else None,
                                                  C.addressof(prm), sc.ctypes.data if scores else None, fr.ctypes.data if frames else None,
                                                  st.ctypes.data if status else None)
        return rc, lib.bp_last_error(h).decode(), fr, st

    def refused(want, **kw):
        rc, msg, _, _ = call(**kw)
        assert rc == INV and what in msg and all(w in msg for w in want), msg
        rc, msg, _, _ = call()  # the handle takes the next call
        assert rc == _native.BP_OK, msg

    def with_ref(i, field, value):
        r = good.copy()
        r[i, field] = value
        return r

    k = len(good) - 1
    refused((f"ref {k}:", "not finite"), refs=with_ref(k, 0, np.nan))
    refused(("ref 1:", "not finite"), refs=with_ref(1, 1, np.inf))
    refused(("ref 2:", "end_s < start_s"), refs=with_ref(2, 1, good[2, 0] - 1e-9))
    down = good_offs.copy()
    down[2] = down[1] - 1
    refused(("segment 1:", "ref_offsets decrease"), ref_offs=down)
    up = good_offs.copy()
    up[0] = 1
    refused(("ref_offsets must start at 0",), ref_offs=up)
    for field in ("onset_tolerance_s", "offset_ratio", "offset_min_tolerance_s", "pitch_tolerance_cents"):
        refused(("score_params", "negative or not finite"), **{field: -0.01})
    refused(("score_params", "reserved"), reserved=1)
    refused(("null ref_offsets or frames",), ref_offs=None)
    refused(("null ref_offsets or frames",), frames=False)
    refused(("status",), status=False)
    refused(("null refs",), refs=None)
    assert call(scores=False)[0] == _native.BP_OK  # a null scores is no refusal here
    refused(("decode 1:", "segment 3"), table=SW.decode_table([(0, 0), (3, 1)]), n_decodes=2)
    refused(("n_sets * n_segments",), n_decodes=5)
    # the clips call checks the same arguments
    arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(model, 22050))]
    sc, fr, st = np.zeros((6, 4), np.int32), np.zeros((6, 5), np.int64), np.zeros(6, np.int32)
    prm = score.score_params()
    bad = with_ref(1, 0, np.nan)
    rc = lib.bp_infer_clips_events_sweep_frame_score(h, 3, CL.clip_table(arrays), 22050, _native.BP_MEM_HOST, 2, C.addressof(sets), 6, None,
                                                     p64(good_offs), bad.ctypes.data, C.addressof(prm), sc.ctypes.data, fr.ctypes.data, st.ctypes.data)
    msg = lib.bp_last_error(h).decode()
    assert rc == INV and "bp_infer_clips_events_sweep_frame_score" in msg and "ref 1:" in msg, msg
    rc = lib.bp_infer_clips_events_sweep_frame_score(h, 3, CL.clip_table(arrays), 22050, _native.BP_MEM_HOST, 2, C.addressof(sets), 6, None,
                                                     p64(good_offs), good.ctypes.data, C.addressof(prm), None, None, st.ctypes.data)
    assert rc == INV and "null ref_offsets or frames" in lib.bp_last_error(h).decode()
    # nothing to do is no error: no decodes; no rows at all (every decode {0, 0, 0, 0, 0}, status 0); no onset threshold anywhere
    rc, msg, _, _ = call(n_decodes=0, table=SW.decode_table([]))
    assert rc == _native.BP_OK, msg
    none = np.zeros(4, np.int64)
    fr[:] = -1
    rc = lib.bp_note_events_sweep_frame_score(h, 3, p64(none), None, None, None, _native.BP_MEM_HOST, 2, C.addressof(sets), 6, None,
                                              p64(good_offs), good.ctypes.data, C.addressof(prm), sc.ctypes.data, fr.ctypes.data, st.ctypes.data)
    assert rc == _native.BP_OK and st.tolist() == [0] * 6 and not fr.any()
    assert sc.tolist() == [[int(good_offs[i + 1] - good_offs[i]), 0, 0, 0] for i in range(3)] * 2
    off = SW.sets_array([TS._prm(dict(TS.BASE, onset_thresh=0.0))] * 2)
    rc = lib.bp_note_events_sweep_frame_score(h, 3, p64(offs), *TG._ptrs(cat, offs), _native.BP_MEM_HOST, 2, C.addressof(off), 6, None,
                                              p64(good_offs), good.ctypes.data, C.addressof(prm), None, fr.ctypes.data, st.ctypes.data)
    assert rc == _native.BP_OK and st.tolist() == [1] * 6 and fr.tolist() == [[142, 0, 0, 0, 0]] * 6


# ---- the other calls on the same handle
def test_the_sweep_the_scoring_and_the_frame_call_in_turn_each_give_what_they_gave_alone(model, job):
    from basic_pitch_amd import _native, score, sweep as SW

    cat, offs, sets = job["cat"], job["offs"], job["sets"]

    def plain():
        events, bends, ev_offs, status = SW.note_events_sweep(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets)
        n = int(ev_offs[-1])
        return bytes(events)[: n * C.sizeof(_native.bp_note_event)], bends[: sum(e.n_bends for e in events[:n])].tobytes(), \
            ev_offs.tobytes(), status.tobytes()

    def scored():
        return score.note_events_sweep_score(model, offs, *TG._ptrs(cat, offs), _native.BP_MEM_HOST, sets, job["refs"]).tobytes()

    def framed(notes=True):
        n, f = _call(model, job, notes=notes)
        return (n.tobytes() if notes else None), f.tobytes()

    a, s, f = plain(), scored(), framed()
    g = framed(False)
    assert framed() == f and g == (None, f[1])        # twice in a row: identical bytes
    assert plain() == a and framed() == f and scored() == s and framed(False) == g and plain() == a and scored() == s
    assert f[0] == s                                   # the note counts are the scoring call's
    assert len(a[0]) >= 300 * 48 and len(a[1]) > 0
    one = TS._single(model, job["segs"][1], sets[0])
    framed()
    TS._same(TS._single(model, job["segs"][1], sets[0]), one, "bp_note_events_from_maps after a frame-score call")
