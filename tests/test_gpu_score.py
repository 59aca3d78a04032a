"""The decodes of a sweep scored on the device (bp_note_events_sweep_score / bp_infer_clips_events_sweep_score,
include/basic_pitch_amd_score.h; csrc/note_score.hip): decode by decode the four counts and the status are those of the host
checker bp_score_note_events on the events the plain sweep call returns for that decode, with the refs of its segment — for
an explicit table and the cross product, host and device maps, PCM clips on every kind of handle, chains only an augmenting
matcher completes, every status, and with the events calls on the same handle undisturbed."""
import ctypes as C

import numpy as np
import pytest

import note_cases
import score_cases as SC
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

MAPS = TS.MAPS
FIELDS = ("n_ref", "n_est", "matched_onset", "matched_offset", "status")


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def _rows(events, lo, hi):
    return SC.notes([(e.start_s, e.end_s, e.pitch_midi) for e in events[lo:hi]])


def _perturbed(rng, own):
    """Refs from a segment's own events: a third moved in onset by up to 80 ms and in end by up to 30 % of the length, some
    dropped, some added."""
    refs = own.copy()
    n = len(refs)
    pick = rng.random(n) < 1 / 3
    length = refs[:, 1] - refs[:, 0]
    refs[pick, 0] += rng.uniform(-0.08, 0.08, int(pick.sum()))
    refs[pick, 1] += rng.uniform(-0.3, 0.3, int(pick.sum())) * length[pick]
    refs[:, 1] = np.maximum(refs[:, 1], refs[:, 0])
    refs = refs[rng.random(n) > 0.15]
    k = int(rng.integers(0, 3))
    start = rng.uniform(0.0, 1.5, k)
    added = np.stack([start, start + rng.uniform(0.05, 0.5, k), rng.integers(40, 80, k) + rng.choice([0.0, 0.3], k)], axis=1)
    return np.concatenate([refs, added])


def _tuples(counts):
    return [tuple(int(c[f]) for f in FIELDS) for c in np.asarray(counts).reshape(-1)]


def _want(got, pairs, refs, **tolerances):
    """The checker on every decode of a plain sweep's result (events, bends, event_offsets, status): the five integers."""
    from basic_pitch_amd import score

    events, _, ev_offs, status = got
    out = []
    for j, (s, _) in enumerate(pairs):
        if status[j]:
            out.append((len(refs[s]), 0, 0, 0, int(status[j])))
            continue
        c = score.score_note_events(_rows(events, int(ev_offs[j]), int(ev_offs[j + 1])), refs[s], **tolerances)
        out.append(tuple(int(c[f]) for f in FIELDS))
    return out


def _ptrs(cat, offs):
    return [cat[k].ctypes.data if offs[-1] else None for k, _ in MAPS]


@pytest.fixture(scope="module")
def job(model):
    """The golden maps cut into one-window segments and the handcrafted segments of tests/test_gpu_sweep.py (0, 1, 5, 142 and
    433 rows: the last keeps its working state in the scratch buffer), that file's twelve sets, refs made from each segment's
    own events under set 0, and the plain sweep of the cross product with the checker's counts for it."""
    from basic_pitch_amd import _native, sweep as SW

    gold = note_cases.golden_output()
    T = gold["note"].shape[0]
    segs = [{k: gold[k][t : t + 142].copy() for k, _ in MAPS} for t in range(0, T, 142)]
    rng = np.random.default_rng(2024)
    segs += [TS._segment(rng, rows) for rows in (0, 1, 5, 142, 433)]
    sets = [TS._prm(dict(TS.BASE, **v)) for v in TS.VARIED]
    cat, offs = TS._cat(segs)
    plain = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    pairs = SW.cross_product(len(sets), len(segs))
    events, _, ev_offs, status = plain
    rng = np.random.default_rng(7)
    refs = [_perturbed(rng, _rows(events, int(ev_offs[i]), int(ev_offs[i + 1]))) for i in range(len(segs))]  # set 0: decodes 0 ...
    want = _want(plain, pairs, refs)
    return dict(segs=segs, sets=sets, cat=cat, offs=offs, refs=refs, pairs=pairs, want=want)


def test_the_reference_is_not_trivial(job):
    want, refs = job["want"], job["refs"]
    assert len(job["segs"]) == 11 and len(job["sets"]) == 12 and len(want) == 132
    ok = [w for w in want if w[4] == 0]
    assert {w[4] for w in want} == {0, 1}  # the set with no onset threshold is the host's
    assert sum(len(r) for r in refs) >= 40
    assert sum(w[2] for w in ok) >= 200 and sum(w[2] > w[3] for w in ok) >= 10  # matches, and offsets that miss
    assert sum(0 < w[2] < min(w[0], w[1]) for w in ok) >= 10                    # partial matchings
    assert len({w[:4] for w in ok}) >= 20


def test_the_cross_product_equals_sweep_plus_checker(model, job):
    from basic_pitch_amd import _native, score

    got = score.note_events_sweep_score(model, job["offs"], *_ptrs(job["cat"], job["offs"]), _native.BP_MEM_HOST, job["sets"],
                                        job["refs"])
    assert _tuples(got) == job["want"]


def test_an_explicit_table_with_a_repeated_pair_equals_its_own_permutation(model, job):
    from basic_pitch_amd import _native, score

    rng = np.random.default_rng(5)
    pairs = job["pairs"]
    order = list(rng.permutation(len(pairs))[:60]) + [17, 17, 40]
    table = [pairs[k] for k in order]
    got = score.note_events_sweep_score(model, job["offs"], *_ptrs(job["cat"], job["offs"]), _native.BP_MEM_HOST, job["sets"],
                                        job["refs"], table)
    assert _tuples(got) == [job["want"][k] for k in order]


def test_maps_in_device_memory_and_the_python_entry(model, job):
    import torch

    from basic_pitch_amd import score

    dev = [{k: torch.from_numpy(s[k]).cuda() for k, _ in MAPS} for s in job["segs"]]
    before = [{k: d[k].clone() for k in d} for d in dev]
    got = model.sweep_note_scores(dev, job["sets"], job["refs"])
    torch.cuda.synchronize()
    for d, b in zip(dev, before):
        for k in d:
            assert torch.equal(d[k].view(torch.int32), b[k].view(torch.int32)), k
    assert got.shape == (12, 11) and got.dtype == score.COUNTS
    native = [w for w in job["want"]]
    flat = _tuples(got)
    for j, (w, g) in enumerate(zip(native, flat)):
        if w[4] == 0:
            assert g == w, j
        else:  # the decodes the device leaves are scored by the host route; the status stays
            assert g[4] == w[4] == 1 and g[0] == w[0], j
    # ... and that host route is the host decoder followed by the checker
    from basic_pitch_amd import note_creation as NC

    p = next(i for i, v in enumerate(TS.VARIED) if v.get("onset_thresh") == 0.0)
    n_host = 0
    for i, seg in enumerate(job["segs"]):
        if seg["note"].shape[0] == 0:
            continue
        maps = [seg[k].copy() for k, _ in MAPS]
        T = maps[0].shape[0]
        decoded = NC._grow_and_call(model._lib.bp_notes_decode, tuple(m.ctypes.data for m in maps) + (T, C.byref(job["sets"][p])), T,
                                    "bp_notes_decode")
        ev = NC._note_events(*decoded, True)
        c = score.score_note_events(ev, job["refs"][i])
        assert flat[p * 11 + i] == tuple(int(c[f]) for f in FIELDS[:4]) + (1,), i
        n_host += len(ev)
    assert n_host >= 10
    # pairs: one record per pair; host maps give the same
    some = [(8, 2), (3, 0), (8, 2), (0, 1)]
    listed = model.sweep_note_scores(job["segs"], job["sets"], job["refs"], pairs=some)
    assert _tuples(listed) == [flat[p * 11 + i] for i, p in some]


def test_other_tolerances_and_strict_reach_the_kernel(model, job):
    from basic_pitch_amd import _native, score, sweep as SW

    segs = job["segs"][:5]
    cat, offs = TS._cat(segs)
    sets = job["sets"][:2]
    plain = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    pairs = SW.cross_product(2, 5)
    seen = set()
    for tol in (dict(strict=1), dict(onset_tolerance_s=0.02, offset_ratio=0.1, offset_min_tolerance_s=0.01),
                dict(onset_tolerance_s=0.2, pitch_tolerance_cents=0.0), dict(pitch_tolerance_cents=130.0, offset_ratio=0.0)):
        got = _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, job["refs"][:5], **tol))
        assert got == _want(plain, pairs, job["refs"][:5], **tol), tol
        seen.add(tuple(got))
    assert len(seen) >= 3  # the tolerances change the counts


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
def test_clips_through_the_model_equal_the_clips_sweep_plus_checker(handles, mode):
    from basic_pitch_amd import clips as CL, score, sweep as SW

    m = handles(mode)
    sets = [TS._prm(v) for v in TS.CLIP_SETS]
    matched = 0
    for sr in (22050, 44100) if mode == "default" else (44100,):
        arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(m, sr))]
        plain = SW.infer_clips_events_sweep(m, arrays, sr, sets)
        events, _, ev_offs, status = plain
        rng = np.random.default_rng(11)
        refs = [_perturbed(rng, _rows(events, int(ev_offs[i]), int(ev_offs[i + 1]))) for i in range(3)]
        pairs = SW.cross_product(3, 3)
        want = _want(plain, pairs, refs)
        assert _tuples(score.infer_clips_events_sweep_score(m, arrays, sr, sets, refs)) == want, (mode, sr)
        table = [(2, 1), (1, 0), (2, 1)]
        assert _tuples(score.infer_clips_events_sweep_score(m, arrays, sr, sets, refs, table)) == [want[p * 3 + i] for i, p in table]
        matched += sum(w[2] for w in want)
    assert matched >= 3


def test_transcribe_clips_sweep_scores_groups_the_rates_and_finishes_on_the_host(model):
    from basic_pitch_amd import note_creation as NC, score

    clips = TS._clips_at(model, 22050)[1:] + TS._clips_at(model, 44100)[1:]
    rates = [22050, 22050, 44100, 44100]
    sets = [NC._note_params(ot, 0.3, 11, True, None, None, True, NC.ENERGY_TOLERANCE, True) for ot in (0.5, 0.0, 0.6)]
    events = model.transcribe_clips_sweep(clips, rates, sets)  # [set][clip], complete: set 1 by the host route
    refs = [SC.notes([(e[0], e[1], e[2]) for e in events[2][i]]) for i in range(4)]  # set 2 is the planted one
    got = model.transcribe_clips_sweep_scores(clips, rates, sets, refs)
    assert got.shape == (3, 4) and got["status"].tolist() == [[0] * 4, [1] * 4, [0] * 4]
    for p in range(3):
        for i in range(4):
            c = score.score_note_events(events[p][i], refs[i])
            assert tuple(int(got[p, i][f]) for f in FIELDS[:4]) == tuple(int(c[f]) for f in FIELDS[:4]), (p, i)
    assert (got["matched_offset"][2] == got["n_ref"][2]).all() and got["n_ref"].sum() >= 4
    assert score.precision_recall_f1(got)[2][2].tolist() == [1.0] * 4
    listed = model.transcribe_clips_sweep_scores(clips, rates, sets, refs, pairs=[(3, 2), (0, 0), (2, 1)])
    assert _tuples(listed) == [_tuples(got[2, 3])[0], _tuples(got[0, 0])[0], _tuples(got[1, 2])[0]]


# ---- augmenting on the device
STEP = 2  # bins between the simultaneous notes: the tracker zeroes a found note's neighbouring bins, adjacent bins cannot sound together


def _eight_notes():
    """Rectangles in the note map with an onset peak on their first row: 8 simultaneous notes, pitches 50, 52 ... 64."""
    T = 40
    m = {"note": np.zeros((T, 88), np.float32), "onset": np.zeros((T, 88), np.float32), "contour": np.zeros((T, 264), np.float32)}
    for i in range(8):
        f = 50 - 21 + STEP * i
        m["note"][5:25, f] = 0.8
        m["onset"][5, f] = 0.9
    return m


@pytest.mark.parametrize("decoy_low", (True, False))
def test_the_device_augments_through_a_chain_of_eight(model, decoy_low):
    from basic_pitch_amd import _native, score, sweep as SW

    seg = _eight_notes()
    sets = [TS._prm(dict(TS.BASE, melodia_trick=False))]
    cat, offs = TS._cat([seg])
    events, _, ev_offs, status = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    est = _rows(events, 0, int(ev_offs[1]))
    # first the stage before: the maps decode to the 8 notes, in the tracker's order (bins from the top)
    assert status[0] == 0 and est[:, 2].tolist() == [64, 62, 60, 58, 56, 54, 52, 50]
    assert len(set(est[:, 0])) == 1 == len(set(est[:, 1])) and est[0, 0] == SC.frame_time(5) and est[0, 1] == SC.frame_time(25)
    # refs between the notes, each hitting two of them at 50 x STEP cents, and the decoy that hits the lowest (highest) alone
    _, ref = SC.long_chain(50.0, decoy_low, start=est[0, 0], end=est[0, 1])
    ref[:, 2] = 50.0 + STEP * (ref[:, 2] - 50.0)
    tol = dict(pitch_tolerance_cents=50.0 * STEP)
    g = SC.graphs(est, ref, **tol)[0]
    assert g.sum() == 15 and SC.matching_size(g) == 8
    assert SC.first_fit(g) == (8 if decoy_low else 7)  # in the tracker's order the high decoy strands a first fit
    assert SC.first_fit(g[:, ::-1]) == (7 if decoy_low else 8)  # ... and the low one a matcher that scans the other way
    got = score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, [ref], **tol)
    assert _tuples(got) == [(8, 8, 8, 8, 0)]
    # with the default 50 cents no ref hits a note
    assert _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, [ref])) == [(8, 8, 0, 0, 0)]


def test_hundreds_of_refs_per_segment_scan_several_chunks_and_deep_paths(model, job):
    """Every event hit by a dozen jittered refs in shuffled order: scans that run over several 64-ref chunks, go on in the
    middle of one after a dead end, mark bits in several words of the bitmap, and paths through many held refs."""
    from basic_pitch_amd import _native, score, sweep as SW

    segs, sets = [job["segs"][9], job["segs"][10]], [job["sets"][0], job["sets"][4]]
    cat, offs = TS._cat(segs)
    plain = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    events, _, ev_offs, _ = plain
    rng = np.random.default_rng(3)
    refs = []
    for i in range(2):
        own = _rows(events, int(ev_offs[i]), int(ev_offs[i + 1]))
        many = np.tile(own, (12, 1))
        many[:, 0] += rng.uniform(-0.06, 0.06, len(many))
        many[:, 1] = np.maximum(many[:, 1] + rng.uniform(-0.1, 0.1, len(many)), many[:, 0])
        many[:, 2] += rng.choice([-1.0, -0.5, 0.0, 0.0, 0.5, 1.0], len(many))
        refs.append(many[rng.permutation(len(many))])
    assert min(len(r) for r in refs) > 128
    pairs = SW.cross_product(2, 2)
    for tol in ({}, dict(strict=1), dict(onset_tolerance_s=0.03, pitch_tolerance_cents=100.0)):
        want = _want(plain, pairs, refs, **tol)
        assert _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, refs, **tol)) == want, tol
        assert all(w[4] == 0 and w[2] >= 10 for w in want), want
    # ... and scarce refs among many that hit nothing: 40 simultaneous notes two bins apart, 40 refs of random pitch that hit one
    # or two of them at 150 cents, 150 refs a second late, shuffled.  A first fit in either order finds less than the maximum.
    T = 40
    seg = {"note": np.zeros((T, 88), np.float32), "onset": np.zeros((T, 88), np.float32), "contour": np.zeros((T, 264), np.float32)}
    seg["note"][5:25, 1:80:2] = 0.8
    seg["onset"][5, 1:80:2] = 0.9
    sets = [TS._prm(dict(TS.BASE, melodia_trick=False))]
    cat, offs = TS._cat([seg])
    plain = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
    est = _rows(plain[0], 0, int(plain[2][1]))
    assert est[:, 2].tolist() == [22 + 2 * i for i in range(39, -1, -1)] and len(set(est[:, 0])) == 1 == len(set(est[:, 1]))
    rng = np.random.default_rng(0)
    hit = np.stack([np.full(40, est[0, 0]), np.full(40, est[0, 1]), rng.uniform(21, 102, 40)], axis=1)
    late = np.stack([np.full(150, est[0, 0] + 1.0), np.full(150, est[0, 1] + 1.0), rng.uniform(21, 102, 150)], axis=1)
    ref = np.concatenate([hit, late])[rng.permutation(190)]
    tol = dict(pitch_tolerance_cents=150.0)
    g = SC.graphs(est, ref, **tol)[0]
    size = SC.matching_size(g)
    assert max(SC.first_fit(g), SC.first_fit(g[:, ::-1])) < size and size >= 25
    got = _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, [ref], **tol))
    assert got == [(190, 40, size, size, 0)] == _want(plain, [(0, 0)], [ref], **tol)


# ---- statuses
def test_statuses_1_2_and_3_leave_n_ref_and_change_no_other_decode(model, job):
    from basic_pitch_amd import _native, score

    clean, refs = job["segs"][:3], job["refs"][:3]
    nan = {k: v.copy() for k, v in job["segs"][1].items()}
    nan["note"][50, 40] = np.nan
    dense = {"note": np.ones((64, 88), np.float32), "onset": np.zeros((64, 88), np.float32), "contour": np.zeros((64, 264), np.float32)}
    # tests/test_gpu_clips_events.py: with a frame threshold of 0 every note runs to the end and the bends the set asks for pass
    # the capacity of the decode's region — the scoring call makes no bends but counts them, so that its statuses are the sweep's
    dense["onset"][1:62:2, ::2] = 0.9
    many = np.tile(np.array([[0.5, 1.0, 60.0]]), (score.MAX_NOTES + 1, 1))
    empty = {k: np.zeros((142, w), np.float32) for k, w in MAPS}  # decodes to no event
    overflow = TS._prm(dict(onset_thresh=0.5, frame_thresh=0.0, min_note_len=0, infer_onsets=False, melodia_trick=False))
    sets = [job["sets"][0], overflow]

    def call(segs, seg_refs):
        cat, offs = TS._cat(segs)
        return _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, seg_refs))

    alone = call(clean, refs)
    assert [a[4] for a in alone] == [0] * 6 and sum(a[2] for a in alone) >= 10
    #                 0..2   3    4      5         6      7
    both = call(clean + [nan, dense, job["segs"][1], empty, empty], refs + [refs[1], refs[0], many, np.zeros((0, 3)), refs[2]])
    n = 8
    for p in range(2):
        assert both[p * n : p * n + 3] == alone[p * 3 : p * 3 + 3], p                  # unchanged
        assert both[p * n + 3] == (len(refs[1]), 0, 0, 0, 1)                           # a NaN
        assert both[p * n + 5] == (score.MAX_NOTES + 1, 0, 0, 0, 3)                    # too many refs
        assert both[p * n + 6] == (0, 0, 0, 0, 0) and both[p * n + 7] == (len(refs[2]), 0, 0, 0, 0)  # no refs; no events
    assert both[4][4] == 0 and both[n + 4] == (len(refs[0]), 0, 0, 0, 2)               # the dense segment under frame threshold 0
    assert len(refs[0]) > 0 and len(refs[1]) > 0 and len(refs[2]) > 0
    # exactly the bound is scored: MAX_NOTES refs at one place, every event near it matches
    at_bound = call([job["segs"][1]], [many[:-1]])
    assert at_bound[0][0] == score.MAX_NOTES and at_bound[0][4] == 0 and at_bound[0][1] > 0


# ---- the events calls on the same handle
def test_the_sweep_calls_before_and_after_a_scoring_call_are_byte_equal(model, job):
    from basic_pitch_amd import _native, score, sweep as SW

    cat, offs, sets = job["cat"], job["offs"], job["sets"]

    def plain():
        events, bends, ev_offs, status = SW.note_events_sweep(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets)
        n = int(ev_offs[-1])
        return bytes(events)[: n * C.sizeof(_native.bp_note_event)], bends[: sum(e.n_bends for e in events[:n])].tobytes(), \
            ev_offs.tobytes(), status.tobytes()

    def scored():
        return _tuples(score.note_events_sweep_score(model, offs, *_ptrs(cat, offs), _native.BP_MEM_HOST, sets, job["refs"]))

    a = plain()
    s1 = scored()
    b = plain()
    s2 = scored()
    assert a == b and s1 == s2 == job["want"]
    assert len(a[0]) >= 300 * 48 and len(a[1]) > 0  # events with their bends, which the scoring calls neither make nor disturb
    one = TS._single(model, job["segs"][1], sets[0])
    scored()
    TS._same(TS._single(model, job["segs"][1], sets[0]), one, "bp_note_events_from_maps after a scoring call")


# ---- refusals
def test_refusals_name_the_index_and_leave_the_handle_usable(model, job):
    from basic_pitch_amd import _native, score, sweep as SW

    INV = _native.BP_ERR_INVALID_ARG
    segs = job["segs"][:3]
    cat, offs = TS._cat(segs)
    lib = score.bind(model._lib)
    h = model._handle
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    sets = SW.sets_array(job["sets"][:2])
    good_offs, good = score.refs_table(job["refs"][:3])
    assert len(good) >= 6 and good_offs[1] >= 2

    def call(ref_offs=good_offs, refs=good, prm=None, n_decodes=6, table=None, scores=True, status=True, **tol):
        prm = prm if prm is not None else score.score_params(**tol)
        sc, st = np.zeros((max(1, n_decodes), 4), np.int32), np.zeros(max(1, n_decodes), np.int32)
        rc = lib.bp_note_events_sweep_score(h, 3, p64(offs), *_ptrs(cat, offs), _native.BP_MEM_HOST, 2, C.addressof(sets), n_decodes,
                                            C.addressof(table) if table is not None else None,
                                            p64(ref_offs) if ref_offs is not None else None, refs.ctypes.data if refs is not None else None,
                                            C.addressof(prm), sc.ctypes.data if scores else None, st.ctypes.data if status else None)
        return rc, lib.bp_last_error(h).decode()

    def refused(want, **kw):
        rc, msg = call(**kw)
        assert rc == INV and "bp_note_events_sweep_score" in msg and all(w in msg for w in want), msg
        rc, msg = call()  # the handle takes the next call
        assert rc == _native.BP_OK, msg

    def with_ref(i, field, value):
        r = good.copy()
        r[i, field] = value
        return r

    k = len(good) - 1
    refused((f"ref {k}:", "not finite"), refs=with_ref(k, 0, np.nan))
    refused(("ref 1:", "not finite"), refs=with_ref(1, 1, np.inf))
    refused(("ref 0:", "not finite"), refs=with_ref(0, 2, -np.inf))
    refused(("ref 2:", "end_s < start_s"), refs=with_ref(2, 1, good[2, 0] - 1e-9))
    down = good_offs.copy()
    down[2] = down[1] - 1
    refused(("segment 1:", "ref_offsets decrease"), ref_offs=down)
    up = good_offs.copy()
    up[0] = 1
    refused(("ref_offsets must start at 0",), ref_offs=up)
    for field in ("onset_tolerance_s", "offset_ratio", "offset_min_tolerance_s", "pitch_tolerance_cents"):
        refused(("score_params", "negative or not finite"), **{field: -0.01})
        refused(("score_params", "negative or not finite"), **{field: np.nan})
    refused(("score_params", "reserved"), reserved=1)
    refused(("null ref_offsets or scores",), ref_offs=None)
    refused(("null ref_offsets or scores",), scores=False)
    refused(("status",), status=False)
    refused(("null refs",), refs=None)
    # what the sweep calls refuse is refused here, by the same words
    tab = SW.decode_table([(0, 0), (3, 1)])
    refused(("decode 1:", "segment 3"), table=tab, n_decodes=2)
    refused(("n_sets * n_segments",), n_decodes=5)
    bad_sets = SW.sets_array([job["sets"][0], TS._prm(dict(TS.BASE, min_note_len=-1))])
    sc, st = np.zeros((6, 4), np.int32), np.zeros(6, np.int32)
    prm = score.score_params()
    rc = lib.bp_note_events_sweep_score(h, 3, p64(offs), *_ptrs(cat, offs), _native.BP_MEM_HOST, 2, C.addressof(bad_sets), 6, None,
                                        p64(good_offs), good.ctypes.data, C.addressof(prm), sc.ctypes.data, st.ctypes.data)
    assert rc == INV and "set 1:" in lib.bp_last_error(h).decode()
    # the clips call checks the same arguments
    from basic_pitch_amd import clips as CL

    arrays = [CL.as_clip(c, i) for i, c in enumerate(TS._clips_at(model, 22050))]
    clip_tab = CL.clip_table(arrays)
    bad = with_ref(1, 0, np.nan)
    rc = lib.bp_infer_clips_events_sweep_score(h, 3, clip_tab, 22050, _native.BP_MEM_HOST, 2, C.addressof(sets), 6, None, p64(good_offs),
                                               bad.ctypes.data, C.addressof(prm), sc.ctypes.data, st.ctypes.data)
    msg = lib.bp_last_error(h).decode()
    assert rc == INV and "bp_infer_clips_events_sweep_score" in msg and "ref 1:" in msg, msg
    # nothing to do is no error: no decodes; no rows at all (every decode {n_ref, 0, 0, 0}, status 0)
    rc, msg = call(n_decodes=0, table=SW.decode_table([]))
    assert rc == _native.BP_OK, msg
    none = np.zeros(4, np.int64)
    rc = lib.bp_note_events_sweep_score(h, 3, p64(none), None, None, None, _native.BP_MEM_HOST, 2, C.addressof(sets), 6, None,
                                        p64(good_offs), good.ctypes.data, C.addressof(prm), sc.ctypes.data, st.ctypes.data)
    assert rc == _native.BP_OK and st.tolist() == [0] * 6
    assert sc.tolist() == [[int(good_offs[i + 1] - good_offs[i]), 0, 0, 0] for i in range(3)] * 2


# ---- Python: the planted set wins
def test_best_set_picks_the_planted_set(model, job):
    from basic_pitch_amd import score

    # the golden segments and the handcrafted one-window segment, whose notes of 5 and 8 frames a minimum length of 7 tells apart
    segs, sets = job["segs"][:6] + [job["segs"][9]], job["sets"]
    planted = 5
    assert TS.VARIED[planted] == {"min_note_len": 7} and segs[6]["note"].shape[0] == 142
    events = model.sweep_note_events(segs, sets, pairs=[(i, planted) for i in range(7)])
    assert all(st == 0 for _, st in events)
    refs = [SC.notes([(e[0], e[1], e[2]) for e in ev]) for ev, _ in events]
    assert sum(len(r) for r in refs) >= 20
    got = model.sweep_note_scores(segs, sets, refs)
    assert got.shape == (12, 7)
    total = {name: got[name].sum(axis=1) for name in FIELDS[:4]}
    assert total["matched_offset"][planted] == total["n_ref"][planted] == total["n_est"][planted] == sum(len(r) for r in refs)
    assert score.best_set(got) == planted and score.best_set(got, offsets=False) == planted
    assert all(total["n_est"][p] != total["n_ref"][p] or total["matched_offset"][p] < total["n_ref"][p] for p in range(planted))
