"""What the analyses share on the host side (basic_pitch_amd/jobs.py), without a handle and without a GPU: the sample rates of a
job and the loops over its rate groups on stub calls, the stacker on small numpy maps, the record arrays and the decodes of
a sweep.  The calls that take a handle are in the tests/test_gpu_*.py of the analyses."""
import ctypes as C

import numpy as np
import pytest

from basic_pitch_amd import _native, align, events, jobs, score, sweep

RATES = [44100, 22050, 44100, 22050, 48000]
ALIGN_MISMATCH = "align: the note and onset maps of a segment must have one length and lie in one kind of memory"


@pytest.mark.parametrize("given", [22050, np.int64(22050), [22050] * 3, (22050,) * 3])
def test_rates_of_takes_a_scalar_or_one_rate_per_clip(given):
    rates = jobs.rates_of([None] * 3, given)
    assert rates == [22050, 22050, 22050] and all(type(r) is int for r in rates)


def test_rates_of_refuses_a_wrong_length_and_takes_no_clips():
    with pytest.raises(ValueError, match=r"^3 clips but 2 sample rates$"):
        jobs.rates_of([None] * 3, [22050, 44100])
    assert jobs.rates_of([], 22050) == []
    assert jobs.rates_of([], np.int32(22050)) == []


def test_rate_groups_are_in_order_of_first_appearance():
    assert jobs.rate_groups(RATES) == [(44100, [0, 2]), (22050, [1, 3]), (48000, [4])]
    assert jobs.rate_groups([]) == []


def test_plain_loop_calls_once_per_rate_and_answers_in_input_order():
    calls = []

    def run(ids, rate):
        calls.append((list(ids), rate))
        return [(i, rate) for i in ids]

    assert jobs.per_rate(RATES, run) == [(i, r) for i, r in enumerate(RATES)]
    assert calls == [([0, 2], 44100), ([1, 3], 22050), ([4], 48000)]
    calls.clear()
    assert jobs.per_rate([], run) == [] and calls == []


def _swept(todo):
    """The swept loop on a stub that answers every local pair with (rate, the clip its local index stands for, set)."""
    calls, landed = [], [None] * len(todo)

    def run(ids, rate, local_pairs):
        calls.append((list(ids), rate, list(local_pairs)))
        return [(rate, ids[k], p) for k, p in local_pairs]

    for j, k, rate, reply in jobs.per_rate_swept(todo, RATES, run):
        assert landed[j] is None and reply[k][0] == rate
        landed[j] = reply[k]
    return calls, landed


def test_swept_loop_renumbers_the_segments_and_scatters_to_j():
    pairs = [(3, 2), (0, 1), (2, 0), (1, 1), (0, 1), (2, 2), (3, 0)]  # scrambled, (0, 1) twice, no clip of 48000
    todo = jobs.pairs_checked(pairs, 5, 3, "job", refs=[None] * 5)
    assert todo == pairs
    calls, landed = _swept(todo)
    assert calls == [([0, 2], 44100, [(0, 1), (1, 0), (0, 1), (1, 2)]),   # todo order within the group, local indices
                     ([1, 3], 22050, [(1, 2), (0, 1), (1, 0)])]           # and no call for 48000
    assert landed == [(RATES[s], s, p) for s, p in pairs]


def test_swept_loop_without_pairs_is_the_set_major_cross_product():
    todo = jobs.pairs_checked(None, 5, 3, "job")
    assert todo == sweep.cross_product(3, 5) and todo[:6] == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, 1)]
    calls, landed = _swept(todo)
    assert [(ids, rate) for ids, rate, _ in calls] == [([0, 2], 44100), ([1, 3], 22050), ([4], 48000)]
    grid = np.empty(len(todo), object)
    grid[:] = landed
    grid = grid.reshape(3, 5)  # the caller's reshape to (n_sets, n_seg)
    assert all(grid[p, s] == (RATES[s], s, p) for p in range(3) for s in range(5))


def test_pairs_checked_keeps_the_messages():
    with pytest.raises(ValueError, match=r"^sweep_note_events: a pair names a segment outside 0\.\.4 or a set outside 0\.\.2$"):
        jobs.pairs_checked([(0, 0), (5, 0)], 5, 3, "sweep_note_events")
    with pytest.raises(ValueError, match=r"^sweep_note_scores: a pair names a segment outside 0\.\.4 or a set outside 0\.\.2$"):
        jobs.pairs_checked([(0, 3)], 5, 3, "sweep_note_scores", refs=[None] * 5)
    with pytest.raises(ValueError, match=r"^sweep_note_scores: 5 segments but refs for 4$"):
        jobs.pairs_checked(None, 5, 3, "sweep_note_scores", refs=[None] * 4)
    assert jobs.pairs_checked([], 5, 3, "job") == []


def _maps(rows, seed=0):
    rng = np.random.default_rng(seed)
    return [{"note": rng.random((t, 88), np.float32), "onset": rng.random((t, 88), np.float32),
             "contour": rng.random((t, 264), np.float32)} for t in rows]


def test_stacker_stacks_numpy_segments_of_0_1_and_3_rows():
    outs = _maps([0, 1, 3])
    offs, maps, ptrs, mem_kind = jobs.stack(outs, ("note", "onset", "contour"), "job")
    assert offs.dtype == np.int64 and offs.tolist() == [0, 0, 1, 4]
    assert list(maps) == ["note", "onset", "contour"] and mem_kind == _native.BP_MEM_HOST
    for k in maps:
        assert maps[k].dtype == np.float32 and maps[k].flags["C_CONTIGUOUS"]
        assert np.array_equal(maps[k], np.concatenate([o[k] for o in outs])) and ptrs[k] == maps[k].ctypes.data
    offs, maps, ptrs, _ = jobs.stack(outs, ("onset",), "job")  # a subset of the planes
    assert list(maps) == ["onset"] == list(ptrs) and offs.tolist() == [0, 0, 1, 4]
    same = events.stack_maps(outs, "job")
    assert same[0].tolist() == [0, 0, 1, 4] and list(same[1]) == ["note", "onset", "contour"]


def test_stacker_passes_one_ready_segment_through_and_converts_the_rest():
    out = _maps([3])[0]
    _, maps, ptrs, _ = jobs.stack([out], ("note", "contour"), "job")
    assert maps["note"] is out["note"] and maps["contour"] is out["contour"] and ptrs["note"] == out["note"].ctypes.data
    wide = out["contour"].astype(np.float64)
    _, maps, _, _ = jobs.stack([wide], ("contour",), "job", bare=True)
    assert maps["contour"] is not wide and maps["contour"].dtype == np.float32 and np.array_equal(maps["contour"], out["contour"])
    fortran = np.asfortranarray(out["note"])
    assert not fortran.flags["C_CONTIGUOUS"]
    _, maps, _, _ = jobs.stack([{"note": fortran}], ("note",), "job")
    assert maps["note"] is not fortran and maps["note"].flags["C_CONTIGUOUS"] and np.array_equal(maps["note"], out["note"])


def test_stacker_refuses_a_wrong_width():
    out = _maps([2])[0]
    with pytest.raises(ValueError, match=r"^contour: expected \(T, 264\)$"):
        jobs.stack([dict(out, contour=out["contour"][:, :263])], ("contour",), "job")
    with pytest.raises(ValueError, match=r"^note: expected \(T, 88\)$"):
        jobs.stack([dict(out, note=out["contour"])], ("note", "onset"), "job")
    with pytest.raises(ValueError, match=r"^onset: expected \(T, 88\)$"):
        jobs.stack([dict(out, onset=out["onset"][0])], ("note", "onset"), "job")


def test_stacker_takes_a_bare_map_only_where_allowed():
    contour = _maps([2])[0]["contour"]
    offs, maps, _, _ = jobs.stack([contour, {"contour": contour}], ("contour",), "job", bare=True)
    assert offs.tolist() == [0, 2, 4] and np.array_equal(maps["contour"], np.concatenate([contour, contour]))
    with pytest.raises(IndexError):  # what indexing an array with the plane's name raises
        jobs.stack([contour], ("contour",), "job")


def test_stacker_without_rows_gives_no_pointers():
    offs, maps, ptrs, mem_kind = jobs.stack(_maps([0, 0]), ("note", "onset", "contour"), "job")
    assert offs.tolist() == [0, 0, 0] and ptrs == {"note": None, "onset": None, "contour": None}
    assert mem_kind == _native.BP_MEM_HOST and maps["contour"].shape == (0, 264)


def test_planes_that_disagree_in_rows_get_each_callers_words():
    outs = _maps([2, 3])
    outs[1]["onset"] = outs[1]["onset"][:2]
    with pytest.raises(ValueError, match=r"^note_events: note, onset and contour of a segment must have the same number of rows$"):
        events.stack_maps(outs, "note_events")
    with pytest.raises(ValueError, match="^" + ALIGN_MISMATCH + "$"):
        align.align(None, outs, [[], []])  # the stacker refuses before the handle is looked at
    with pytest.raises(ValueError, match="^" + ALIGN_MISMATCH + "$"):
        jobs.stack(outs, ("note", "onset"), "align", mismatch=ALIGN_MISMATCH)


def test_records_fill_field_by_field():
    table = np.arange(12, dtype=np.int32).reshape(3, 4) + 1
    status = np.array([0, 2, 0, 7], np.int32)  # longer than n, as the calls' buffers may be
    out = jobs.records(score.COUNTS, table, status, 3)
    assert out.dtype == score.COUNTS and out.shape == (3,)
    for i, name in enumerate(("n_ref", "n_est", "matched_onset", "matched_offset")):
        assert out[name].tolist() == table[:, i].tolist()
    assert out["status"].tolist() == [0, 2, 0]
    assert jobs.records(score.COUNTS, np.zeros((1, 4), np.int32), np.zeros(1, np.int32), 0).shape == (0,)


def test_decodes_block_of_the_cross_product_and_of_a_pair_list():
    sets = (_native.bp_note_params * 3)()
    block, n = jobs.decodes_block(sets, 3, None, 5)
    assert n == 15 and block == (3, C.addressof(sets), 15, None)
    pairs = [(4, 2), (0, 0), (4, 2)]
    block, n = jobs.decodes_block(sets, 3, pairs, 5)
    assert n == 3 and block[:3] == (3, C.addressof(sets), 3) and len(block) == 4
    table = C.cast(block[3], C.POINTER(_native.bp_sweep_decode))  # as the call reads it; the tuple holds the array
    assert [(table[j].segment, table[j].params, table[j].reserved) for j in range(n)] == [(s, p, 0) for s, p in pairs]


def test_offsets_of():
    assert jobs.offsets_of([0, 1, 3]).tolist() == [0, 0, 1, 4] and jobs.offsets_of([0, 1, 3]).dtype == np.int64
    assert jobs.offsets_of([]).tolist() == [0] and jobs.offsets_of([]).dtype == np.int64
    assert jobs.offsets_of(np.array([2, 2], np.int32)).dtype == np.int64
