"""The launch decisions of the dense path (csrc/launch_plan.h, read through the handle-free hook bp_launch_plan) over every
batch size n = 1 .. 4 n_cu + 64, for n_cu in {64, 128, 256, 304} and the three modes, without a device: the batch sizes
tests/launch_regimes.py hands to tests/test_gpu_launch_regimes.py enter every regime and stand on both sides of every
change; the thresholds of a 256-CU device are pinned as literals, so that a moved threshold is seen and not silently
followed; every grid stays within the residency cap its launcher states; conv2's launches cover exactly n windows.

The figures pinned below are what the launchers compute.  Two of them differ from the arithmetic of the issue that asked
for this test, which took the rim march's items per workgroup as 11 n / 128 rounded down: the first workgroup of a side
has ceil(11 n / 128) items (the kernel's n_my), so a workgroup first has two items at 12 windows, exactly the five of the
ring at 47 and the first wrap at 59."""
import os
import re

import pytest

import launch_regimes as L
from conftest import ROOT

N_CU = (64, 128, 256, 304)


def problems(chosen, n_cu, mode):
    """what a list of sizes misses: values no size enters, changes that are neither straddled nor excused"""
    sigs = L.enumerate_signatures(n_cu, mode)
    chosen = set(chosen)
    out = []
    entered = {f: {sigs[n - 1][f] for n in chosen} for f in L.FIELDS}
    for f in L.FIELDS:
        for v in {s[f] for s in sigs} - entered[f]:
            out.append(f"no size enters {f} = {v}")
    ch = L.changes(n_cu, mode)
    straddled = {f for n, f, _a, _b in ch if n - 1 in chosen and n in chosen}
    first = {}
    for n, f, a, b in ch:
        first.setdefault(f, n)
        if n - 1 in chosen and n in chosen:
            continue
        # thinning may drop a change only when the field has another change straddled and both values are entered —
        # and never the field's first change
        if first[f] == n or f not in straddled or a not in entered[f] or b not in entered[f]:
            out.append(f"{f}: {a} -> {b} at {n - 1} | {n} is not straddled")
    return out


@pytest.mark.parametrize("mode", list(L.MODES))
@pytest.mark.parametrize("n_cu", N_CU)
def test_chosen_sizes_enter_every_regime_and_straddle_every_change(n_cu, mode):
    s = L.sizes(n_cu, mode)
    assert list(s) == sorted(set(s)) and s[0] == 1 and s[-1] == L.largest(n_cu)
    assert {1, n_cu, 2 * n_cu, L.largest(n_cu)} <= set(s)
    assert len(s) <= L.MAX_SIZES and sum(n > 2 * n_cu for n in s) <= L.MAX_ABOVE, (len(s), s)
    assert set(s) <= set(L.unthinned_sizes(n_cu, mode))  # thinning only removes
    assert problems(s, n_cu, mode) == []
    # the stage subsets are subsets, and straddle the first change of each of their fields
    for stage, fields in L.STAGE_FIELDS.items():
        sub = L.stage_sizes(stage, n_cu, mode)
        assert set(sub) <= set(s)
        seen = set()
        for n, f, _a, _b in L.changes(n_cu, mode, fields):
            if f not in seen:
                seen.add(f)
                assert n - 1 in sub and n in sub, (stage, f, n)


def test_the_check_notices_a_missing_straddling_size():
    """take one side of a pinned change out of the list: the check that passed above must fail"""
    s = L.sizes(256, "default")
    for gone in (86, 127, 257, 18, 47, 683):
        assert gone in s and problems([n for n in s if n != gone], 256, "default"), gone


def test_bf16_weights_take_the_default_mode_s_launches():
    for n_cu in N_CU:
        for n in range(1, L.largest(n_cu) + 1):
            assert L.plan(n, n_cu, "bf16_weights") == L.plan(n, n_cu, "default")


# (field, from, to): last size of `from` | first size of `to`, on a device of 256 compute units
PINNED_256 = {
    "default": [
        ("pyramid", "chain", "one_launch", 86),       # 3 n >= n_cu
        ("fused", False, True, 128),                  # 2 n >= n_cu
        ("fb_multi", False, True, 257),               # the first filterbank workgroup that owns two windows
        ("chunks", 32, 16, 19), ("chunks", 16, 8, 37), ("chunks", 8, 4, 74),   # n chunks 7 < 2 n_cu 4
        ("rim", "1", "2-4", 12), ("rim", "2-4", "5", 47), ("rim", "5", "6+", 59),  # ceil(11 n / 128) items against a ring of 5
        ("c2_launches", "1", "2+", 257),              # a second launch of one window
        ("c2_groups", "1", "2-15", 17), ("c2_groups", "2-15", "16", 241), ("c2_groups", "16", "1", 257),
        ("c2_slabs", 16, 14, 49), ("c2_slabs", 14, 11, 65), ("c2_slabs", 11, 9, 81), ("c2_slabs", 9, 8, 97),
        ("c2_slabs", 8, 7, 113), ("c2_slabs", 7, 6, 129), ("c2_slabs", 6, 5, 145), ("c2_slabs", 5, 4, 177),
        ("c2_slabs", 4, 3, 225), ("c2_slabs", 3, 16, 257),
        ("c2_ragged", True, False, 16), ("c2_ragged", False, True, 17),
        ("note_sat", False, True, 48), ("note_prio", False, True, 48),     # 43 n / 4 workgroups reach 2 n_cu
        ("onset_sat", False, True, 24), ("onset_prio", False, True, 24),   # 86 n / 4
        ("note_aligned", False, True, 256), ("note_aligned", True, False, 257),
        ("onset_aligned", False, True, 256), ("onset_aligned", True, False, 257),
        ("note_spans", False, True, 683), ("onset_spans", False, True, 683),   # 3 n > 2048 waves
    ],
    "ext_cqt_44k": [
        ("pyramid", "chain", "one_launch", 128),      # n >= n_cu / 2
        ("fused", False, True, 128),
        ("fb_multi", False, True, 257),
    ],
}
# the sizes the GPU test must hold on a 256-CU device, whatever else the list carries
MUST_RUN_256 = {
    "default": [1, 11, 12, 16, 17, 18, 19, 23, 24, 36, 37, 46, 47, 48, 58, 59, 73, 74, 85, 86, 127, 128, 255, 256, 257, 512, 682, 683, 1088],
    "ext_cqt_44k": [1, 16, 17, 18, 19, 23, 24, 36, 37, 47, 48, 73, 74, 127, 128, 255, 256, 257, 512, 682, 683, 1088],
}


@pytest.mark.parametrize("mode", list(L.MODES))
def test_thresholds_of_a_256_cu_device_are_where_they_were(mode):
    key = "ext_cqt_44k" if mode == "ext_cqt_44k" else "default"
    first = {}
    for n, f, a, b in L.changes(256, mode):
        first.setdefault((f, a, b), n)
    for f, a, b, n in PINNED_256[key]:
        assert first.get((f, a, b)) == n, (f, a, b, n, first.get((f, a, b)))
    if key == "default":  # nothing changes that the table does not name
        assert set(first) == {(f, a, b) for f, a, b, _n in PINNED_256[key]}, set(first) ^ {(f, a, b) for f, a, b, _n in PINNED_256[key]}
    else:
        assert all(sig["rim"] == "0" for sig in L.enumerate_signatures(256, mode))  # the rim GEMM: a workgroup per item
    s = L.sizes(256, mode)
    assert set(MUST_RUN_256[key]) <= set(s), sorted(set(MUST_RUN_256[key]) - set(s))
    # the pairs by name: pyramid, filterbank, the first two-window workgroup / second conv2 launch, a size in the
    # end-to-end cut's several-pairs regime
    pyr = 128 if key == "ext_cqt_44k" else 86
    assert {pyr - 1, pyr, 127, 128, 256, 257} <= set(s) and any(n >= 683 for n in s)


@pytest.mark.parametrize("mode", list(L.MODES))
@pytest.mark.parametrize("n_cu", N_CU)
def test_grids_stay_within_the_residency_caps_and_conv2_covers_every_window(n_cu, mode):
    for n in range(1, L.largest(n_cu) + 1):
        p = L.plan(n, n_cu, mode)
        # pyramid: 16 waves per CU, four per workgroup; one workgroup per window otherwise
        assert p["pyramid_decimate_grid_cap"] == 4 * n_cu
        assert (p["pyramid_decimate_grid"] == 0) if p["pyramid_one_launch"] else (1 <= p["pyramid_decimate_grid"] <= 4 * n_cu), n
        # filterbank: at most one workgroup of 1024 threads per CU; fused: every window has an owner
        assert 1 <= p["filterbank_grid"] <= n_cu, n
        if p["filterbank_fused"]:
            assert p["filterbank_grid"] == min(n, n_cu), n
        # contour conv1: two workgroups per CU; chunks a power of two between the full-batch 4 and 32
        assert 1 <= p["conv1_grid"] <= 2 * n_cu and p["conv1_chunks"] in (4, 8, 16, 32), n
        assert p["conv1_grid"] == min(2 * n_cu, -(-n * p["conv1_chunks"] * 7 // 4)), n
        # rim march: one workgroup per CU, half of them per side; every workgroup has an item; shares differ by at most one
        if p["rim_march"]:
            assert p["rim_items"] == 11 * n and 1 <= p["rim_per_side"] <= max(n_cu // 2, 1) and 2 * p["rim_per_side"] <= n_cu, n
            assert p["rim_items_max"] == -(-p["rim_items"] // p["rim_per_side"]), n
            assert 1 <= p["rim_items_min"] <= p["rim_items_max"] <= p["rim_items_min"] + 1, n
            assert p["rim_ring"] == 5
        else:
            assert mode == "ext_cqt_44k"
        # conv2: launches of at most 256 windows that cover exactly n; a launch of several slabs fits the resident waves
        launches = -(-n // 256)
        assert p["conv2_launches"] == launches and p["conv2_windows"] == n, n
        assert p["conv2_first_windows"] == min(n, 256) and p["conv2_last_windows"] == n - 256 * (launches - 1), n
        assert p["conv2_first_windows"] * (launches - 1) + p["conv2_last_windows"] == n, n
        assert p["conv2_slots"] == 16 * n_cu
        for which in ("first", "last"):
            w, g, slabs, rows, grid = (p[f"conv2_{which}_{k}"] for k in ("windows", "groups", "slabs", "slab_rows", "grid"))
            assert g == -(-w // 16) and 1 <= slabs <= 16, n
            assert (slabs - 1) * rows < 172 <= slabs * rows, (n, slabs, rows)   # the slabs tile the 172 frames, none empty
            assert grid == -(-g * slabs * 72 // 4), n
            assert slabs == 1 or g * slabs * 72 <= p["conv2_slots"], (n, g, slabs)
        # marches: two workgroups per CU; the hand-over only with both halves resident
        for m in ("note", "onset"):
            assert p[f"{m}_grid_cap"] == 2 * n_cu and 1 <= p[f"{m}_grid"] <= 2 * n_cu, n
            assert (p[f"{m}_prio"] != 0) == (p[f"{m}_grid"] == 2 * n_cu), n
            assert p[f"{m}_prio"] in (0, 45), n
            assert bool(p[f"{m}_aligned"]) == (4 * p[f"{m}_grid"] == 8 * n), n
            assert bool(p[f"{m}_share_spans_pairs"]) == (3 * n > 4 * p[f"{m}_grid"] and not p[f"{m}_aligned"]), n
        assert p["conv1_prio"] == 0


def test_hook_is_declared_and_refuses_what_it_cannot_plan():
    """the ctypes struct has the header's fields in the header's order; bad arguments are refused, not planned"""
    import ctypes as C

    from basic_pitch_amd import _native

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd.h")).read()
    body = re.search(r"typedef struct bp_launch_plan_out \{(.*?)\} bp_launch_plan_out;", header, flags=re.S).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [name for name, _ in _native.bp_launch_plan_out._fields_]
    assert C.sizeof(_native.bp_launch_plan_out) == 4 * len(fields)
    lib = L._lib()
    out = _native.bp_launch_plan_out()
    assert lib.bp_launch_plan(0, 256, 0, C.byref(out)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_launch_plan(16385, 256, 0, C.byref(out)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_launch_plan(5, 0, 0, C.byref(out)) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_launch_plan(5, 256, 0, None) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_launch_plan(5, 256, _native.BP_FLAG_F32_MFMA, C.byref(out)) == _native.BP_ERR_UNSUPPORTED
    assert lib.bp_launch_plan(16384, 256, 0, C.byref(out)) == 0 and out.conv2_launches == 64 and out.conv2_windows == 16384
