"""The launch regimes of the dense path as the launchers themselves state them (csrc/launch_plan.h through the handle-free
hook bp_launch_plan), and the batch sizes that enter every regime and stand on both sides of every change.  Shared by
tests/test_launch_plan_cpu.py (which checks the list against the full enumeration) and tests/test_gpu_launch_regimes.py
(which runs every size).  Needs the library, no device.

A plan is reduced to its SIGNATURE, one categorical value per decision:

  pyramid        one per-window launch | the wide decimators + tail chain
  fused          the filterbank normalises its own windows | strided tasks + zpack
  fb_multi       a filterbank workgroup owns more than one window
  chunks         frame chunks per window of the contour conv1 march
  rim            items of a rim-march workgroup against its ring of five LDS-DMA buffers: 0 (no rim march: the extended
                 mode's GEMM), 1, 2-4 (a prologue shorter than the ring), 5 (the ring exactly full), 6+ (the first wrap)
  c2_launches    conv2 launches of at most 256 windows: 1 | 2+ (a third launch repeats the loop step of the second)
  c2_groups      groups of 16 windows of the LAST conv2 launch: 1 | 2-15 | 16
  c2_slabs       frame slabs of the last conv2 launch (each slab count has its own slab height and its own halo seams)
  c2_ragged      the last group of the last conv2 launch holds fewer than 16 windows
  note_sat, onset_sat    the march's grid has reached its resident workgroups
  note_aligned, onset_aligned    the eight-waves-per-window cut
  note_prio, onset_prio, conv1_prio    the priority hand-over is on
  note_spans, onset_spans    a wave's share is longer than one (window, strip) pair

`sizes()` thins what the enumeration yields to MAX_SIZES sizes (MAX_ABOVE of them above 2 n_cu), because every size is a
GPU case of every mode for every later run of the suite.  What it never gives up: 1, n_cu, 2 n_cu and the largest size;
the FIRST change of every field, on both sides; one size inside every value of every field.  Then it adds, smallest size
first and as long as the caps hold, the first occurrence of every other transition (field, from, to), on both sides.  A
change that is left without its two sizes is therefore one whose field has another change straddled and whose two values
are both entered: a further step of a ladder (slab counts, chunk counts) whose every rung is run, or a repetition (the
ragged flag flips every 16 windows)."""
import ctypes as C
from functools import lru_cache

MODES = {"default": {}, "bf16_weights": {"bf16_weights": True}, "ext_cqt_44k": {"ext_cqt_44k": True}}
MAX_SIZES, MAX_ABOVE = 40, 6
FIELDS = ("pyramid", "fused", "fb_multi", "chunks", "rim", "c2_launches", "c2_groups", "c2_slabs", "c2_ragged", "note_sat",
          "onset_sat", "note_aligned", "onset_aligned", "note_prio", "onset_prio", "conv1_prio", "note_spans", "onset_spans")
# the stage of bp_run_stage whose launchers decide each field (the whole path decides all of them)
STAGE_FIELDS = {
    "pyramid": ("pyramid",),
    "contour": ("chunks", "rim", "c2_launches", "c2_groups", "c2_slabs", "c2_ragged", "conv1_prio"),
    "note": ("note_sat", "note_aligned", "note_prio", "note_spans"),
    "onset": ("onset_sat", "onset_aligned", "onset_prio", "onset_spans"),
}


def _lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


def mode_flags(mode):
    from basic_pitch_amd import _native

    return {"default": 0, "bf16_weights": _native.BP_FLAG_BF16_WEIGHTS, "ext_cqt_44k": _native.BP_FLAG_EXT_CQT_44K}[mode]


@lru_cache(maxsize=None)
def plan(n, n_cu, mode):
    """bp_launch_plan's struct as a dict"""
    from basic_pitch_amd import _native

    out = _native.bp_launch_plan_out()
    rc = _lib().bp_launch_plan(n, n_cu, mode_flags(mode), C.byref(out))
    assert rc == 0, (rc, n, n_cu, mode)
    return {name: int(getattr(out, name)) for name, _ in out._fields_}


def _rim_class(p):
    if not p["rim_march"]:
        return "0"
    k = p["rim_items_max"]
    return "1" if k == 1 else "2-4" if k < p["rim_ring"] else "5" if k == p["rim_ring"] else "6+"


def signature(n, n_cu, mode):
    p = plan(n, n_cu, mode)
    g = p["conv2_last_groups"]
    return {
        "pyramid": "one_launch" if p["pyramid_one_launch"] else "chain",
        "fused": bool(p["filterbank_fused"]),
        "fb_multi": bool(p["filterbank_fused"]) and n > p["filterbank_grid"],
        "chunks": p["conv1_chunks"],
        "rim": _rim_class(p),
        "c2_launches": "1" if p["conv2_launches"] == 1 else "2+",
        "c2_groups": "1" if g == 1 else "16" if g == 16 else "2-15",
        "c2_slabs": p["conv2_last_slabs"],
        "c2_ragged": p["conv2_last_windows"] % 16 != 0,
        "note_sat": p["note_grid"] == p["note_grid_cap"],
        "onset_sat": p["onset_grid"] == p["onset_grid_cap"],
        "note_aligned": bool(p["note_aligned"]),
        "onset_aligned": bool(p["onset_aligned"]),
        "note_prio": p["note_prio"] != 0,
        "onset_prio": p["onset_prio"] != 0,
        "conv1_prio": p["conv1_prio"] != 0,
        "note_spans": bool(p["note_share_spans_pairs"]),
        "onset_spans": bool(p["onset_share_spans_pairs"]),
    }


def largest(n_cu):
    return 4 * n_cu + 64


@lru_cache(maxsize=None)
def enumerate_signatures(n_cu, mode):
    """signatures of n = 1 .. largest(n_cu), index n - 1"""
    return tuple(signature(n, n_cu, mode) for n in range(1, largest(n_cu) + 1))


def changes(n_cu, mode, fields=FIELDS):
    """[(n, field, from, to)] for every n whose signature differs from that of n - 1 in `field`, ascending in n"""
    sigs = enumerate_signatures(n_cu, mode)
    return [(n, f, sigs[n - 2][f], sigs[n - 1][f]) for n in range(2, len(sigs) + 1) for f in fields if sigs[n - 2][f] != sigs[n - 1][f]]


def unthinned_sizes(n_cu, mode, fields=FIELDS):
    """both sides of every change, and 1, n_cu, 2 n_cu, the largest size"""
    s = {1, n_cu, 2 * n_cu, largest(n_cu)}
    for n, _f, _a, _b in changes(n_cu, mode, fields):
        s |= {n - 1, n}
    return sorted(s)


@lru_cache(maxsize=None)
def sizes(n_cu, mode):
    """the batch sizes to run on a device of n_cu compute units: see the module's text"""
    sigs = enumerate_signatures(n_cu, mode)
    ch = changes(n_cu, mode)
    chosen = {1, n_cu, 2 * n_cu, largest(n_cu)}
    seen_field = set()
    for n, f, _a, _b in ch:  # the first change of every field
        if f not in seen_field:
            seen_field.add(f)
            chosen |= {n - 1, n}
    for f in FIELDS:  # a size inside every value: the first size that enters it, which is a side of the change that leads there
        for v in sorted({s[f] for s in sigs}, key=str):
            if not any(sigs[n - 1][f] == v for n in chosen):
                chosen.add(next(n for n in range(1, len(sigs) + 1) if sigs[n - 1][f] == v))

    def fits(extra):
        now = chosen | extra
        return len(now) <= MAX_SIZES and sum(n > 2 * n_cu for n in now) <= MAX_ABOVE

    assert fits(set()), (n_cu, mode, sorted(chosen))
    seen_transition = set()
    for n, f, a, b in ch:  # the first occurrence of every transition, while the caps hold
        if (f, a, b) in seen_transition:
            continue
        seen_transition.add((f, a, b))
        if fits({n - 1, n}):
            chosen |= {n - 1, n}
    return tuple(sorted(chosen))


def stage_sizes(stage, n_cu, mode):
    """the subset of sizes(n_cu, mode) that stands on both sides of a change of one of the stage's own fields"""
    s = set(sizes(n_cu, mode))
    keep = {1}
    for n, _f, _a, _b in changes(n_cu, mode, STAGE_FIELDS[stage]):
        if n - 1 in s and n in s:
            keep |= {n - 1, n}
    return tuple(sorted(keep))


def describe(n, n_cu, mode):
    return ", ".join(f"{k}={v}" for k, v in signature(n, n_cu, mode).items())
