"""The seam and halo geometry of contour conv2 inside the conv1 march (csrc/launch_plan.h kCf*, cf_*), re-stated here and
enumerated without a device: for 4, 8, 16 and 32 frame chunks every one of the 25 taps of every output (172 x 264) is
delivered exactly once, and the terms of an output are added in the order dt = 0 .. 4 whatever the chunk count.

The layout factorises — a record is (kind of row) x (class, element) — so the frame direction (chunks, prefixes, single
terms) and the bin direction (strips, classes, halo columns, rim lanes) are enumerated separately; an output's taps are the
product of the two.  The writer below is the march's epilogue (conv_contour_march.hip), the reader is
contour_conv2_seam_kernel + contour_conv2_finish_kernel (conv_contour2.hip); the constants come from bp_launch_plan."""
import ctypes as C

import pytest

import launch_regimes as L
from basic_pitch_amd import _native

FRAMES, BINS, STRIPS = 172, 264, 7


@pytest.fixture(scope="module")
def plan():
    out = _native.bp_launch_plan_out()
    assert L._lib().bp_launch_plan(256, 256, 0, C.byref(out)) == 0
    return out


def test_plan_states_the_layout(plan):
    assert plan.conv2_fused == 1
    assert (plan.fused_cols, plan.fused_seam_rows, plan.fused_term_rows) == (36, 4, 10)
    seam = (plan.fused_seam_rows + plan.fused_term_rows) * 3 * 32
    assert plan.fused_window_floats == STRIPS * FRAMES * plan.fused_cols + 31 * STRIPS * seam
    assert plan.fused_window_floats <= 8 * FRAMES * BINS  # the plane the partial sums live in
    # the finisher: slabs tile the frames; several slabs only within the resident waves (two per SIMD)
    for n in (1, 2, 19, 37, 74, 256, 300):
        p = _native.bp_launch_plan_out()
        assert L._lib().bp_launch_plan(n, 256, 0, C.byref(p)) == 0
        assert 1 <= p.finish_slabs <= 16 and (p.finish_slabs - 1) * p.finish_slab_rows < FRAMES <= p.finish_slabs * p.finish_slab_rows
        assert p.finish_grid == -(-n * p.finish_slabs // 4)
        assert p.finish_slabs == 1 or n * p.finish_slabs <= 256 * 4 * 2
    ext = _native.bp_launch_plan_out()
    assert L._lib().bp_launch_plan(256, 256, _native.BP_FLAG_EXT_CQT_44K, C.byref(ext)) == 0 and ext.conv2_fused == 0


def chunk_t0(ci, chunks):
    return ci * FRAMES // chunks


def seam_of_row(t, chunks):
    """(ci, r) when output row t is one of the rows T0 - 2 .. T0 + 1 of a chunk ci >= 1 (cf_seam_of_row)"""
    x = min(t + 2, FRAMES - 1)
    ci = ((x + 1) * chunks - 1) // FRAMES
    t0 = chunk_t0(ci, chunks)
    return (ci, t - (t0 - 2)) if ci >= 1 and t0 >= t - 1 else None


def term_index(r, dt):
    return r * (r + 1) // 2 + dt - (4 - r)


@pytest.mark.parametrize("chunks", [4, 8, 16, 32])
def test_frame_direction(chunks):
    """the march's rows: c1 row t adds tap d to output row t + 2 - d, into a finished row, a prefix or a single term"""
    bounds = [chunk_t0(ci, chunks) for ci in range(chunks + 1)]
    assert bounds[0] == 0 and bounds[-1] == FRAMES and min(b - a for a, b in zip(bounds, bounds[1:])) >= 5
    for ci in range(chunks):  # cf_chunk_of inverts cf_chunk_t0
        for x in range(bounds[ci], bounds[ci + 1]):
            assert ((x + 1) * chunks - 1) // FRAMES == ci
    rec = {}  # record -> the taps added into it, in the order of the additions
    for ci in range(chunks):
        t0, t1 = bounds[ci], bounds[ci + 1]
        for t in range(t0, t1):
            k = t - t0
            for d in range(5):  # the chain a_d = a_(d - 1) + P_d: one more tap on the row that had d before
                row = t + 2 - d
                if ci > 0 and d > k:  # the chunk's head: the tap of a seam row, stored alone
                    key = ("term", ci, k + 4 - d, d)
                    assert key not in rec and 0 <= term_index(k + 4 - d, d) < 10
                elif ci < chunks - 1 and row >= t1 - 2:  # still open at the chunk's end: a prefix of the next seam
                    key = ("pref", ci + 1, row - (t1 - 2))
                else:
                    key = ("main", row)
                rec.setdefault(key, []).append((d, t))
    # single terms have slots of their own
    terms = [k for k in rec if k[0] == "term"]
    assert len({(k[1], term_index(k[2], k[3])) for k in terms}) == len(terms) == 10 * (chunks - 1)
    for t in range(-2, FRAMES + 2):  # the reader
        s = seam_of_row(t, chunks) if 0 <= t < FRAMES else None
        if s:
            ci, r = s
            assert 0 <= r <= 3 and t == bounds[ci] - 2 + r
            got = rec.pop(("pref", ci, r)) + [x for d in range(4 - r, 5) for x in rec.pop(("term", ci, r, d))]
        else:
            got = rec.pop(("main", t), [])
        if not 0 <= t < FRAMES:
            continue  # rows outside the window are never stored (the march skips them) nor read
        want = [(d, t + d - 2) for d in range(5) if 0 <= t + d - 2 < FRAMES]
        assert got == want, (chunks, t, got)  # every tap once, dt ascending
    assert not rec


def test_bin_direction():
    """the march's columns and the finisher's lanes: every (input bin, frequency tap) of an output bin exactly once"""
    cols = {}  # (strip, column of a finished row) -> [(class, input bin, df)] in the order the classes are added
    cls = {}
    for s in range(STRIPS):
        for n in range(16):
            for j in range(2):
                for df in range(5):
                    ob = j - df + 2  # output bin relative to bin 2 p of the position
                    e = ob % 2
                    c = (ob - e) // 2 + 1  # ob = e - 2, e, e + 2: classes 0, 1, 2
                    assert c in (0, 1, 2)
                    cls.setdefault((s, c, 2 * n + e), []).append((20 + 32 * s + 2 * n + j, df))
    for s in range(STRIPS):
        for col in range(32):
            parts = [(2, col - 2), (1, col), (0, col + 2)]  # (left + own) + right
            cols[(s, col)] = [x for c, el in parts if 0 <= el < 32 for x in cls[(s, c, el)]]
        for e in range(2):
            cols[(s, 32 + e)] = list(cls[(s, 0, e)])        # in front of the strip: class 0 of position 0
            cols[(s, 34 + e)] = list(cls[(s, 2, 30 + e)])   # behind it: class 2 of position 15
    used = set()

    def take(s, col):
        assert (s, col) not in used
        used.add((s, col))
        return cols[(s, col)]

    for f in range(BINS):
        got = []
        if 24 <= f < 240:  # lanes 0 .. 53, four bins each
            s, col = (f - 20) >> 5, (f - 20) & 31
            got += take(s, col)
            if col < 2 and s >= 1:
                got += take(s - 1, 34 + col)
            if col >= 30 and s <= 5:
                got += take(s + 1, 32 + col - 30)
        elif 18 <= f < 24:  # the rim lanes' share of the march's sums
            got += take(0, f - 20) if f >= 20 else take(0, f + 14)
        elif 240 <= f < 246:
            got += take(6, f - 212) if f <= 243 else take(6, f - 210)
        want = sorted((fi, fi - f + 2) for fi in range(20, 244) if 0 <= fi - f + 2 <= 4)
        assert sorted(got) == want, (f, got)
    assert used == set(cols)  # nothing the march stores is left unread
    # the rim's own pixels (bins 0 .. 19, 244 .. 263) reach bins 0 .. 21 and 242 .. 263 only: inside the 24 + 24 rim lanes,
    # whose tiles (padded columns 0 .. 31, 236 .. 267) hold every neighbour they read
    for f in range(BINS):
        reached = any(0 <= f + df - 2 < 20 or 244 <= f + df - 2 < BINS for df in range(5))
        assert reached == (f < 22 or f >= 242)
        if f < 24 or f >= 240:
            lane = f + 2 if f < 24 else f - 234  # the bin's lane in its tile
            assert 0 <= lane - 2 and lane + 2 <= 31
