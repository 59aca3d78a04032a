"""Stamps of EVERY wave of one B = 256 launch of the three wave-private marches (contour conv1, note, onset).

Build the tool library with the stamps and the A/B switches, then run this file once per rule:

    tools/build_all_variant.sh prof -DBP_MARCH_PROF -DBP_AB_KERNELS
    BASIC_PITCH_AMD_LIB=basic_pitch_amd/lib/var_prof.so BP_MARCH_PRIO=off python tools/experiments/march_prof.py [OUT.npz]

The kernels write (csrc/march_common.h, BP_MARCH_PROF_*) per wave: entry, set-up done, end of each piece, exit (100 MHz
ticks), rows marched, XCC_ID and HW_ID.  Printed, as markdown: the distributions of µs per row and of the end time (from the
launch's first entry) per half of the grid and per XCD, and what the two waves that share a SIMD do to each other."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from basic_pitch_amd import _native, inference

STEPS = int(os.environ.get("MARCH_PROF_STEPS", "40"))  # back-to-back steps before the stamped one: sustained clocks


def fetch(lib, name):
    buf = np.zeros(2048 * 8, dtype=np.uint64)
    fn = getattr(lib, "bp_prof_%s_read" % name)
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    assert fn(buf.ctypes.data) == 0, name
    return buf.reshape(2048, 8)


def dist(v):
    q = np.percentile(v, [0, 5, 50, 95, 100])
    return "%.3f | %.3f | %.3f | %.3f | %.3f" % tuple(q)


def report(name, rec):
    meta = rec[:, 7]
    rows = (meta & np.uint64(0xFFFF)).astype(np.int64)
    pieces = ((meta >> np.uint64(16)) & np.uint64(15)).astype(np.int64)
    xcc = ((meta >> np.uint64(20)) & np.uint64(15)).astype(np.int64)
    hw = (meta >> np.uint64(32)).astype(np.int64)
    block = np.arange(2048) // 4
    half = (block >= 256).astype(np.int64)
    t0 = rec[:, 0].astype(np.int64).min()
    us = lambda col: (rec[:, col].astype(np.int64) - t0) / 100.0
    entry, setup, end = us(0), us(1), us(6)
    last = np.zeros(2048)
    for i in range(2048):
        last[i] = (int(rec[i, 1 + max(int(pieces[i]), 1)]) - t0) / 100.0 if pieces[i] else setup[i]
    work = rows > 0
    per_row = np.where(work, (last - setup) / np.maximum(rows, 1), np.nan)
    print("\n### `%s`: %d waves with rows, launch %.1f µs from the first entry to the last exit\n" % (name, int(work.sum()), end.max()))
    print("| waves | n | rows (mean) | µs / row: min | p5 | median | p95 | max | end µs: min | p5 | median | p95 | max |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    groups = [("first half", work & (half == 0)), ("second half", work & (half == 1))]
    groups += [("XCD %d" % x, work & (xcc == x)) for x in sorted(set(xcc[work]))]
    groups += [("XCD %d, %s half" % (x, "first" if h == 0 else "second"), work & (xcc == x) & (half == h))
               for x in sorted(set(xcc[work])) for h in (0, 1)]
    for label, m in groups:
        if m.any():
            print("| %s | %d | %.1f | %s | %s |" % (label, int(m.sum()), rows[m].mean(), dist(per_row[m]), dist(end[m])))
    print("\nentry µs (min | p5 | median | p95 | max): first half %s; second half %s" % (dist(entry[half == 0]), dist(entry[half == 1])))
    # the two waves of a SIMD: same XCC, shader engine / array, CU and SIMD (HW_ID bits 15:8 and 5:4)
    key = xcc * 65536 + (hw & 0xFF00) + ((hw >> 4) & 3)
    pairs = {}
    for i in np.nonzero(work)[0]:
        pairs.setdefault(int(key[i]), []).append(i)
    both = [p for p in pairs.values() if len(p) == 2 and half[p[0]] != half[p[1]]]
    print("\nSIMDs that hold exactly one wave of each half: %d of %d occupied" % (len(both), len(pairs)))
    if both:
        a = np.array([[p[0], p[1]] if half[p[0]] == 0 else [p[1], p[0]] for p in both])
        d_end = end[a[:, 1]] - end[a[:, 0]]
        d_rows = rows[a[:, 1]] - rows[a[:, 0]]
        print("second-half wave's end minus its SIMD partner's, µs (min | p5 | median | p95 | max): %s; it ends later on %d of %d SIMDs; "
              "rows, second minus first: mean %.2f" % (dist(d_end), int((d_end > 0).sum()), len(both), d_rows.mean()))
        solo = np.abs(d_end)
        print("time a SIMD runs with one wave left (|difference of the ends|), µs: %s; the SIMD's last exit: %s"
              % (dist(solo), dist(np.maximum(end[a[:, 0]], end[a[:, 1]]))))


def main():
    lib = _native.load_library()
    m = inference.Model(max_windows=256)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = (torch.rand(256, 43844, device="cuda", generator=g) * 2 - 1).float()
    for _ in range(STEPS):
        m.predict(x)
    torch.cuda.synchronize()
    recs = {k: fetch(lib, k) for k in ("contour", "note", "onset")}
    print("## rule: BP_MARCH_PRIO=%s, %d steps before the stamped one" % (os.environ.get("BP_MARCH_PRIO", "(adopted)"), STEPS))
    for k, r in recs.items():
        report(k, r)
    if len(sys.argv) > 1:
        np.savez(sys.argv[1], **recs)


if __name__ == "__main__":
    main()
