"""Timings of chords and key on the device (bp_chords_from_maps, include/basic_pitch_amd_chord.h) against the only route
without it; the numbers of profiles/chord.md.

    python tools/bench_chord.py --out chord.json    both routes of the jobs; REPS repetitions each after one that is not timed
    python tools/bench_chord.py --one-call          ONE device call per job and nothing else timed (for a kernel trace)

Jobs, all with the note map held in device memory: 512 one-window segments (142 rows each), 64 four-window segments (568 rows
each) and one track of 110 windows (15,620 rows, one segment), in frame units; and the 512 segments once more with the beats
of bp_beats_from_maps on a synthetic onset map (a beat every 43 frames) as boundaries.  The note maps are synthetic: uniform
noise below 0.25 and a triad of the majmin table in two octaves at 0.6 ... 1.0 that changes every 86 frames.  Default
parameters.  Routes, each the native call alone with every argument and buffer made before:
  a   bp_chords_from_maps
  h   the note map copied home (one device-to-host copy into pageable memory, as a caller without this call would), then
      bp_chord_rows per segment on one host thread — the only route of the parent commit (there in numpy)
Before anything is timed the summaries and labels of a are compared with those of h (equal bytes).  A repetition runs the
routes one after the other in an order that rotates; a route's figure is the median of its repetitions, with their range; host
clock around calls that return after the stream has been waited for.  After the last a the path kernel's own clock readings
(100 MHz, bp_internal_chord_clocks) give, as medians over the job's segments, the time to pick the key and load the table, the
recurrence, the time per unit, and the backtrace."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPS = 9
PERIOD = 43


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def repeat(routes):
    names = list(routes)
    for r in names:  # not timed: first launches, first growth of the buffers
        routes[r]()
    samples = {r: [] for r in names}
    for k in range(REPS):
        for r in names[k % len(names):] + names[:k % len(names)]:
            samples[r].append(timed(routes[r]))
    return samples


def summarise(samples):
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3)}


def synthetic_note(rows, rng):
    m = rng.uniform(0.0, 0.25, (rows, 88)).astype(np.float32)
    classes = (np.arange(88) + 9) % 12
    for t in range(0, rows, 2 * PERIOD):
        root, third = int(rng.integers(0, 12)), int(rng.choice([3, 4]))
        tones = np.isin(classes, [(root + d) % 12 for d in (0, third, 7)]) & (np.arange(88) >= 27) & (np.arange(88) < 51)
        m[t : t + 2 * PERIOD, tones] = np.float32(rng.uniform(0.6, 1.0))
    return m


def synthetic_onset(rows, rng):
    m = rng.uniform(0.0, 0.25, (rows, 88)).astype(np.float32)
    for t in range(int(rng.integers(1, PERIOD)), rows, PERIOD):
        m[t, rng.choice(88, 3, replace=False)] = rng.uniform(0.6, 1.0, 3).astype(np.float32)
    return m


class Job:
    def __init__(self, model, name, seg_rows, with_beats=False):
        import torch

        from basic_pitch_amd import _native, beat as BT, chord as CH

        self.name, self.lib, self.h, self.n = name, CH.bind(model._lib), model._handle, len(seg_rows)
        self.lib.bp_internal_chord_clocks.restype = C.c_int
        self.lib.bp_internal_chord_clocks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        rng = np.random.default_rng(11)
        self.host = np.ascontiguousarray(np.concatenate([synthetic_note(r, rng) for r in seg_rows]), np.float32)
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.total = int(self.offs[-1])
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.home = np.empty_like(self.host)
        self.p64 = C.POINTER(C.c_int64)
        self.fixed = (self.h, self.n, self.offs.ctypes.data_as(self.p64), self.dev.data_ptr(), _native.BP_MEM_DEVICE)
        self.p = CH.chord_params()
        self.b_offs = self.bounds = None
        if with_beats:  # the beats of the device's own beat call on an onset map of the same rows
            onset = np.ascontiguousarray(np.concatenate([synthetic_onset(r, rng) for r in seg_rows]), np.float32)
            _, beats, offsets = BT.beats_from_maps(model, self.offs, onset.ctypes.data, _native.BP_MEM_HOST)
            parts = [beats[int(offsets[i]) : int(offsets[i + 1])] for i in range(self.n)]
            parts = [b[b != 0] for b in parts]  # a beat at frame 0 is no boundary
            self.b_offs = np.concatenate([[0], np.cumsum([len(b) for b in parts])]).astype(np.int64)
            self.bounds = np.ascontiguousarray(np.concatenate(parts), np.int32)
            assert len(self.bounds)
        self.units = int(self.total if self.bounds is None else len(self.bounds) + self.n)
        self.summaries, self.host_summaries = np.zeros(self.n, CH.CHORD_SUMMARY), np.zeros(self.n, CH.CHORD_SUMMARY)
        self.labels, self.host_labels = np.zeros(self.total, np.uint8), np.zeros(self.total, np.uint8)
        # the checks
        assert self.a() == 0 and not self.summaries["status"].any()
        self.h_route()
        assert self.summaries.tobytes() == self.host_summaries.tobytes(), "the device's summaries are not the checker's"
        assert self.labels.tobytes() == self.host_labels.tobytes(), "the device's labels are not the checker's"
        self.changes = int(self.summaries["n_changes"].sum())

    def a(self):
        return self.lib.bp_chords_from_maps(*self.fixed, C.addressof(self.p), self.b_offs.ctypes.data_as(self.p64) if self.b_offs is not None else None,
                                            self.bounds.ctypes.data if self.bounds is not None else None, self.summaries.ctypes.data,
                                            self.labels.ctypes.data, self.total)

    def h_route(self):
        import torch

        torch.from_numpy(self.home).copy_(self.dev)  # one device-to-host copy into pageable memory; returns when it has landed
        for i in range(self.n):
            r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
            b0, b1 = (int(self.b_offs[i]), int(self.b_offs[i + 1])) if self.b_offs is not None else (0, 0)
            rc = self.lib.bp_chord_rows(self.home.ctypes.data + r0 * 88 * 4, r1 - r0, C.addressof(self.p),
                                        self.bounds.ctypes.data + 4 * b0 if b1 > b0 else None, b1 - b0, self.host_labels.ctypes.data + r0, r1 - r0,
                                        self.host_summaries.ctypes.data + 32 * i)
            assert rc == 0

    def clocks(self):
        """Medians over the segments of the last device call, in us: (key and table, recurrence, per unit, backtrace)."""
        ticks = np.zeros(4, np.int64)
        pick, rec, unit, back = [], [], [], []
        for c in range(self.n):
            assert self.lib.bp_internal_chord_clocks(self.h, c, ticks.ctypes.data) == 0
            units = int(self.summaries["n_units"][c])
            pick.append((ticks[1] - ticks[0]) / 100.0), rec.append((ticks[2] - ticks[1]) / 100.0), back.append((ticks[3] - ticks[2]) / 100.0)
            unit.append(rec[-1] / units)
        med = lambda v: round(float(statistics.median(v)), 3)  # noqa: E731
        return {"key_us": med(pick), "recurrence_us": med(rec), "per_unit_us": med(unit), "backtrace_us": med(back),
                "backtrace_per_unit_us": med([b / int(self.summaries["n_units"][c]) for c, b in enumerate(back)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=8) as model:
        for name, seg_rows, with_beats in (("512 one-window segments", [142] * 512, False), ("64 four-window segments", [568] * 64, False),
                                           ("one 110-window track", [110 * 142], False), ("512 one-window segments, beat units", [142] * 512, True)):
            job = Job(model, name, seg_rows, with_beats)
            if args.one_call:
                assert job.a() == 0
                continue
            samples = repeat({"a": job.a, "h": job.h_route})
            assert job.a() == 0
            row = {"job": name, "rows": job.total, "segments": job.n, "units": job.units, "changes": job.changes,
                   **{r: summarise(v) for r, v in samples.items()}, **job.clocks()}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
