"""Timings of tempo and beats on the device (bp_beats_from_maps, include/basic_pitch_amd_beat.h) against the only route
without it; the numbers of profiles/beat.md.

    python tools/bench_beat.py --out beat.json     both routes of the three jobs; REPS repetitions each
    python tools/bench_beat.py --one-call          ONE device call per job and nothing else timed (for a kernel trace)

Jobs, all with the onset map held in device memory: 512 one-window segments (142 rows each), 64 four-window segments (568 rows
each) and one track of 110 windows (15,620 rows, one segment).  The maps are synthetic: uniform noise below 0.25, three pitches
of 0.6 ... 1.0 on a beat every 43 frames (120 a minute) that starts at a random phase per segment, and one distractor of 0.7 in
40 rows.  Default parameters.  Routes, each the native call alone with every argument and buffer made before:
  a   bp_beats_from_maps
  h   the onset map copied home (one device-to-host copy into pageable memory, as a caller without this call would), then
      bp_beat_rows per segment on one host thread — the only route of the parent commit (there in numpy)
Before anything is timed the summaries, offsets and beats of a are compared with those of h (equal bytes).  A repetition runs
the routes one after the other in an order that rotates; a route's figure is the median of its repetitions, with their range;
host clock around calls that return after the stream has been waited for.  After the last a the path kernel's own clock
readings (100 MHz, bp_internal_beat_clocks) give, as medians over the job's segments, the time to pick the period, the
recurrence, the time per block of dmin frames, and the ending with the backtrace.

The forms the path kernel is measured against are in the A/B library only (python -m basic_pitch_amd.build --ab, then
BASIC_PITCH_AMD_LIB=.../libbasicpitch_amd_ab.so with BP_BEAT_PATH=serial: frame by frame in one wave, or =walk: the
backtrace by one lane in global memory); --form labels the rows of such a run."""
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

REPS = 5
PERIOD = 43


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def repeat(routes):
    names = list(routes)
    samples = {r: [] for r in names}
    for k in range(REPS):
        for r in names[k % len(names):] + names[:k % len(names)]:
            samples[r].append(timed(routes[r]))
    return samples


def summarise(samples):
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3)}


def synthetic(rows, rng):
    m = rng.uniform(0.0, 0.25, (rows, 88)).astype(np.float32)
    for t in range(int(rng.integers(0, PERIOD)), rows, PERIOD):
        m[t, rng.choice(88, 3, replace=False)] = rng.uniform(0.6, 1.0, 3).astype(np.float32)
    for t in rng.choice(rows, max(1, rows // 40), replace=False):
        m[t, rng.integers(0, 88)] = np.float32(0.7)
    return m


class Job:
    def __init__(self, model, name, seg_rows):
        import torch

        from basic_pitch_amd import _native, beat as BT

        self.name, self.lib, self.h, self.n = name, BT.bind(model._lib), model._handle, len(seg_rows)
        self.lib.bp_internal_beat_clocks.restype = C.c_int
        self.lib.bp_internal_beat_clocks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        rng = np.random.default_rng(11)
        self.host = np.ascontiguousarray(np.concatenate([synthetic(r, rng) for r in seg_rows]), np.float32)
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.total = int(self.offs[-1])
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.home = np.empty_like(self.host)
        self.p64 = C.POINTER(C.c_int64)
        self.fixed = (self.h, self.n, self.offs.ctypes.data_as(self.p64), self.dev.data_ptr(), _native.BP_MEM_DEVICE)
        self.p = BT.beat_params()
        self.caps = [BT.beats_capacity(r, self.p.lag_min) for r in seg_rows]
        self.room = sum(self.caps)
        self.summaries, self.host_summaries = np.zeros(self.n, BT.BEAT_SUMMARY), np.zeros(self.n, BT.BEAT_SUMMARY)
        self.beats, self.host_beats = np.zeros(self.room, np.int32), np.zeros(self.room, np.int32)
        self.offsets, self.host_offsets = np.zeros(self.n + 1, np.int64), np.zeros(self.n + 1, np.int64)
        # the checks
        assert self.a() == 0 and not self.summaries["status"].any()
        self.h_route()
        n = int(self.offsets[-1])
        assert self.summaries.tobytes() == self.host_summaries.tobytes(), "the device's summaries are not the checker's"
        assert self.offsets.tobytes() == self.host_offsets.tobytes() and self.beats[:n].tobytes() == self.host_beats[:n].tobytes()
        self.n_beats = n
        self.periods = sorted(set(self.summaries["period"].tolist()))

    def a(self):
        return self.lib.bp_beats_from_maps(*self.fixed, C.addressof(self.p), self.summaries.ctypes.data, self.beats.ctypes.data, self.room,
                                           self.offsets.ctypes.data_as(self.p64))

    def h_route(self):
        import torch

        torch.from_numpy(self.home).copy_(self.dev)  # one device-to-host copy into pageable memory; returns when it has landed
        at = 0
        for i in range(self.n):
            r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
            rc = self.lib.bp_beat_rows(self.home.ctypes.data + r0 * 88 * 4, r1 - r0, C.addressof(self.p), self.host_beats.ctypes.data + 4 * at,
                                       self.caps[i], self.host_summaries.ctypes.data + 32 * i)
            assert rc == 0
            self.host_offsets[i] = at
            at += int(self.host_summaries["n_beats"][i])
        self.host_offsets[self.n] = at

    def clocks(self):
        """Medians over the segments of the last device call, in us: (period picked, recurrence, per block of frames, ending
        and backtrace)."""
        ticks = np.zeros(4, np.int64)
        pick, rec, block, back = [], [], [], []
        for c in range(self.n):
            assert self.lib.bp_internal_beat_clocks(self.h, c, ticks.ctypes.data) == 0
            rows, dmin = int(self.offs[c + 1] - self.offs[c]), max(1, int(self.summaries["period"][c]) // 2)
            pick.append((ticks[1] - ticks[0]) / 100.0), rec.append((ticks[2] - ticks[1]) / 100.0), back.append((ticks[3] - ticks[2]) / 100.0)
            block.append(rec[-1] / -(-rows // dmin))
        med = lambda v: round(float(statistics.median(v)), 3)  # noqa: E731
        return {"pick_us": med(pick), "recurrence_us": med(rec), "per_block_us": med(block), "ending_backtrace_us": med(back)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--form", default="product")
    args = ap.parse_args()
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=8) as model:
        for name, seg_rows in (("512 one-window segments", [142] * 512), ("64 four-window segments", [568] * 64),
                               ("one 110-window track", [110 * 142])):
            job = Job(model, name, seg_rows)
            if args.one_call:
                assert job.a() == 0
                continue
            samples = repeat({"a": job.a, "h": job.h_route})
            assert job.a() == 0
            row = {"form": args.form, "job": name, "rows": job.total, "segments": job.n, "beats": job.n_beats, "periods": job.periods,
                   **{r: summarise(v) for r, v in samples.items()}, **job.clocks()}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
