"""Timings of the melody decode on the device (bp_melody_from_maps, bp_melody_sweep_score, include/basic_pitch_amd_melody.h)
against the only routes without them; the numbers of profiles/melody.md.

    python tools/bench_melody.py --out melody.json     every route of both jobs; REPS repetitions each
    python tools/bench_melody.py --one-call            ONE records call and ONE sweep call per job and nothing else timed (for a kernel trace)

Jobs, both with the contour map held in device memory: 512 one-window segments (142 rows each) and one track of 110 windows
(15,620 rows, one segment); the maps are tools/bench_note_sweep.py's synthetic ones (noise below 0.2 with ridges of +0.6 three
bins wide).  The sweep is over 64 sets, thresholds 0.10 ... 0.73 with the other fields at their defaults; a segment's reference
track follows its own records under the default set, with an octave error, a half-semitone error or flipped voicing on three
frames in ten.  Routes, each the native call alone with every argument and buffer made before:
  a   bp_melody_from_maps, default set
  h   the contour map copied home (one hipMemcpy into pageable memory, as a caller without this call would), then
      bp_melody_rows per segment on one host thread — the only route of the parent commit
  s   bp_melody_sweep_score under the 64 sets
  t   64 x (bp_melody_from_maps, then bp_score_melody_frames per segment on one host thread)
Before anything is timed the records of a are compared with those of h (equal bytes) and the counts of s with those of t (equal
in every decode).  A repetition runs the routes one after the other in an order that rotates; a route's figure is the median of
its repetitions, with their range; host clock around calls that return after the stream has been waited for."""
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
N_SETS = 64
FIELDS = ("n_frames", "ref_voiced", "est_voiced", "both_voiced", "pitch_ok", "chroma_ok")


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


class Job:
    def __init__(self, model, name, seg_rows):
        import torch

        from basic_pitch_amd import _native, melody as ME, score
        from bench_note_sweep import synthetic

        self.name, self.lib, self.h, self.n = name, ME.bind(score.bind(model._lib)), model._handle, len(seg_rows)
        rng = np.random.default_rng(11)
        self.host = np.ascontiguousarray(np.concatenate([synthetic(r, rng)["contour"] for r in seg_rows]), np.float32)
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.total = int(self.offs[-1])
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.home = np.empty_like(self.host)
        self.p64 = C.POINTER(C.c_int64)
        self.fixed = (self.h, self.n, self.offs.ctypes.data_as(self.p64), self.dev.data_ptr(), _native.BP_MEM_DEVICE)
        self.p = ME.melody_params()
        self.sets = ME.sets_array([dict(threshold=0.10 + 0.01 * k) for k in range(N_SETS)])
        self.status = np.zeros(self.n, np.int32)
        self.points = np.zeros(self.total, ME.MELODY_POINT)
        self.host_points = np.zeros(self.total, ME.MELODY_POINT)
        self.prm = score.score_params()
        assert self.a() == 0 and not self.status.any()
        self.voiced = int((self.points["bin"] >= 0).sum())
        # the reference track from the default set's records
        ref = np.where(self.points["bin"] >= 0, self.points["pitch_midi"], 0.0).astype(np.float64)
        kind = rng.integers(0, 10, self.total)
        on = ref > 0
        ref[on & (kind == 1)] += 12.0
        ref[on & (kind == 2)] += 0.5
        ref[on & (kind == 3)] = 0.0
        ref[~on & (kind == 4)] = 60.0
        self.ref = ref
        nd = N_SETS * self.n
        self.scores, self.dec_status = np.zeros((nd, 6), np.int64), np.zeros(nd, np.int32)
        self.host_scores = np.zeros((nd, 6), np.int64)
        # the checks
        self.h_route()
        assert self.host_points.tobytes() == self.points.tobytes(), "the device's records are not the checker's"
        assert self.s() == 0 and not self.dec_status.any()
        self.t()
        assert np.array_equal(self.scores, self.host_scores), "the device's counts are not the checker's"
        self.sums = {k: int(v) for k, v in zip(FIELDS, self.scores.sum(axis=0))}

    def a(self, p=None, points=None):
        return self.lib.bp_melody_from_maps(*self.fixed, C.addressof(p if p is not None else self.p),
                                            (points if points is not None else self.points).ctypes.data, self.total, self.status.ctypes.data)

    def h_route(self):
        import torch

        torch.from_numpy(self.home).copy_(self.dev)  # one device-to-host copy into pageable memory; returns when it has landed
        st = C.c_int(0)
        for i in range(self.n):
            r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
            rc = self.lib.bp_melody_rows(self.home.ctypes.data + r0 * 264 * 4, r1 - r0, C.addressof(self.p),
                                         self.host_points.ctypes.data + 16 * r0, r1 - r0, C.byref(st))
            assert rc == 0

    def s(self):
        return self.lib.bp_melody_sweep_score(*self.fixed, N_SETS, C.addressof(self.sets), N_SETS * self.n, None, self.ref.ctypes.data,
                                              C.addressof(self.prm), self.scores.ctypes.data, self.dec_status.ctypes.data)

    def t(self):
        for k in range(N_SETS):
            assert self.a(self.sets[k], self.host_points) == 0
            for i in range(self.n):
                r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
                rc = self.lib.bp_score_melody_frames(self.host_points.ctypes.data + 16 * r0, self.ref.ctypes.data + 8 * r0, r1 - r0,
                                                     C.addressof(self.prm), self.host_scores.ctypes.data + 48 * (k * self.n + i))
                assert rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=8) as model:
        for name, seg_rows in (("512 one-window segments", [142] * 512), ("one 110-window track", [110 * 142])):
            job = Job(model, name, seg_rows)
            if args.one_call:
                assert job.a() == 0 and job.s() == 0
                continue
            samples = repeat({"a": job.a, "h": job.h_route, "s": job.s, "t": job.t})
            row = {"job": name, "rows": job.total, "segments": job.n, "voiced": job.voiced, "sets": N_SETS, "decodes": N_SETS * job.n,
                   **job.sums, **{r: summarise(v) for r, v in samples.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
