"""Timings of multi-pitch estimates on the device (bp_multipitch_from_maps, bp_multipitch_sweep_frame_score,
include/basic_pitch_amd_multipitch.h) against the only routes without them; the numbers of profiles/multipitch.md.

    python tools/bench_multipitch.py --out multipitch.json     every route of both jobs; REPS repetitions each
    python tools/bench_multipitch.py --one-call                ONE points call and ONE sweep call per job and nothing else timed (for a kernel trace)

Jobs, both with the contour map held in device memory: 512 one-window segments (142 rows each) and one track of 110 windows
(15,620 rows, one segment); the maps are tools/bench_note_sweep.py's synthetic ones (noise below 0.2 with ridges of +0.6 three
bins wide).  The sweep is over 64 thresholds 0.05 ... 0.68 on all bins; a segment's refs are made from its own points under
the default set (a third on a peak, a third 0.7 semitones above one, a third where nothing is), eight per window.  Routes, each
the native call alone with every argument and buffer made before:
  a   bp_multipitch_from_maps, default set, room for exactly the points
  h   the contour map copied home (one hipMemcpy into pageable memory, as a caller without this call would), then
      bp_multipitch_rows per segment on one host thread — the only route of the parent commit
  s   bp_multipitch_sweep_frame_score under the 64 sets
  t   64 x (bp_multipitch_from_maps, then bp_score_f0_frames per segment on one host thread)
Before anything is timed the points of a are compared with those of h (equal bytes) and the counts of s with those of t (equal
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

        from basic_pitch_amd import _native, multipitch as MP, score
        from bench_note_sweep import synthetic

        self.name, self.lib, self.h, self.n = name, MP.bind(score.bind(model._lib)), model._handle, len(seg_rows)
        rng = np.random.default_rng(11)
        self.host = np.ascontiguousarray(np.concatenate([synthetic(r, rng)["contour"] for r in seg_rows]), np.float32)
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.home = np.empty_like(self.host)
        self.p64 = C.POINTER(C.c_int64)
        self.fixed = (self.h, self.n, self.offs.ctypes.data_as(self.p64), self.dev.data_ptr(), _native.BP_MEM_DEVICE)
        self.p = MP.mp_params()
        self.sets = MP.sets_array([dict(threshold=0.05 + 0.01 * k) for k in range(N_SETS)])
        self.p_offs, self.status = np.zeros(self.n + 1, np.int64), np.zeros(self.n, np.int32)
        # the room: the most points any set needs (the lowest threshold), asked for by a call without room
        self.points = None
        need = 0
        for k in (0, None):
            rc = self.lib.bp_multipitch_from_maps(*self.fixed, C.addressof(self.sets[k]) if k is not None else C.addressof(self.p), None, 0,
                                                  self.p_offs.ctypes.data_as(self.p64), self.status.ctypes.data)
            assert rc in (0, -1)
            need = max(need, int(self.p_offs[self.n]))
        self.room = need
        self.points = np.zeros(max(1, need), MP.F0_POINT)
        self.host_points = np.zeros(max(1, need), MP.F0_POINT)
        self.prm = score.score_params()
        assert self.a() == 0
        self.n_points = int(self.p_offs[self.n])
        # refs from the default set's points
        refs = []
        for i in range(self.n):
            pts = self.points[int(self.p_offs[i]) : int(self.p_offs[i + 1])]
            rows = int(seg_rows[i])
            mine = []
            for k in range(8 * max(1, rows // 142)):
                f0 = int(rng.integers(0, rows))
                on = pts[pts["frame"] == f0]
                pitch = float(on["pitch_midi"][int(rng.integers(0, len(on)))]) + (0.0, 0.7)[k % 3] if len(on) and k % 3 != 2 else 15.0
                mine.append((MP.frames_to_time_at([f0])[0], MP.frames_to_time_at([min(rows, f0 + int(rng.integers(5, 60)))])[0], pitch))
            refs.append(mine)
        self.ref_offs, self.refs = score.refs_table(refs)
        nd = N_SETS * self.n
        self.frames, self.dec_status = np.zeros((nd, 5), np.int64), np.zeros(nd, np.int32)
        self.host_frames = np.zeros((nd, 5), np.int64)
        # the checks
        self.h_route()
        assert self.host_points[: self.n_points].tobytes() == self.points[: self.n_points].tobytes(), "the device's points are not the checker's"
        assert self.s() == 0 and not self.dec_status.any()
        self.t()
        assert np.array_equal(self.frames, self.host_frames), "the device's counts are not the checker's"
        self.sums = {k: int(v) for k, v in zip(("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub"), self.frames.sum(axis=0))}

    def a(self, p=None, points=None):
        return self.lib.bp_multipitch_from_maps(*self.fixed, C.addressof(p if p is not None else self.p),
                                                (points if points is not None else self.points).ctypes.data, self.room,
                                                self.p_offs.ctypes.data_as(self.p64), self.status.ctypes.data)

    def h_route(self):
        import torch

        torch.from_numpy(self.home).copy_(self.dev)  # one device-to-host copy into pageable memory; returns when it has landed
        n, st = C.c_int64(0), C.c_int(0)
        done = 0
        for i in range(self.n):
            r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
            rc = self.lib.bp_multipitch_rows(self.home.ctypes.data + r0 * 264 * 4, r1 - r0, C.addressof(self.p),
                                             self.host_points.ctypes.data + 16 * done, self.room - done, C.byref(n), C.byref(st))
            assert rc == 0
            done += n.value

    def s(self):
        return self.lib.bp_multipitch_sweep_frame_score(*self.fixed, N_SETS, C.addressof(self.sets), N_SETS * self.n, None,
                                                        self.ref_offs.ctypes.data_as(self.p64), self.refs.ctypes.data, C.addressof(self.prm),
                                                        self.frames.ctypes.data, self.dec_status.ctypes.data)

    def t(self):
        for k in range(N_SETS):
            assert self.a(self.sets[k], self.host_points) == 0
            for i in range(self.n):
                e0, e1, r0, r1 = int(self.p_offs[i]), int(self.p_offs[i + 1]), int(self.ref_offs[i]), int(self.ref_offs[i + 1])
                rc = self.lib.bp_score_f0_frames(self.host_points.ctypes.data + 16 * e0, e1 - e0, self.refs.ctypes.data + 24 * r0, r1 - r0,
                                                 int(self.offs[i + 1] - self.offs[i]), C.addressof(self.prm),
                                                 self.host_frames.ctypes.data + 40 * (k * self.n + i))
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
            row = {"job": name, "rows": int(job.offs[-1]), "segments": job.n, "points": job.n_points, "sets": N_SETS,
                   "decodes": N_SETS * job.n, "refs": int(job.ref_offs[-1]), **job.sums, **{r: summarise(v) for r, v in samples.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
