"""Timings of forced alignment on the device (bp_align_from_maps, include/basic_pitch_amd_align.h) against the only route
without it; the numbers of profiles/align.md.

    python tools/bench_align.py --out align.json     both routes of every job; REPS repetitions each
    python tools/bench_align.py --one-call           ONE device call per job and nothing else timed (for a kernel trace)

Jobs, all with the note and onset maps held in device memory: 512 one-window segments (142 rows each) of 8 states, 64
four-window segments (568 rows) of 64 states, and one track of 110 windows (15,620 rows, one segment) at 1,024 and at
BP_ALIGN_MAX_STATES states.  The maps are planted: a random list of chord states (notes start, end and are struck again), cut
points spread evenly and jittered, 0.8 on what sounds and on what begins where it begins, 0.1 elsewhere, +-0.05 of noise.
Routes, each the native call alone with every argument and buffer made before:
  a   bp_align_from_maps, default parameters
  h   the two maps copied home (one hipMemcpy each into pageable memory, as a caller without this call would), then
      bp_align_rows per segment on one host thread — the only route of the parent commit
Before anything is timed the first frames, totals and statuses of a are compared with those of h (equal bytes), and the first
frames with the planted ones.  A repetition runs the routes one after the other in an order that rotates; a route's figure is
the median of its repetitions, with their range; host clock around calls that return after the stream has been waited for."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REPS = 5


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


def planted(rng, rows, S, state_dtype):
    """(note, onset, states, first_frame) of one segment."""
    sounding, active, begins = set(), [], []
    for _ in range(S):
        while True:
            now, beg = set(sounding), set()
            for p in list(now):
                r = rng.integers(0, 6)
                if r == 0:
                    now.discard(p)
                elif r == 1:
                    beg.add(p)
            for p in rng.choice(88, int(rng.integers(0, 3)), replace=False).tolist():
                if p not in now:
                    now.add(p)
                    beg.add(p)
            if not active or now != sounding or beg:
                break
        sounding = now
        active.append(sorted(now))
        begins.append(sorted(beg))
    f = np.zeros(S, np.int64)
    if S > 1:
        even = np.arange(1, S) * rows // S
        slack = max(0, rows // S // 2 - 1)
        f[1:] = even + (rng.integers(-slack, slack + 1, S - 1) if slack else 0)
        assert np.all(np.diff(f) > 0)
    note, onset = np.full((rows, 88), 0.1), np.full((rows, 88), 0.1)
    states = np.zeros(S, state_dtype)
    states["latest"] = 2**31 - 1
    ends = np.concatenate([f[1:], [rows]])
    for j in range(S):
        note[f[j]:ends[j], active[j]] = 0.8
        onset[f[j], begins[j]] = 0.8
        for field, pitches in (("active", active[j]), ("begins", begins[j])):
            for p in pitches:
                states[field][j, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    note += rng.uniform(-0.05, 0.05, note.shape)
    onset += rng.uniform(-0.05, 0.05, onset.shape)
    return note.astype(np.float32), onset.astype(np.float32), states, f.astype(np.int32)


class Job:
    def __init__(self, model, name, seg_rows, S):
        import torch

        from basic_pitch_amd import _native, align as AL

        self.name, self.lib, self.h, self.n, self.S = name, AL.bind(model._lib), model._handle, len(seg_rows), S
        rng = np.random.default_rng(11)
        parts = [planted(rng, r, S, AL.ALIGN_STATE) for r in seg_rows]
        self.note = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
        self.onset = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
        self.states = np.ascontiguousarray(np.concatenate([p[2] for p in parts]))
        self.planted = np.concatenate([p[3] for p in parts])
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.s_offs = (np.arange(self.n + 1) * S).astype(np.int64)
        self.total = int(self.offs[-1])
        self.d_note, self.d_onset = torch.from_numpy(self.note).cuda(), torch.from_numpy(self.onset).cuda()
        torch.cuda.synchronize()
        self.home = (np.empty_like(self.note), np.empty_like(self.onset))
        p64 = C.POINTER(C.c_int64)
        self.p = AL.align_params()
        self.ff, self.tot, self.status = np.zeros(self.n * S, np.int32), np.zeros(self.n, np.int64), np.zeros(self.n, np.int32)
        self.h_ff, self.h_tot, self.h_status = np.zeros_like(self.ff), np.zeros_like(self.tot), np.zeros_like(self.status)
        self.args = (self.h, self.n, self.offs.ctypes.data_as(p64), self.d_note.data_ptr(), self.d_onset.data_ptr(), _native.BP_MEM_DEVICE,
                     self.s_offs.ctypes.data_as(p64), self.states.ctypes.data, C.addressof(self.p), self.ff.ctypes.data, self.n * S,
                     self.tot.ctypes.data_as(p64), self.status.ctypes.data)
        assert self.a() == 0 and not self.status.any()
        self.h_route()
        assert self.h_ff.tobytes() == self.ff.tobytes() and self.h_tot.tobytes() == self.tot.tobytes() and not self.h_status.any(), \
            "the device's alignment is not the checker's"
        self.recovered = int((self.ff == self.planted).sum())

    def a(self):
        return self.lib.bp_align_from_maps(*self.args)

    def h_route(self):
        import torch

        torch.from_numpy(self.home[0]).copy_(self.d_note)  # a device-to-host copy into pageable memory; returns when it has landed
        torch.from_numpy(self.home[1]).copy_(self.d_onset)
        st, tot = C.c_int(0), C.c_int64(0)
        for i in range(self.n):
            r0, r1 = int(self.offs[i]), int(self.offs[i + 1])
            rc = self.lib.bp_align_rows(self.home[0].ctypes.data + r0 * 352, self.home[1].ctypes.data + r0 * 352, r1 - r0,
                                        self.states.ctypes.data + 40 * i * self.S, self.S, C.addressof(self.p),
                                        self.h_ff.ctypes.data + 4 * i * self.S, self.S, C.byref(tot), C.byref(st))
            assert rc == 0
            self.h_tot[i], self.h_status[i] = tot.value, st.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd import align as AL
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=8) as model:
        for name, seg_rows, S in (("512 one-window segments of 8 states", [142] * 512, 8),
                                  ("64 four-window segments of 64 states", [568] * 64, 64),
                                  ("one 110-window track, 1024 states", [110 * 142], 1024),
                                  (f"one 110-window track, {AL.MAX_STATES} states", [110 * 142], AL.MAX_STATES)):
            job = Job(model, name, seg_rows, S)
            if args.one_call:
                assert job.a() == 0
                continue
            samples = repeat({"a": job.a, "h": job.h_route})
            row = {"job": name, "rows": job.total, "segments": job.n, "states": job.n * S, "cells": job.total * S,
                   "planted_recovered": job.recovered, **{r: summarise(v) for r, v in samples.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
