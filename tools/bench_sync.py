"""Timings of the synchronisation of two recordings on the device (bp_sync_from_maps, include/basic_pitch_amd_sync.h) against
the only route without it; the numbers of profiles/sync.md.

    python tools/bench_sync.py --out sync.json     both routes of the jobs; REPS repetitions each after one that is not timed
    python tools/bench_sync.py --one-call          ONE device call per job and nothing else timed (for a kernel trace)

Jobs, all with the note map held in device memory: 512 pairs of one-window segments (142 rows each: 36 x 36 units at the
default hop), 64 pairs of four-window segments (568 rows: 142 x 142 units), one pair of 110-window tracks (15,620 rows) at hop 4
(3,905 x 3,905 units) and at hop 2 (7,810 x 7,810), and one one-window reference segment against 255 others.  The note maps are
synthetic: uniform noise below 0.25 and a triad in two octaves at 0.6 ... 1.0 that changes every 86 frames; the second segment
of a pair is the first played unevenly — its rows repeated or dropped by a seeded warp — under noise of its own.  Default
parameters but for hop.  Routes, each the native call alone with every argument and buffer made before:
  a   bp_sync_from_maps
  h   the note map copied home (one device-to-host copy into pageable memory, as a caller without this call would), then
      bp_sync_rows per pair on one host thread — the only route of the parent commit (there in numpy)
Before anything is timed the summaries and paths of a are compared with those of h (equal bytes).  A repetition runs the routes
one after the other in an order that rotates; a route's figure is the median of its repetitions, with their range; host clock
around calls that return after the stream has been waited for."""
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
    m = np.zeros((rows, 88), np.float32)
    classes = (np.arange(88) + 9) % 12
    for t in range(0, rows, 2 * PERIOD):
        root, third = int(rng.integers(0, 12)), int(rng.choice([3, 4]))
        tones = np.isin(classes, [(root + d) % 12 for d in (0, third, 7)]) & (np.arange(88) >= 27) & (np.arange(88) < 51)
        m[t : t + 2 * PERIOD, tones] = np.float32(rng.uniform(0.6, 1.0))
    return m


def another_take(note, rng):
    """The same rows played unevenly: every row once, twice or not at all (cut or padded to the same length), noise of its own."""
    times = rng.choice([0, 1, 1, 1, 2], len(note))
    rows = np.repeat(np.arange(len(note)), times)
    rows = np.concatenate([rows, np.full(max(0, len(note) - len(rows)), len(note) - 1)])[: len(note)]
    return note[rows]


def noisy(note, rng):
    return np.maximum(note, rng.uniform(0.0, 0.25, note.shape).astype(np.float32))


class Job:
    def __init__(self, model, name, seg_rows, pairs, hop):
        import torch

        from basic_pitch_amd import _native, sync as SY

        self.name, self.lib, self.h, self.n, self.pairs = name, SY.bind(model._lib), model._handle, len(seg_rows), pairs
        rng = np.random.default_rng(11)
        maps = []
        for i, r in enumerate(seg_rows):  # a pair's second segment is another take of its first; a lone segment is its own piece
            first = [a for a, b in pairs if b == i and a != i]
            maps.append(another_take(maps[first[0]][1], rng) if first and len(maps[first[0]][1]) == r else synthetic_note(r, rng))
            maps[-1] = (noisy(maps[-1], rng), maps[-1])
        self.host = np.ascontiguousarray(np.concatenate([m[0] for m in maps]), np.float32)
        self.offs = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.home = np.empty_like(self.host)
        self.p64 = C.POINTER(C.c_int64)
        self.fixed = (self.h, self.n, self.offs.ctypes.data_as(self.p64), self.dev.data_ptr(), _native.BP_MEM_DEVICE)
        self.p = SY.sync_params(hop=hop)
        self.tab = SY.pair_table(pairs)
        self.room = SY.path_room(seg_rows, self.tab, hop)
        units = SY.units_of(seg_rows, hop)
        self.cells = int(sum(int(units[a]) * int(units[b]) for a, b in pairs))
        self.units = (int(units[pairs[0][0]]), int(units[pairs[0][1]]))
        self.summaries, self.host_summaries = np.zeros(len(pairs), SY.SYNC_SUMMARY), np.zeros(len(pairs), SY.SYNC_SUMMARY)
        self.path, self.host_path = np.zeros((self.room, 2), np.int32), np.zeros((self.room, 2), np.int32)
        # the checks
        assert self.a() == 0 and not self.summaries["status"].any()
        self.h_route()
        self.host_summaries["path_first"] = self.summaries["path_first"]  # (the checker counts a pair's region from 0)
        assert self.summaries.tobytes() == self.host_summaries.tobytes(), "the device's summaries are not the checker's"
        assert self.path.tobytes() == self.host_path.tobytes(), "the device's paths are not the checker's"
        self.steps = int(self.summaries["n_path"].sum())
        diag = sum(int(np.sum(np.diff(self.path[int(s["path_first"]) : int(s["path_first"]) + int(s["n_path"])], axis=0).sum(axis=1) == 2))
                   for s in self.summaries)
        self.diagonal_share = round(diag / max(1, self.steps), 3)

    def a(self):
        return self.lib.bp_sync_from_maps(*self.fixed, len(self.pairs), self.tab.ctypes.data, C.addressof(self.p), self.summaries.ctypes.data,
                                          self.path.ctypes.data, self.room)

    def h_route(self):
        import torch

        torch.from_numpy(self.home).copy_(self.dev)  # one device-to-host copy into pageable memory; returns when it has landed
        first = 0
        for k, (a, b) in enumerate(self.pairs):
            a0, a1, b0, b1 = int(self.offs[a]), int(self.offs[a + 1]), int(self.offs[b]), int(self.offs[b + 1])
            room = int(self.summaries["units_a"][k] + self.summaries["units_b"][k] - 1)
            rc = self.lib.bp_sync_rows(self.home.ctypes.data + a0 * 88 * 4, a1 - a0, self.home.ctypes.data + b0 * 88 * 4, b1 - b0,
                                       C.addressof(self.p), self.host_path.ctypes.data + 8 * first, room, self.host_summaries.ctypes.data + 32 * k)
            assert rc == 0
            first += room


def jobs():
    one, four, track = 142, 568, 110 * 142
    yield "512 pairs of one-window segments", [one] * 1024, [(2 * i, 2 * i + 1) for i in range(512)], 4
    yield "64 pairs of four-window segments", [four] * 128, [(2 * i, 2 * i + 1) for i in range(64)], 4
    yield "one pair of 110-window tracks, hop 4", [track] * 2, [(0, 1)], 4
    yield "one pair of 110-window tracks, hop 2", [track] * 2, [(0, 1)], 2
    yield "one one-window segment against 255 others", [one] * 256, [(0, i) for i in range(1, 256)], 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=8) as model:
        for name, seg_rows, pairs, hop in jobs():
            job = Job(model, name, seg_rows, pairs, hop)
            if args.one_call:
                assert job.a() == 0
                continue
            samples = repeat({"a": job.a, "h": job.h_route})
            row = {"job": name, "rows": int(job.offs[-1]), "segments": job.n, "pairs": len(pairs), "hop": hop, "units": list(job.units),
                   "cells": job.cells, "path_steps": job.steps, "diagonal_share": job.diagonal_share, **{r: summarise(v) for r, v in samples.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
