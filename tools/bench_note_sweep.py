"""Timings of a sweep of parameter sets (bp_note_events_sweep, include/basic_pitch_amd_sweep.h) against the loop of single-set
calls it replaces, and against decoding on host threads; the numbers of profiles/note_sweep.md.

    python tools/bench_note_sweep.py --out note_sweep.json          every workload, route and S; three repetitions each
    python tools/bench_note_sweep.py --one-sweep frame|onset [--S N]  ONE sweep at S = N (8) and nothing else (for a kernel trace)
    python tools/bench_note_sweep.py --one-single                   ONE bp_note_events_from_maps on the same segments (likewise)

Workloads: 512 one-window segments (142 rows) and 64 four-window segments (568 rows) held in device memory, and 512
one-window int16 clips in host memory.  Sets: S = 1, 8, 64 that differ in frame_threshold only (one dense key) or in
onset_threshold (S dense keys).  A repetition runs every device route once, one after the other and in an order that rotates
from repetition to repetition, so the routes share the box's state and none is always the one that follows the others; the
host-thread routes, which leave the device idle for a long time, have their repetitions after those.  A route's figure is
the median of its repetitions, with their range.  Every call returns after its stream has been
waited for: the host clock around a call is the call.  At S = 1 two more routes time the native call alone, with the sets, the
table and the output buffers made beforehand: what the Python binding adds is the difference to the routes above."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REPS = 3
SETS = (1, 8, 64)


def synthetic(T, rng):
    """Noise with note-like ridges, an onset at the start of most: a segment's posteriorgrams."""
    note = rng.uniform(0, 0.25, (T, 88)).astype(np.float32)
    onset = rng.uniform(0, 0.3, (T, 88)).astype(np.float32)
    contour = rng.uniform(0, 0.2, (T, 264)).astype(np.float32)
    for _ in range(max(1, T // 25)):
        f, t0, ln = int(rng.integers(0, 88)), int(rng.integers(0, max(1, T - 5))), int(rng.integers(3, 60))
        t1 = min(T, t0 + ln)
        note[t0:t1, f] = (rng.uniform(0.31, 0.95) + rng.normal(0, 0.03, t1 - t0)).clip(0, 1).astype(np.float32)
        if rng.random() < 0.7:
            onset[t0, f] = np.float32(rng.uniform(0.45, 0.99))
        contour[t0:t1, max(0, 3 * f - 1) : min(264, 3 * f + 2)] += np.float32(0.6)
    return {"note": note, "onset": onset, "contour": contour.clip(0, 1)}


def param_sets(kind, S):
    from basic_pitch_amd import note_creation as NC

    out = []
    for k in range(S):
        x = k / max(1, S - 1) if S > 1 else 0.5
        onset, frame = (0.5, 0.2 + 0.25 * x) if kind == "frame" else (0.3 + 0.4 * x, 0.3)
        out.append(NC._note_params(onset, frame, 11, True, None, None, True, NC.ENERGY_TOLERANCE, True))
    return out


class Job:
    """Segments in device memory, the output buffers of every route sized once, and the routes."""

    def __init__(self, model, segs):
        import torch

        from basic_pitch_amd import _native, events as EV, sweep as SW

        self.m, self.nat, self.EV, self.SW = model, _native, EV, SW
        self.lib = SW.bind(EV.bind(model._lib))
        self.segs = segs
        self.offs = np.concatenate([[0], np.cumsum([s["note"].shape[0] for s in segs])]).astype(np.int64)
        self.dev = {k: torch.from_numpy(np.concatenate([s[k] for s in segs])).cuda() for k in ("note", "onset", "contour")}
        self.dev_segs = [{k: v[int(a):int(b)] for k, v in self.dev.items()} for a, b in zip(self.offs[:-1], self.offs[1:])]
        torch.cuda.synchronize()
        self.ptr = [self.dev[k].data_ptr() for k in ("note", "onset", "contour")]

    def sweep(self, sets, room=None):
        return self.SW.note_events_sweep(self.m, self.offs, *self.ptr, self.nat.BP_MEM_DEVICE, sets, None, room)

    def loop(self, sets, room=None):
        return [self.EV.note_events_from_maps(self.m, self.offs, *self.ptr, self.nat.BP_MEM_DEVICE, p, room) for p in sets]

    def call_only(self, sets, room, sweep):
        """() -> rc of the native call alone: every argument and output buffer is made here, once."""
        n = len(self.segs) * len(sets)
        arr = self.SW.sets_array(sets)
        events, bends = (self.nat.bp_note_event * room[0])(), np.empty(room[1], np.int32)
        ev_offs, status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
        p64 = C.POINTER(C.c_int64)
        head = (self.m._handle, len(self.segs), self.offs.ctypes.data_as(p64), *self.ptr, self.nat.BP_MEM_DEVICE)
        tail = (C.addressof(events), room[0], bends.ctypes.data, room[1], ev_offs.ctypes.data_as(p64), status.ctypes.data)
        keep = (arr, events, bends, ev_offs, status)
        if sweep:
            return lambda: (keep, self.lib.bp_note_events_sweep(*head, len(sets), C.addressof(arr), n, None, *tail))[1]
        return lambda: (keep, self.lib.bp_note_events_from_maps(*head, C.addressof(arr), *tail))[1]

    def host(self, sets, threads):
        """Per set and segment the dense half on the device (bp_note_candidates), the sequential half on a pool of host threads."""
        from basic_pitch_amd import note_creation as NC

        with ThreadPoolExecutor(max_workers=threads) as pool:
            futs = []
            for p in sets:
                for s in self.dev_segs:
                    note, bits, bend, status = self.m.note_candidates(s, p)
                    futs.append(pool.submit(NC.decode_candidates, note, bits, bend, p))
            return [f.result() for f in futs]


def rooms(result):
    events, bends, offs, status = result
    last = events[int(offs[-1]) - 1] if int(offs[-1]) else None
    return int(offs[-1]), (int(last.bend_offset + last.n_bends) if last is not None else 0)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def repeat(routes, rotate):
    """REPS timings of every route: {route: [ms]}."""
    names = list(routes)
    samples = {r: [] for r in names}
    for k in range(REPS):
        for r in (names[k % len(names):] + names[:k % len(names)]) if rotate else names:
            samples[r].append(timed(routes[r]))
    return samples


def summarise(samples):
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3)}


def bench_maps(model, name, segs, host_upto, rows_out):
    job = Job(model, segs)
    for kind in ("frame", "onset"):
        for S in SETS:
            sets = param_sets(kind, S)
            sw = job.sweep(sets)          # warms every shape, sizes the buffers, and is compared with the loop
            lp = job.loop(sets)
            n_ev, n_b = rooms(sw)
            assert n_ev == sum(rooms(r)[0] for r in lp) and n_b == sum(rooms(r)[1] for r in lp), (name, kind, S)
            room_sw, room_lp = (max(1, n_ev), max(1, n_b)), (max(1, max(rooms(r)[0] for r in lp)), max(1, max(rooms(r)[1] for r in lp)))
            routes = {"sweep": lambda: job.sweep(sets, room_sw), "loop": lambda: job.loop(sets, room_lp)}
            if S == 1:
                routes["sweep_call_only"], routes["loop_call_only"] = job.call_only(sets, room_sw, True), job.call_only(sets, room_lp, False)
                assert routes["sweep_call_only"]() == 0 == routes["loop_call_only"]()
            samples = repeat(routes, True)
            if S <= host_upto:
                samples.update(repeat({"host_1_thread": lambda: job.host(sets, 1), "host_8_threads": lambda: job.host(sets, 8)}, False))
            row = {"workload": name, "sets": kind, "S": S, "decodes": S * len(segs), "events": n_ev,
                   **{r: summarise(v) for r, v in samples.items()}}
            rows_out.append(row)
            print(json.dumps(row), flush=True)


def bench_pcm(model, rows_out):
    from basic_pitch_amd import clips as CL, events as EV, sweep as SW

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import clip_files as CF

    n = 36164 - 3840  # one window at the model's rate
    base = [np.clip(np.round(CF.tones(n, 1, 22050, seed) * 20000), -32768, 32767).astype(np.int16) for seed in range(16)]
    arrays = [CL.as_clip(base[i % 16], i) for i in range(512)]
    for kind in ("frame", "onset"):
        for S in SETS:
            sets = param_sets(kind, S)
            sw = SW.infer_clips_events_sweep(model, arrays, 22050, sets)
            lp = [EV.infer_clips_events(model, arrays, 22050, p) for p in sets]
            n_ev, n_b = rooms(sw)
            assert n_ev == sum(rooms(r)[0] for r in lp), (kind, S)
            room_sw, room_lp = (max(1, n_ev), max(1, n_b)), (max(1, max(rooms(r)[0] for r in lp)), max(1, max(rooms(r)[1] for r in lp)))
            routes = {"sweep": lambda: SW.infer_clips_events_sweep(model, arrays, 22050, sets, None, room_sw),
                      "loop": lambda: [EV.infer_clips_events(model, arrays, 22050, p, room_lp) for p in sets]}
            samples = repeat(routes, True)
            row = {"workload": "512 one-window PCM clips", "sets": kind, "S": S, "decodes": S * 512, "events": n_ev,
                   **{r: summarise(v) for r, v in samples.items()}}
            rows_out.append(row)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-sweep", choices=("frame", "onset"), default=None)
    ap.add_argument("--one-single", action="store_true")
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--host-upto", type=int, default=8, help="largest S the host-thread routes are timed at")
    ap.add_argument("--skip-pcm", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd.inference import Model

    rng = np.random.default_rng(11)
    one_window = [synthetic(142, rng) for _ in range(512)]
    with Model(device=0, max_windows=64) as model:
        if args.one_sweep:
            Job(model, one_window).sweep(param_sets(args.one_sweep, args.S))
            return
        if args.one_single:
            Job(model, one_window).loop(param_sets("frame", 1))
            return
        rows = []
        bench_maps(model, "512 one-window segments", one_window, args.host_upto, rows)
        bench_maps(model, "64 four-window segments", [synthetic(568, rng) for _ in range(64)], args.host_upto, rows)
        if not args.skip_pcm:
            bench_pcm(model, rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
