#!/usr/bin/env python
"""Time the note events of a job of short clips two ways (profiles/clips_events.md):

  (a) bp_infer_clips_candidates, then bp_notes_decode_candidates for every clip — with the library given by --loop-lib (a build
      of the parent commit; default: the in-tree library, whose two calls are the same code) — the decoding once on one host
      thread and once on a pool of --threads;
  (b) one bp_infer_clips_events call for the whole job — the in-tree library.

    python tools/experiments/clips_events_time.py [--loop-lib PATH] [--clips 512] [--reps 20] [--warmup 3] [--threads 8] [--out OUT.json]

Workload: `--clips` clips of one window and as many of four windows, 44.1 kHz stereo 16-bit PCM with a few tones that start
and stop inside the clip, in pageable host memory; the outputs in pageable host memory.  The ways run in one process on one
device, each on its own handle (max_windows 256), and alternate repetition by repetition, so drifting clocks and neighbours
on the host hit all alike.  A repetition is a host clock around calls that end in a device synchronise plus, for (a), the
host decoding of every clip.  Reported: the median and the extremes of the repetitions after the warm-ups, the bytes each way
copies from the device to the host, and the events found.  The events of the ways are compared byte for byte before anything
is timed."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from basic_pitch_amd import _native, build, clips as CL, events as EV  # noqa: E402

HOP, LEAD = 36164, 3840


def make_clips(n_clips: int, windows: int, seed: int):
    """Clips whose model-rate length fills `windows` windows exactly: a noise floor and three tones per window that start and
    stop inside the clip, 44.1 kHz stereo int16."""
    rng = np.random.default_rng(seed)
    n = 2 * (windows * HOP - LEAD)
    t = np.arange(n) / 44100.0
    out = []
    for _ in range(n_clips):
        x = 2e-3 * rng.standard_normal(n)
        for _ in range(3 * windows):
            f = 110.0 * 2 ** (rng.integers(0, 40) / 12.0)
            a, b = sorted(rng.uniform(0, n / 44100.0, 2))
            x += rng.uniform(0.1, 0.3) * np.sin(2 * np.pi * f * t) * ((t >= a) & (t < b))
        out.append(np.ascontiguousarray(np.stack([x, x], axis=1) * 32767).clip(-32768, 32767).astype(np.int16))
    return out


def create(lib, blob):
    h = C.c_void_p()
    rc = lib.bp_create(blob, len(blob), 0, 0, 256, C.byref(h))
    if rc != 0:
        raise _native.NativeLibraryError(f"bp_create: {rc}: {lib.bp_last_error(None).decode()}")
    return h


def event_bytes(events, n, bends, n_bends):
    """What is compared: every field of the first n records (the struct has no padding) and the bends."""
    return C.string_at(C.addressof(events), n * C.sizeof(_native.bp_note_event)) + bends[:n_bends].tobytes()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    new = EV.bind(CL.bind(_native.load_library(build.build_library())))
    old = CL.bind(_native.load_library(a.loop_lib)) if a.loop_lib else new
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    h_new, h_old = create(new, blob), create(old, blob)
    prm = _native.bp_note_params()
    new.bp_note_params_default(C.byref(prm))
    result = {"clips": a.clips, "reps": a.reps, "warmup": a.warmup, "threads": a.threads, "loop_lib": a.loop_lib or "in-tree",
              "shapes": {}}
    pool = ThreadPoolExecutor(max_workers=a.threads)
    for windows in (1, 4):
        arrays = make_clips(a.clips, windows, windows)
        n = len(arrays)
        tab = CL.clip_table(arrays)
        offs = np.zeros(n + 1, np.int64)
        assert new.bp_clips_row_offsets(h_new, n, tab, 44100, offs.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        T = int(offs[-1])
        note, bits, bend = np.empty((T, 88), np.float32), np.empty((T, 12), np.uint8), np.empty((T, 88), np.int8)
        status = np.zeros(n, np.int32)
        # per clip of (a): room for its region's capacity would be wasteful on the host; the clips are short
        cap_ev, cap_b = 512 * windows, 88 * 142 * windows
        host_ev = [(_native.bp_note_event * cap_ev)() for _ in range(n)]
        host_b = [np.empty(cap_b, np.int32) for _ in range(n)]
        host_n = np.zeros((n, 2), np.int64)
        max_ev, max_b = n * cap_ev, n * cap_b
        dev_ev = (_native.bp_note_event * max_ev)()
        dev_b = np.empty(max_b, np.int32)
        dev_offs, dev_status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)

        def candidates():
            rc = old.bp_infer_clips_candidates(h_old, n, tab, 44100, _native.BP_MEM_HOST, C.addressof(prm), note.ctypes.data,
                                               bits.ctypes.data, bend.ctypes.data, status.ctypes.data)
            assert rc == 0, old.bp_last_error(h_old)

        def decode(i):
            r0, r1 = int(offs[i]), int(offs[i + 1])
            ne, nb = C.c_int64(0), C.c_int64(0)
            rc = old.bp_notes_decode_candidates(note[r0:].ctypes.data, bits[r0:].ctypes.data, bend[r0:].ctypes.data, r1 - r0,
                                                C.byref(prm), C.addressof(host_ev[i]), cap_ev, host_b[i].ctypes.data, cap_b,
                                                C.byref(ne), C.byref(nb))
            assert rc == 0, old.bp_notes_last_error()
            host_n[i] = ne.value, nb.value

        def host_1():
            candidates()
            for i in range(n):
                decode(i)

        def host_n_threads():
            candidates()
            list(pool.map(lambda k: [decode(i) for i in range(k, n, a.threads)], range(a.threads)))

        def device():
            rc = new.bp_infer_clips_events(h_new, n, tab, 44100, _native.BP_MEM_HOST, C.addressof(prm), C.addressof(dev_ev), max_ev,
                                           dev_b.ctypes.data, max_b, dev_offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                           dev_status.ctypes.data)
            assert rc == 0, new.bp_last_error(h_new)

        ways = (("host_1_thread", host_1), (f"host_{a.threads}_threads", host_n_threads), ("device", device))
        # the byte comparison comes first
        host_1()
        device()
        assert not status.any() and not dev_status.any()
        bo = 0
        for i in range(n):
            ne, nb = int(host_n[i, 0]), int(host_n[i, 1])
            assert int(dev_offs[i + 1] - dev_offs[i]) == ne, ("events of clip", i)
            got = (_native.bp_note_event * ne).from_buffer_copy(C.string_at(C.addressof(dev_ev) + int(dev_offs[i]) * C.sizeof(_native.bp_note_event),
                                                                            ne * C.sizeof(_native.bp_note_event)))
            for e in got:
                e.bend_offset -= bo  # the host decodes each clip into its own bend array
            assert event_bytes(got, ne, dev_b[bo:], nb) == event_bytes(host_ev[i], ne, host_b[i], nb), ("bytes of clip", i)
            bo += nb
        n_events, n_bends = int(dev_offs[-1]), bo
        times = {name: [] for name, _ in ways}
        for rep in range(a.warmup + a.reps):
            k = rep % len(ways)
            for name, fn in ways[k:] + ways[:k]:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if rep >= a.warmup:
                    times[name].append(dt * 1e3)
        shape = {"windows_in_all": a.clips * windows, "rows": T, "events": n_events, "bends": n_bends, "bytes_equal": True,
                 "d2h_bytes_host_route": T * (88 * 4 + 12 + 88) + 16 * n,
                 "d2h_bytes_device_route": 8 * (3 * n + 2) + 16 * n_events + n_bends}
        for name, v in times.items():
            shape[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        result["shapes"][f"{windows}_window"] = shape
        print(f"{windows}-window clips x {a.clips}: " + ", ".join(f"{k} {statistics.median(v):.2f} ms" for k, v in times.items()) +
              f"; {n_events} events; device to host {shape['d2h_bytes_host_route']} / {shape['d2h_bytes_device_route']} bytes", flush=True)
    pool.shutdown()
    new.bp_destroy(h_new)
    old.bp_destroy(h_old)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
