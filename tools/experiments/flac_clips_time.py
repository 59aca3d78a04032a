#!/usr/bin/env python
"""Time a job of short FLAC clips on the routes the library offers (profiles/flac_clips.md):

  (a)  a loop of bp_infer_flac_candidates, one clip per call: the device decoder, four launches, an upload and a wait per clip;
  (b1) bp_flac_decode of every clip on ONE host thread, then one bp_infer_clips_candidates call on the float32 samples;
  (b8) the same with the host decoder on EIGHT threads;
  (c)  one bp_infer_flac_clips_candidates call for the whole job;
  (d)  one bp_infer_flac_clips_events call for the whole job (the tracker on the device too: events and bends come home).

    python tools/experiments/flac_clips_time.py [--loop-lib PATH] [--clips 512] [--reps 9] [--warmup 2] [--out OUT.json]

(a), (b1) and (b8) are what the commit before the batched FLAC calls offers; they are the same code in this library.  With
--loop-lib (a build of that commit) route (a) runs a second time on that library: the single-file kernels' device code is
scheduled differently since their bodies moved to csrc/flac_kernels.h (profiles/flac_clips_digest.md), and the two loops side
by side say what that costs.  Workload:
`--clips` clips of one window and as many of four windows, 44.1 kHz stereo 16-bit, written as FLAC by tools/flac_synth.c
(block size 4096, LPC order 8, Rice partitions: a stream like a real encoder's), the bytes and all outputs in pageable host
memory.  Everything runs in one process on one device, each route on its own handle (max_windows 256); the routes take turns
repetition by repetition in rotating order, so drifting clocks and neighbours on the host hit all alike.  A repetition is a host
clock around calls that end in a device synchronise.  Reported: the median and the extremes of the repetitions after the
warm-ups.  Before anything is timed the rows of (a), (b8) and (c) are compared byte for byte, and the events of (d) are counted."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from basic_pitch_amd import _native, build, clips as CL, events as EV, flac_clips as FC  # noqa: E402

HOP, LEAD = 36164, 3840


def make_flac_clips(n_clips: int, windows: int, seed: int, synth: str, tmp: str):
    """FLAC clips whose model-rate length fills `windows` windows exactly: a tone of the piano's range with a little noise."""
    rng = np.random.default_rng(seed)
    n = 2 * (windows * HOP - LEAD)
    t = np.arange(n) / 44100.0
    out = []
    wav, flac = os.path.join(tmp, "c.wav"), os.path.join(tmp, "c.flac")
    for _ in range(n_clips):
        x = 0.2 * np.sin(2 * np.pi * 110.0 * 2 ** (rng.integers(0, 40) / 12.0) * t) + 2e-3 * rng.standard_normal(n)
        pcm = np.ascontiguousarray(np.stack([x, x], axis=1) * 32767).astype(np.int16)
        with wave.open(wav, "wb") as w:
            w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100)
            w.writeframes(pcm.tobytes())
        subprocess.run([synth, wav, flac], check=True, stdout=subprocess.DEVNULL)
        with open(flac, "rb") as f:
            out.append(f.read())
    return out, n


def create(lib, blob):
    h = C.c_void_p()
    rc = lib.bp_create(blob, len(blob), 0, 0, 256, C.byref(h))
    if rc != 0:
        raise _native.NativeLibraryError(f"bp_create: {rc}: {lib.bp_last_error(None).decode()}")
    return h


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    lib = FC.bind(EV.bind(CL.bind(_native.load_library(build.build_library()))))
    lib.bp_infer_flac_candidates.restype = C.c_int
    lib.bp_infer_flac_candidates.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t] + [C.c_void_p] * 4 + [C.POINTER(C.c_int)]
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    old = _native.load_library(a.loop_lib) if a.loop_lib else None
    if old is not None:
        old.bp_infer_flac_candidates.restype, old.bp_infer_flac_candidates.argtypes = C.c_int, lib.bp_infer_flac_candidates.argtypes
    routes = ("loop", "host1", "host8", "candidates", "events") + (("loop_parent",) if old is not None else ())
    handles = {r: create(old if r == "loop_parent" else lib, blob) for r in routes}
    prm = _native.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    pool = ThreadPoolExecutor(max_workers=8)
    result = {"clips": a.clips, "reps": a.reps, "warmup": a.warmup, "loop_lib": a.loop_lib, "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        synth = os.path.join(tmp, "flac_synth")
        subprocess.run(["gcc", "-O2", "-o", synth, os.path.join(ROOT, "tools", "flac_synth.c"), "-lm"], check=True)
        for windows in (1, 4):
            blobs, n_frames = make_flac_clips(a.clips, windows, windows, synth, tmp)
            n = len(blobs)
            tab, keep = FC.clip_table(blobs)
            offs = np.zeros(n + 1, np.int64)
            status = np.zeros(n, np.int32)
            p64 = offs.ctypes.data_as(C.POINTER(C.c_int64))
            assert lib.bp_flac_clips_row_offsets(handles["candidates"], n, tab, 44100, p64, status.ctypes.data) == 0 and not status.any()
            T = int(offs[-1])
            outs = {r: (np.empty((T, 88), np.float32), np.empty((T, 12), np.uint8), np.empty((T, 88), np.int8)) for r in routes if r != "events"}
            floats = [np.empty((n_frames, 2), np.float32) for _ in range(n)]
            ftab = CL.clip_table(floats)
            cap_e, cap_b = 64 * n * windows, 88 * T
            ev, bd = (_native.bp_note_event * cap_e)(), np.empty(cap_b, np.int32)
            ev_offs = np.zeros(n + 1, np.int64)
            one = C.c_int(0)

            def loop(route="loop", lib=lib):
                note, bits, bend = outs[route]
                h = handles[route]
                for i, b in enumerate(blobs):
                    r = int(offs[i])
                    rc = lib.bp_infer_flac_candidates(h, b, len(b), C.addressof(prm), note[r:].ctypes.data, bits[r:].ctypes.data,
                                                      bend[r:].ctypes.data, C.byref(one))
                    assert rc == 0 and one.value == 0, lib.bp_last_error(h)

            def decode_one(i):
                got = C.c_int64(0)
                assert lib.bp_flac_decode(blobs[i], len(blobs[i]), floats[i].ctypes.data, n_frames, C.byref(got)) == 0 and got.value == n_frames

            def host(route, threads):
                if threads == 1:
                    for i in range(n):
                        decode_one(i)
                else:
                    list(pool.map(decode_one, range(n)))
                note, bits, bend = outs[route]
                h = handles[route]
                rc = lib.bp_infer_clips_candidates(h, n, ftab, 44100, _native.BP_MEM_HOST, C.addressof(prm), note.ctypes.data,
                                                   bits.ctypes.data, bend.ctypes.data, status.ctypes.data)
                assert rc == 0 and not status.any(), lib.bp_last_error(h)

            def candidates():
                note, bits, bend = outs["candidates"]
                h = handles["candidates"]
                rc = lib.bp_infer_flac_clips_candidates(h, n, tab, 44100, C.addressof(prm), note.ctypes.data, bits.ctypes.data,
                                                        bend.ctypes.data, status.ctypes.data)
                assert rc == 0 and not status.any(), lib.bp_last_error(h)

            def events():
                h = handles["events"]
                rc = lib.bp_infer_flac_clips_events(h, n, tab, 44100, C.addressof(prm), C.addressof(ev), cap_e, bd.ctypes.data, cap_b,
                                                    ev_offs.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data)
                assert rc == 0 and not status.any(), lib.bp_last_error(h)

            fns = {"loop": loop, "host1": lambda: host("host1", 1), "host8": lambda: host("host8", 8), "candidates": candidates,
                   "events": events, "loop_parent": lambda: loop("loop_parent", old)}
            for r in ("loop", "host8", "candidates", "events") + routes[5:]:  # before anything is timed: the routes agree
                fns[r]()
            for r in ("host8", "candidates") + routes[5:]:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(outs["loop"], outs[r])), f"{r} disagrees with the loop"
            n_events = int(ev_offs[-1])
            times = {r: [] for r in routes}
            for rep in range(a.warmup + a.reps):
                order = routes[rep % len(routes):] + routes[: rep % len(routes)]
                for r in order:
                    t0 = time.perf_counter()
                    fns[r]()
                    dt = time.perf_counter() - t0
                    if rep >= a.warmup:
                        times[r].append(dt * 1e3)
            med = {r: statistics.median(v) for r, v in times.items()}
            result["shapes"][f"{windows}_window"] = {
                "windows_in_all": n * windows, "rows": T, "flac_bytes": sum(len(b) for b in blobs), "pcm_bytes": n * n_frames * 4,
                "events": n_events, "bytes_equal": True,
                **{f"{r}_ms": {"median": med[r], "min": min(times[r]), "max": max(times[r])} for r in routes},
                "candidates_over": {r: med[r] / med["candidates"] for r in ("loop", "host1", "host8")},
                "events_over": {r: med[r] / med["events"] for r in ("loop", "host1", "host8")},
            }
            print(f"{windows}-window clips x {n}: " + ", ".join(f"{r} {med[r]:.1f} ms" for r in routes), flush=True)
    for r, h in handles.items():
        (old if r == "loop_parent" else lib).bp_destroy(h)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
