#!/usr/bin/env python
"""Time a job of short clips two ways (profiles/clips_batched.md):

  (a) a loop of bp_infer_pcm_raw_candidates, one clip per call — with the library given by --loop-lib (a build of the parent
      commit, which has no batched call; default: the in-tree library, whose single-clip call is the same code);
  (b) one bp_infer_clips_candidates call for the whole job — the in-tree library.

    python tools/experiments/clips_time.py [--loop-lib PATH] [--clips 512] [--reps 20] [--warmup 3] [--out OUT.json]

Workload: `--clips` clips of one window and as many of four windows, 44.1 kHz stereo 16-bit PCM in pageable host memory, the
outputs in pageable host memory.  Both ways run in one process on one device, each on its own handle (max_windows 256), and
alternate repetition by repetition, so drifting clocks and neighbours on the host hit both alike.  A repetition is a host clock
around calls that end in a device synchronise (every call of this ABI waits for its results).  Reported: the median and the
extremes of the repetitions after the warm-ups, and the ratio of the medians.  The outputs of the two ways are compared byte
for byte before anything is timed."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from basic_pitch_amd import _native, build, clips as CL  # noqa: E402

HOP, LEAD = 36164, 3840


def make_clips(n_clips: int, windows: int, seed: int):
    """Clips whose model-rate length fills `windows` windows exactly: noise with a sine, 44.1 kHz stereo int16."""
    rng = np.random.default_rng(seed)
    n = 2 * (windows * HOP - LEAD)
    t = np.arange(n) / 44100.0
    out = []
    for _ in range(n_clips):
        x = 0.2 * np.sin(2 * np.pi * 110.0 * 2 ** (rng.integers(0, 40) / 12.0) * t) + 2e-3 * rng.standard_normal(n)
        out.append(np.ascontiguousarray(np.stack([x, x], axis=1) * 32767).astype(np.int16))
    return out


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    new = CL.bind(_native.load_library(build.build_library()))
    old = _native.load_library(a.loop_lib) if a.loop_lib else new
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    h_new, h_old = create(new, blob), create(old, blob)
    prm = _native.bp_note_params()
    new.bp_note_params_default(C.byref(prm))
    result = {"clips": a.clips, "reps": a.reps, "warmup": a.warmup, "loop_lib": a.loop_lib or "in-tree", "shapes": {}}
    for windows in (1, 4):
        arrays = make_clips(a.clips, windows, windows)
        tab = CL.clip_table(arrays)
        offs = np.zeros(len(arrays) + 1, np.int64)
        assert new.bp_clips_row_offsets(h_new, len(arrays), tab, 44100, offs.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        T = int(offs[-1])
        outs = [(np.empty((T, 88), np.float32), np.empty((T, 12), np.uint8), np.empty((T, 88), np.int8)) for _ in range(2)]
        status = np.zeros(len(arrays), np.int32)
        one = C.c_int(0)

        def loop():
            note, bits, bend = outs[0]
            for i, x in enumerate(arrays):
                r = int(offs[i])
                rc = old.bp_infer_pcm_raw_candidates(h_old, x.ctypes.data, _native.BP_PCM_S16, x.shape[0], 2, 44100, C.byref(prm),
                                                     note[r:].ctypes.data, bits[r:].ctypes.data, bend[r:].ctypes.data, C.byref(one))
                assert rc == 0, old.bp_last_error(h_old)

        def batched():
            note, bits, bend = outs[1]
            rc = new.bp_infer_clips_candidates(h_new, len(arrays), tab, 44100, _native.BP_MEM_HOST, C.addressof(prm),
                                               note.ctypes.data, bits.ctypes.data, bend.ctypes.data, status.ctypes.data)
            assert rc == 0, new.bp_last_error(h_new)

        times = {"loop": [], "batched": []}
        for rep in range(a.warmup + a.reps):
            for name, fn in (("loop", loop), ("batched", batched)) if rep % 2 == 0 else (("batched", batched), ("loop", loop)):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if rep >= a.warmup:
                    times[name].append(dt * 1e3)
            if rep == 0:
                same = all(x.tobytes() == y.tobytes() for x, y in zip(*outs)) and not status.any()
                assert same, "the two ways disagree"
        med = {k: statistics.median(v) for k, v in times.items()}
        result["shapes"][f"{windows}_window"] = {
            "windows_in_all": a.clips * windows, "rows": T,
            "loop_ms": {"median": med["loop"], "min": min(times["loop"]), "max": max(times["loop"])},
            "batched_ms": {"median": med["batched"], "min": min(times["batched"]), "max": max(times["batched"])},
            "ratio": med["loop"] / med["batched"], "bytes_equal": True,
        }
        print(f"{windows}-window clips x {a.clips}: loop {med['loop']:.2f} ms, batched {med['batched']:.2f} ms, "
              f"ratio {med['loop'] / med['batched']:.2f}", flush=True)
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
