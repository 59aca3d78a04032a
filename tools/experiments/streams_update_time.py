#!/usr/bin/env python
"""Time the live-transcript update of N rolling sessions two ways (profiles/streams_update_many.md):

  (a) a loop of bp_stream_candidates_rolling, one stream per call — with the library given by --loop-lib (a build of the parent
      commit, which has no many-stream call; default: the in-tree library, whose single-stream call is the same code);
  (b) one bp_streams_candidates call for all N — the in-tree library.

    python tools/experiments/streams_update_time.py [--loop-lib PATH] [--many 8 64 256] [--reps 20] [--warmup 3] [--out OUT.json]

Set-up: N rolling sessions (a horizon of 60 s: 5,168 rows) on a handle of 256 windows per library, each aged to 30 s of a sine
over noise at 22.05 kHz, mono float32, pushed from pageable memory.  A round: one bp_streams_push of a 0.25 s chunk per stream on
both handles (not timed), then the update both ways, in an order that alternates round by round; the clock is the host's around
calls that end in a device synchronise.  Both ways keep the held-rows bookkeeping of a transcriber.  Before anything is timed
the contractual bytes of (a) and (b) are compared.  Then the same rounds through Python on the in-tree library: a loop of
`StreamingTranscriber.transcript()` against one `transcripts()`, host decoding included.  Reported: median (min - max)."""
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

from basic_pitch_amd import Model, _native, build, streaming  # noqa: E402

H_ROWS, RING = 5168, 5168 + 284
CHUNK, AGE = 5512, 30 * 22050


def signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    return (0.2 * np.sin(2 * np.pi * 110.0 * 2 ** (rng.integers(0, 40) / 12.0) * t) + 2e-3 * rng.standard_normal(n)).astype(np.float32)


class Side:
    """N rolling streams on a handle of one library, with a transcriber's host rings and held rows."""

    def __init__(self, lib, blob, n, prm):
        self.lib, self.n = lib, n
        protos = {**streaming.PROTOTYPES, **streaming.ROLLING_PROTOTYPES}
        if hasattr(lib, "bp_streams_candidates"):  # the parent commit's library has no such call
            protos.update(streaming.UPDATE_PROTOTYPES)
        for name, (res, args) in protos.items():
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
        self.h = C.c_void_p()
        assert lib.bp_create(blob, len(blob), 0, 0, 256, C.byref(self.h)) == 0
        self.s = []
        for _ in range(n):
            s = C.c_void_p()
            assert lib.bp_stream_open(self.h, _native.BP_PCM_F32, 1, 22050, C.byref(s)) == 0
            assert lib.bp_stream_keep_rolling(s, C.addressof(prm), H_ROWS) == 0
            self.s.append(s)
        self.rows, self.held = [0] * n, [0] * n
        self.rings = [(np.zeros((RING, 88), np.float32), np.zeros((RING, 12), np.uint8), np.zeros((RING, 88), np.int8)) for _ in range(n)]
        self.out = [np.empty((4 * 142, w), np.float32) for w in (88, 88, 264) for _ in range(n)]

    def push(self, chunks):
        n, vp = self.n, C.c_void_p
        arr = lambda v: (vp * n)(*v)  # noqa: E731
        got = (C.c_int64 * n)()
        k = chunks[0].shape[0]
        for lo in range(0, k, 2 * 36164):  # at most two windows a step: the rows fit self.out
            part = [c[lo : lo + 2 * 36164] for c in chunks]
            rc = self.lib.bp_streams_push(self.h, n, arr([s.value for s in self.s]), arr([p.ctypes.data for p in part]),
                                          (C.c_int64 * n)(*[p.shape[0] for p in part]), 0, arr([o.ctypes.data for o in self.out[:n]]),
                                          arr([o.ctypes.data for o in self.out[n : 2 * n]]), arr([o.ctypes.data for o in self.out[2 * n :]]),
                                          (C.c_int64 * n)(*[4 * 142] * n), 0, got)
            assert rc == 0, self.lib.bp_last_error(self.h)
            self.rows = [r + g for r, g in zip(self.rows, got)]

    def loop(self):
        a, T, st = C.c_int64(0), C.c_int64(0), C.c_int(0)
        res = []
        for i, s in enumerate(self.s):
            note, bits, bend = self.rings[i]
            rc = self.lib.bp_stream_candidates_rolling(s, 1, note.ctypes.data, bits.ctypes.data, bend.ctypes.data, RING, self.held[i],
                                                       C.byref(a), C.byref(T), C.addressof(st))
            assert rc == 0, self.lib.bp_last_error(self.h)
            res.append((a.value, T.value, st.value))
        self.held = list(self.rows)
        return res

    def many(self, bufs):
        tab = (_native.bp_stream_update * self.n)()
        for i, s in enumerate(self.s):
            tab[i].stream, tab[i].held_rows = s.value, self.held[i]
        note, bend, bits = bufs
        rc = self.lib.bp_streams_candidates(self.h, self.n, C.addressof(tab), 1, note.ctypes.data, bend.ctypes.data, bits.ctypes.data,
                                            note.shape[0], bits.shape[0])
        assert rc == 0, self.lib.bp_last_error(self.h)
        self.held = list(self.rows)
        return tab


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--many", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    new = _native.load_library(build.build_library())
    old = _native.load_library(a.loop_lib) if a.loop_lib else new
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    prm = _native.bp_note_params()
    new.bp_note_params_default(C.byref(prm))
    result = {"reps": a.reps, "warmup": a.warmup, "loop_lib": a.loop_lib or "in-tree", "native": {}, "python": {}}
    rounds = a.warmup + a.reps
    for n in a.many:
        xs = [signal(AGE + (rounds + 1) * CHUNK, i) for i in range(n)]
        A, B = Side(old, blob, n, prm), Side(new, blob, n, prm)
        for side in (A, B):
            side.push([x[:AGE] for x in xs])
        room = n * (AGE // 36164 + rounds + 4) * 142  # rows: every stream is below its horizon
        bufs = (np.empty((room, 88), np.float32), np.empty((room, 88), np.int8), np.empty((room, 12), np.uint8))
        times = {"loop": [], "many": []}
        for r in range(rounds + 1):
            chunk = [x[AGE + r * CHUNK : AGE + (r + 1) * CHUNK] for x in xs]
            A.push(chunk), B.push(chunk)
            for name in ("loop", "many") if r % 2 == 0 else ("many", "loop"):
                t0 = time.perf_counter()
                got = A.loop() if name == "loop" else B.many(bufs)
                dt = (time.perf_counter() - t0) * 1e3
                if r > a.warmup:
                    times[name].append(dt)
                if name == "loop":
                    single = got
                else:
                    tab = got
            if r == 0:  # the contractual bytes, before anything is timed: held 0, so every row of the slice
                note, bend, bits = bufs
                for i in range(n):
                    u, (fa, T, st) = tab[i], single[i]
                    assert (u.first_row, u.n_rows, u.status, u.new_row) == (fa, T, st, fa) and st == 0, i
                    idx = np.arange(fa, T) % RING
                    rn, rb, rd = A.rings[i]
                    assert note[u.note_offset : u.note_offset + T - fa].tobytes() == rn[idx].tobytes(), i
                    assert bend[u.note_offset : u.note_offset + T - fa].tobytes() == rd[idx].tobytes(), i
                    assert bits[u.bits_offset : u.bits_offset + T - fa].tobytes() == rb[idx].tobytes(), i
        result["native"][str(n)] = {"rows_per_stream": A.rows[0], "loop_ms": stats(times["loop"]), "many_ms": stats(times["many"]),
                                    "ratio": statistics.median(times["loop"]) / statistics.median(times["many"]), "bytes_equal": True}
        print(f"N = {n}: loop {stats(times['loop'])}, one call {stats(times['many'])}", flush=True)
        for side in (A, B):
            for s in side.s:
                side.lib.bp_stream_close(s)
            side.lib.bp_destroy(side.h)
    # through Python, host decoding included: the in-tree library both ways
    model = Model(max_windows=256)
    for n in [n for n in a.many if n <= 64]:  # 256 sessions twice over are 2.5 GB of host rings: the native table covers them
        xs = [signal(AGE + (rounds + 1) * CHUNK, i) for i in range(n)]
        sets = [[streaming.StreamingTranscriber(model, 22050, live=True, horizon_seconds=60.0) for _ in range(n)] for _ in range(2)]
        for ts in sets:
            for lo in range(0, AGE, 4 * 36164):
                model.push_streams([t.stream for t in ts], [x[lo : min(AGE, lo + 4 * 36164)] for x in xs])
        times = {"loop": [], "many": []}
        for r in range(rounds + 1):
            for ts in sets:
                model.push_streams([t.stream for t in ts], [x[AGE + r * CHUNK : AGE + (r + 1) * CHUNK] for x in xs])
            for name in ("loop", "many") if r % 2 == 0 else ("many", "loop"):
                t0 = time.perf_counter()
                got = [t.transcript() for t in sets[0]] if name == "loop" else model.transcripts(sets[1])
                dt = (time.perf_counter() - t0) * 1e3
                if r > a.warmup:
                    times[name].append(dt)
                if name == "loop":
                    single = got
                else:
                    batch = got
            if r == 0:
                assert [[(e[0], e[1], e[2], float(e[3]), e[4]) for e in ev] for _, ev in single] == \
                       [[(e[0], e[1], e[2], float(e[3]), e[4]) for e in ev] for _, ev in batch]
        result["python"][str(n)] = {"loop_ms": stats(times["loop"]), "many_ms": stats(times["many"]),
                                    "ratio": statistics.median(times["loop"]) / statistics.median(times["many"])}
        print(f"N = {n}, Python: loop {stats(times['loop'])}, transcripts() {stats(times['many'])}", flush=True)
        for ts in sets:
            for t in ts:
                t.close()
    model.close()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
