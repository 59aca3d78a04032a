#!/usr/bin/env python
"""Time the note events of N rolling live sessions two ways (profiles/streams_events.md):

  (a) the parent commit's route, on the library given by --loop-lib (a build of the parent commit; default: the in-tree
      library, which has the same calls): one bp_streams_candidates for all N, then bp_notes_decode_candidates_at per session
      over its slice of the host rings — on one host thread and on eight;
  (b) one bp_streams_events call for all N — the in-tree library.

    python tools/experiments/streams_events_time.py [--loop-lib PATH] [--many 8 64 256] [--reps 20] [--warmup 3] [--out OUT.json]
                                                    [--device-only] [--no-python]

Set-up, as tools/experiments/streams_update_time.py: N rolling sessions (a horizon of 60 s: 5,168 rows) on a handle of 256
windows per library, each aged to 30 s of a sine over noise at 22.05 kHz, mono float32, pushed from pageable memory.  A round:
one bp_streams_push of a 0.25 s chunk per stream on both handles (not timed), then the ways in an order that rotates round by
round; the clock is the host's around calls that end in a device synchronise.  (a) keeps the held-rows bookkeeping of a
transcriber.  Before anything is timed every field of every event and every bend of (a) and (b) are compared.  Then the same
rounds through Python on the in-tree library: `transcripts()` against `transcripts(decode="device", midi=False)`.
--device-only: (b) alone, for a kernel trace of it (rocprofv3 --kernel-trace --stats).  Reported: median (min - max)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools", "experiments"))

from basic_pitch_amd import Model, _native, build, streaming  # noqa: E402
from streams_update_time import AGE, CHUNK, RING, Side, signal, stats  # noqa: E402

_pi64 = C.POINTER(C.c_int64)


class EventsSide(Side):
    """The streams of streams_update_time.Side with both ways of getting events."""

    def __init__(self, lib, blob, n, prm):
        super().__init__(lib, blob, n, prm)
        self.prm = prm
        lib.bp_notes_decode_candidates_at.restype = C.c_int
        lib.bp_notes_decode_candidates_at.argtypes = streaming.ROLLING_PROTOTYPES["bp_notes_decode_candidates_at"][1]
        cap_e, cap_b = 2048, 1 << 17  # per session, far above what these signals give; a call that needs more fails its assert
        self.ev = [((_native.bp_note_event * cap_e)(), np.empty(cap_b, np.int32)) for _ in range(n)]  # (a): per session
        if hasattr(lib, "bp_streams_events"):
            for name, (res, args) in streaming.STREAM_EVENTS_PROTOTYPES.items():
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
            self.all_ev, self.all_bends = (_native.bp_note_event * (n * cap_e))(), np.empty(n * cap_b, np.int32)
            self.offs = np.zeros(n + 1, np.int64)
        self.home = 0

    def decode(self, i, a, T):
        note, bits, bend = self.rings[i]
        idx = np.arange(a, T) % RING
        ln, lb, ld = note[idx], bits[idx], bend[idx]  # the slice, linear, as a transcriber unwraps it
        ev, bends = self.ev[i]
        n_ev, n_b = C.c_int64(0), C.c_int64(0)
        rc = self.lib.bp_notes_decode_candidates_at(ln.ctypes.data, lb.ctypes.data, ld.ctypes.data, T - a, a, C.addressof(self.prm),
                                                    C.addressof(ev), len(ev), bends.ctypes.data, bends.shape[0], C.byref(n_ev), C.byref(n_b))
        assert rc == 0
        return n_ev.value, n_b.value

    def host_route(self, bufs, pool):
        """(a): one bp_streams_candidates, the packed rows into the rings, the decode per session."""
        tab = self.many(bufs)
        note, bend, bits = bufs
        for i in range(self.n):
            u = tab[i]
            rn, rb, rd = self.rings[i]
            streaming.scatter_rows(rn, note[u.note_offset : u.note_offset + u.n_rows - u.new_row], u.new_row, u.n_rows)
            streaming.scatter_rows(rd, bend[u.note_offset : u.note_offset + u.n_rows - u.new_row], u.new_row, u.n_rows)
            streaming.scatter_rows(rb, bits[u.bits_offset : u.bits_offset + u.n_rows - u.first_row], u.first_row, u.n_rows)
        self.home = sum((u.n_rows - u.new_row) * (352 + 88) + (u.n_rows - u.first_row) * 12 for u in tab[: self.n])
        jobs = [(i, tab[i].first_row, tab[i].n_rows) for i in range(self.n)]
        counts = list(pool.map(lambda j: self.decode(*j), jobs)) if pool else [self.decode(*j) for j in jobs]
        return tab, counts

    def device_route(self):
        """(b): one bp_streams_events."""
        tab = (_native.bp_stream_events * self.n)()
        for i, s in enumerate(self.s):
            tab[i].stream = s.value
        rc = self.lib.bp_streams_events(self.h, self.n, C.addressof(tab), 1, C.addressof(self.all_ev), len(self.all_ev),
                                        self.all_bends.ctypes.data, self.all_bends.shape[0], self.offs.ctypes.data_as(_pi64))
        assert rc == 0, self.lib.bp_last_error(self.h)
        n_ev = int(self.offs[self.n])
        # what crosses PCIe: 16-byte event records, a byte per bend, the offsets and statuses
        self.home = n_ev * 16 + (int(self.all_ev[n_ev - 1].bend_offset + self.all_ev[n_ev - 1].n_bends) if n_ev else 0) + (3 * self.n + 2) * 8
        return tab


def fields(e, bends):
    return (e.start_frame, e.end_frame, e.pitch_midi, np.float32(e.amplitude).tobytes(), e.start_s, e.end_s, e.n_bends, e.reserved,
            bends[e.bend_offset : e.bend_offset + e.n_bends].tolist())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--many", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    new = _native.load_library(build.build_library())
    old = _native.load_library(a.loop_lib) if a.loop_lib else new
    blob = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    prm = _native.bp_note_params()
    new.bp_note_params_default(C.byref(prm))
    result = {"reps": a.reps, "warmup": a.warmup, "loop_lib": a.loop_lib or "in-tree", "native": {}, "python": {}}
    rounds = a.warmup + a.reps
    ways = ("device",) if a.device_only else ("host1", "host8", "device")
    pool8 = ThreadPoolExecutor(max_workers=8)
    for n in a.many:
        xs = [signal(AGE + (rounds + 1) * CHUNK, i) for i in range(n)]
        A, B = EventsSide(old, blob, n, prm), EventsSide(new, blob, n, prm)
        for side in (A, B):
            side.push([x[:AGE] for x in xs])
        room = n * (AGE // 36164 + rounds + 4) * 142  # rows: every stream is below its horizon
        bufs = (np.empty((room, 88), np.float32), np.empty((room, 88), np.int8), np.empty((room, 12), np.uint8))
        times = {w: [] for w in ways}
        home = {}
        for r in range(rounds + 1):
            chunk = [x[AGE + r * CHUNK : AGE + (r + 1) * CHUNK] for x in xs]
            A.push(chunk), B.push(chunk)
            held0 = list(A.held)
            for k in range(len(ways)):
                name = ways[(r + k) % len(ways)]
                if name != "device":
                    A.held = list(held0)  # both host ways refresh from the same held rows, as one transcriber would
                t0 = time.perf_counter()
                if name == "device":
                    tab = B.device_route()
                else:
                    single = A.host_route(bufs, pool8 if name == "host8" else None)
                dt = (time.perf_counter() - t0) * 1e3
                if r > a.warmup:
                    times[name].append(dt)
                    home[name] = (A if name != "device" else B).home
            if r == 0 and len(ways) == 3:  # every event and bend of every stream, before anything is timed
                utab, counts = single
                total = 0
                for i in range(n):
                    u, (n_ev, n_b) = tab[i], counts[i]
                    assert (u.first_row, u.n_rows, u.status) == (utab[i].first_row, utab[i].n_rows, utab[i].status) and u.status == 0, i
                    lo, hi = int(B.offs[i]), int(B.offs[i + 1])
                    assert hi - lo == n_ev, (i, hi - lo, n_ev)
                    ev, bends = A.ev[i]
                    assert [fields(e, B.all_bends) for e in B.all_ev[lo:hi]] == [fields(e, bends) for e in ev[:n_ev]], i
                    total += n_ev
                assert total > 0
                result["native"].setdefault(str(n), {})["events_compared"] = total
        res = result["native"].setdefault(str(n), {})
        res.update({"rows_per_stream": A.rows[0], "bytes_home": home, **{w + "_ms": stats(times[w]) for w in ways}})
        if len(ways) == 3:
            med = {w: statistics.median(times[w]) for w in ways}
            res.update({"ratio_host1": med["host1"] / med["device"], "ratio_host8": med["host8"] / med["device"], "bytes_equal": True})
        print(f"N = {n}: " + "; ".join(f"{w} {stats(times[w])}" for w in ways) + f"; bytes home {home}", flush=True)
        for side in (A, B):
            for s in side.s:
                side.lib.bp_stream_close(s)
            side.lib.bp_destroy(side.h)
    # through Python on the in-tree library: transcripts() against transcripts(decode="device", midi=False)
    if not a.no_python and not a.device_only:
        model = Model(max_windows=256)
        for n in [n for n in a.many if n <= 64]:
            xs = [signal(AGE + (rounds + 1) * CHUNK, i) for i in range(n)]
            sets = [[streaming.StreamingTranscriber(model, 22050, live=True, horizon_seconds=60.0) for _ in range(n)] for _ in range(2)]
            for ts in sets:
                for lo in range(0, AGE, 4 * 36164):
                    model.push_streams([t.stream for t in ts], [x[lo : min(AGE, lo + 4 * 36164)] for x in xs])
            times = {"host": [], "device": []}
            for r in range(rounds + 1):
                for ts in sets:
                    model.push_streams([t.stream for t in ts], [x[AGE + r * CHUNK : AGE + (r + 1) * CHUNK] for x in xs])
                for name in ("host", "device") if r % 2 == 0 else ("device", "host"):
                    t0 = time.perf_counter()
                    got = model.transcripts(sets[0]) if name == "host" else model.transcripts(sets[1], decode="device", midi=False)
                    dt = (time.perf_counter() - t0) * 1e3
                    if r > a.warmup:
                        times[name].append(dt)
                    if name == "host":
                        host = got
                    else:
                        dev = got
                if r == 0:
                    flat = lambda res: [[(e[0], e[1], e[2], np.float32(e[3]).tobytes(), e[4]) for e in ev] for _, ev in res]  # noqa: E731
                    assert flat(host) == flat(dev)
            result["python"][str(n)] = {"host_ms": stats(times["host"]), "device_ms": stats(times["device"]),
                                        "ratio": statistics.median(times["host"]) / statistics.median(times["device"])}
            print(f"N = {n}, Python: transcripts() {stats(times['host'])}, decode='device', midi=False {stats(times['device'])}", flush=True)
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
