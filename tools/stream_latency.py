"""What a streaming step costs beside the one-shot call on the same windows (recorded in profiles/stream_latency.md; no gate).

    python tools/stream_latency.py --out profiles/stream_latency.md       # the wall-time tables (a) and (b)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/stream_latency.py --trace 64 20
    python tools/stream_latency.py --launches DIR 64 20                   # (c): kernel launches per step from that trace
    python tools/stream_latency.py --peek --out profiles/stream_peek_latency.md   # (d): a live session, per update
    python tools/stream_latency.py --push-only [--package DIR]            # (d)'s push-only row; DIR: another checkout's root
    python tools/stream_latency.py --ages rolling --out profiles/stream_rolling_latency.md   # (e): an update at session ages
    python tools/stream_latency.py --ages plain [--package DIR]           # (e) for the mode that keeps every row

The yardstick is existing code in the same process on the same device: `bp_infer` with host buffers on the same number of
windows in one call.  Every stream is a 22.05 kHz mono float stream primed with 3840 samples, so that each further push of
one hop (36164 samples) completes exactly one window.  All calls are made at the C ABI with the argument arrays built once:
what is timed is the library, not Python.  Medians of wall times, each call ending in the library's own wait for the device.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

import numpy as np

# --package DIR: the basic_pitch_amd of another checkout (built there), e.g. the parent commit's for a same-box comparison
_pkg = sys.argv[sys.argv.index("--package") + 1] if "--package" in sys.argv[:-1] else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(_pkg))

HOP, WIN, LEAD = 36164, 43844, 3840


class Bench:
    def __init__(self, max_windows: int = 256):
        from basic_pitch_amd import Model, streaming

        self.model = Model(max_windows=max_windows)
        self.lib = streaming.bind(self.model._lib)
        self.h = self.model._handle
        rng = np.random.default_rng(0)
        self.hop = rng.uniform(-1, 1, HOP).astype(np.float32)
        self.windows = rng.uniform(-1, 1, (max_windows, WIN)).astype(np.float32)
        self.out = {k: np.empty((max_windows * 172, w), np.float32) for k, w in (("note", 88), ("onset", 88), ("contour", 264))}

    def ok(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}: {self.lib.bp_last_error(self.h).decode()}")

    def infer(self, n: int):
        o = self.out
        args = (self.h, self.windows.ctypes.data, n, o["note"].ctypes.data, o["onset"].ctypes.data, o["contour"].ctypes.data, 0)
        return lambda: self.ok(self.lib.bp_infer(*args), "bp_infer")

    def open(self, n: int):
        """n primed streams: the next hop-sized push of each completes exactly one window."""
        streams = [self.model.open_stream(22050) for _ in range(n)]
        for s in streams:
            s.push(self.hop[: WIN - LEAD - HOP])
        return streams

    def single_push(self, s):
        o, rows = self.out, C.c_int64(0)
        args = (s._s, self.hop.ctypes.data, HOP, 0, o["note"].ctypes.data, o["onset"].ctypes.data, o["contour"].ctypes.data, 142,
                0, C.byref(rows))

        def call():
            self.ok(self.lib.bp_stream_push(*args), "bp_stream_push")
            assert rows.value == 142

        return call

    def step(self, active, idle=()):
        """One bp_streams_push: a hop for every stream of `active`, an empty entry for every stream of `idle`."""
        n, o = len(active) + len(idle), self.out
        arr = lambda vals: (C.c_void_p * n)(*vals)  # noqa: E731
        at = lambda k, i, w: o[k].ctypes.data + i * 142 * w * 4  # noqa: E731
        rows = (C.c_int64 * n)()
        slot = list(range(len(active))) + [0] * len(idle)  # an idle entry gets no rows: any valid pointer serves
        args = (self.h, n, arr([s._s.value for s in list(active) + list(idle)]),
                arr([self.hop.ctypes.data] * len(active) + [None] * len(idle)), (C.c_int64 * n)(*([HOP] * len(active) + [0] * len(idle))),
                0, arr([at("note", i, 88) for i in slot]), arr([at("onset", i, 88) for i in slot]),
                arr([at("contour", i, 264) for i in slot]), (C.c_int64 * n)(*([142] * n)), 0, rows)

        def call():
            self.ok(self.lib.bp_streams_push(*args), "bp_streams_push")
            assert sum(rows) == 142 * len(active)

        return call


def median_ms(call, repeats: int, warmup: int = 10) -> float:
    for _ in range(warmup):
        call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times)


def tables(out_path: str) -> None:
    b = Bench()
    lines = ["# Streaming steps beside the one-shot call (tools/stream_latency.py)", "",
             "Wall time per call in ms, median; every call ends in the library's wait for the device.  22.05 kHz mono float",
             "streams, each push one hop (36164 samples, 141 KB from pageable host memory) completing exactly one window; the",
             "yardstick `bp_infer` takes the same number of windows (43844 samples each) from pageable host memory in one call.",
             "Handle of 256 windows.", ""]
    (s,) = b.open(1)
    a_push, a_infer = median_ms(b.single_push(s), 300), median_ms(b.infer(1), 300)
    lines += ["## (a) one stream, one window per push (median of 300)", "", "| call | ms |", "|---|---|",
              f"| `bp_stream_push` completing 1 window | {a_push:.3f} |", f"| `bp_infer`, 1 window | {a_infer:.3f} |", ""]
    s.close()
    lines += ["## (b) N streams, one window each per step", "",
              "`N single pushes`: the same N windows through N `bp_stream_push` calls, per step of N (median over the steps;",
              "at least 300 pushes and 5 steps per row).  `+4N idle`: the same step with 4 N further streams in the call whose",
              "entries are empty.", "",
              "| N | `bp_streams_push` (300 steps) | `+4N idle` (300 steps) | `bp_infer`, N windows (300 calls) | N single pushes |",
              "|---|---|---|---|---|"]
    for n in (16, 64, 256):
        streams = b.open(5 * n)
        active, idle = streams[:n], streams[n:]
        t_step = median_ms(b.step(active), 300)
        t_idle = median_ms(b.step(active, idle), 300)
        t_infer = median_ms(b.infer(n), 300)
        pushes = [b.single_push(s) for s in active]
        t_single = median_ms(lambda: [p() for p in pushes], max(5, -(-300 // n)), warmup=2)
        lines.append(f"| {n} | {t_step:.3f} | {t_idle:.3f} | {t_infer:.3f} | {t_single:.3f} |")
        for s in streams:
            s.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def live_signal(seconds: float) -> np.ndarray:
    """A seeded melody of decaying three-partial tones, 22.05 kHz mono float: notes for the decoder to find."""
    rng = np.random.default_rng(3)
    n = int(seconds * 22050)
    x = 1e-3 * rng.standard_normal(n)
    for a in range(0, n, 22050 // 3):
        t = np.arange(min(22050 // 3, n - a)) / 22050.0
        f0 = 220.0 * 2 ** (int(rng.integers(0, 24)) / 12.0)
        x[a : a + t.size] += sum(0.3 / h * np.sin(2 * np.pi * f0 * h * t) for h in (1, 2, 3)) * np.exp(-3.0 * t)
    return x.astype(np.float32)


def push_only_times(model, x: np.ndarray, chunk: int) -> list:
    """Wall time of every `Stream.push` of a session that only pushes (ms)."""
    times = []
    with model.open_stream(22050) as s:
        for a in range(0, len(x), chunk):
            t0 = time.perf_counter()
            s.push(x[a : a + chunk])
            times.append(1e3 * (time.perf_counter() - t0))
    return times


def push_only(sessions: int = 3, updates: int = 120, chunk_s: float = 0.25) -> None:
    """The push-only row of (d) on its own, with nothing but `Model.open_stream` and `Stream.push`: runs on any commit that
    has streams (--package), so the same box can time the commit before a change to the push path beside the one after."""
    import basic_pitch_amd
    from basic_pitch_amd import Model

    model = Model(max_windows=8)
    chunk = int(chunk_s * 22050)
    x = live_signal(updates * chunk_s)
    push_only_times(model, x[: 20 * chunk], chunk)
    print(f"package: {os.path.dirname(os.path.abspath(basic_pitch_amd.__file__))}")
    print("| session | median ms | worst ms |\n|---|---|---|")
    for i in range(sessions):
        t = push_only_times(model, x, chunk)
        print(f"| push only, {len(t)} pushes, run {i} | {statistics.median(t):.3f} | {max(t):.3f} |")
    model.close()


def peek_table(out_path: str, updates: int = 120, chunk_s: float = 0.25) -> None:
    """(d) A live session: 0.25-second chunks of a 22.05 kHz mono float stream; after every push a `Stream.peek()` (the rows
    of the audio so far) and a `StreamingTranscriber.transcript()` (its note events).  Wall times at the Python interface,
    which is where a live user stands; a session that only pushes, on the same chunks, beside it."""
    from basic_pitch_amd import Model
    from basic_pitch_amd.streaming import StreamingTranscriber

    model = Model(max_windows=8)
    chunk = int(chunk_s * 22050)
    x = live_signal(updates * chunk_s)
    push_only_times(model, x[: 20 * chunk], chunk)  # warm-up: allocations, the first launches
    base = push_only_times(model, x, chunk)
    t_push, t_peek, t_tr, n_events, tail_rows = [], [], [], 0, []
    with StreamingTranscriber(model, 22050, live=True) as t:
        for a in range(0, len(x), chunk):
            t0 = time.perf_counter()
            t.push(x[a : a + chunk])
            t1 = time.perf_counter()
            tail = t.stream.peek()
            t2 = time.perf_counter()
            _, events = t.transcript()
            t3 = time.perf_counter()
            t_push.append(1e3 * (t1 - t0)), t_peek.append(1e3 * (t2 - t1)), t_tr.append(1e3 * (t3 - t2))
            tail_rows.append(tail["note"].shape[0])
            n_events = len(events)
    row = lambda name, v: f"| {name} | {statistics.median(v):.3f} | {max(v):.3f} |"  # noqa: E731
    lines = ["# A live session, per update (tools/stream_latency.py --peek)", "",
             f"{len(t_push)} updates of {chunk_s} s ({chunk} samples, 22.05 kHz mono float32 from pageable host memory), handle of 8",
             "windows, wall time in ms at the Python interface; every call ends in the library's wait for the device.  A peek runs",
             f"the one or two tail windows ({min(tail_rows)} to {max(tail_rows)} rows here); `transcript()` runs them again behind the",
             "kept maps, the stats fold, the peak bitmap of all rows and the bends of the new rows, then the host's note tracker",
             f"({n_events} events at the last update, {updates * chunk_s:.0f} s of audio).  No time is gated.", "",
             "| call | median | worst |", "|---|---|---|",
             row("`push` in a session that only pushes", base), row("`push` in the live session (rows kept on the device)", t_push),
             row("`Stream.peek()`", t_peek), row("`StreamingTranscriber.transcript()`", t_tr), ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    model.close()


def ages_table(mode: str, out_path: str, updates: int = 40, chunk_s: float = 0.25, runs: int = 2) -> None:
    """(e) What an update costs at a session age.  One live session is aged with pushes of eight hops (not timed) to just
    short of 1, 10 and 60 minutes; at each age `updates` chunks of 0.25 s are pushed, each followed by a `transcript()`; the
    wall time of push + transcript() is taken per update.  mode "rolling": horizon_seconds = 600; mode "plain": the mode that
    keeps every row (`bp_stream_keep`, default max_rows of ten minutes), which uses nothing newer than `live=True` and so runs
    on an older checkout (--package); it stops after the ten-minute age, beyond which its pushes are refused."""
    import basic_pitch_amd
    from basic_pitch_amd import Model
    from basic_pitch_amd.streaming import StreamingTranscriber

    model = Model(max_windows=8)
    chunk = int(chunk_s * 22050)
    loop = live_signal(60.0)
    span = updates * chunk
    ages = (1, 10, 60) if mode == "rolling" else (1, 10)
    push_only_times(model, loop[: 20 * chunk], chunk)  # warm-up: allocations, the first launches
    lines = [f"package: {os.path.dirname(os.path.abspath(basic_pitch_amd.__file__))}", "",
             f"mode {mode}: {updates} updates of {chunk_s} s per age, wall time of `push` + `transcript()` in ms", "",
             "| run | age at the last update | rows decoded | events | median | p10 | p90 | worst | bytes home per update | state bytes |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for run in range(runs):
        kw = {"horizon_seconds": 600.0} if mode == "rolling" else {}
        with StreamingTranscriber(model, 22050, live=True, **kw) as t:
            at = 0

            def feed(n):
                nonlocal at
                t.push(np.take(loop, np.arange(at, at + n) % loop.size))  # the 60-second melody, over and over
                at += n

            for age in ages:
                target = int(age * 60 * 22050) - span
                while at < target:
                    feed(min(8 * HOP, target - at))
                t.transcript()  # the rows of the ageing pushes come home here, not in a timed update
                times, n_events, sent = [], 0, []
                for _ in range(updates):
                    held = t.stream.rows
                    t0 = time.perf_counter()
                    feed(chunk)
                    _, events = t.transcript()
                    times.append(1e3 * (time.perf_counter() - t0))
                    total = t.stream.rows + t.stream.rows_bound(0)
                    decoded = min(total, t.horizon_rows) if mode == "rolling" else total
                    sent.append((total - held) * (88 * 4 + 88) + 12 * decoded + 16)
                    n_events = len(events)
                q = np.percentile(times, [50, 10, 90])
                lines.append(f"| {run} | {at / 22050 / 60:.2f} min | {decoded} | {n_events} | {q[0]:.3f} | {q[1]:.3f} | {q[2]:.3f} | "
                             f"{max(times):.3f} | {int(np.median(sent))} | {t.stream.state_bytes()} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    model.close()


def trace(n: int, steps: int) -> None:
    """The traced program: n primed streams, `steps` steps of one window each (run it under rocprofv3)."""
    b = Bench()
    call = b.step(b.open(n))
    for _ in range(steps):
        call()


def launches(trace_dir: str, n: int, steps: int) -> None:
    """Kernel launches per step from the kernel statistics of the traced run: the n priming pushes launch one downmix
    each and nothing else, everything beyond them belongs to the steps."""
    calls = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    if not calls:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    print(f"## (c) kernel launches, {n} streams, {steps} steps of one window per stream (rocprofv3 --kernel-trace --stats)\n")
    print("| kernel | launches | per step |\n|---|---|---|")
    total = 0
    for name, c in sorted(calls.items(), key=lambda kv: -kv[1]):
        c_steps = c - n if "stream_mono_kernel" in name else c
        total += c_steps
        print(f"| `{name[:90]}` | {c} | {c_steps / steps:.2f} |")
    print(f"\nPer step: {total / steps:.2f} launches, of which {n} are the ingest of the {n} chunks (one per stream with input).")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", nargs=2, type=int, metavar=("N", "STEPS"))
    ap.add_argument("--launches", nargs=3, metavar=("DIR", "N", "STEPS"))
    ap.add_argument("--peek", action="store_true", help="(d): push, peek and transcript() per update of a live session")
    ap.add_argument("--push-only", action="store_true", help="the push-only sessions of (d) alone")
    ap.add_argument("--ages", choices=("rolling", "plain"), help="(e): push + transcript() at session ages of 1, 10 (, 60) minutes")
    ap.add_argument("--package", default="", help="root of the checkout whose basic_pitch_amd is timed (default: this one)")
    a = ap.parse_args()
    if a.ages:
        ages_table(a.ages, a.out)
    elif a.push_only:
        push_only()
    elif a.peek:
        peek_table(a.out)
    elif a.trace:
        trace(*a.trace)
    elif a.launches:
        launches(a.launches[0], int(a.launches[1]), int(a.launches[2]))
    else:
        tables(a.out)
