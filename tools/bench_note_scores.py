"""Timings of a scored sweep (bp_note_events_sweep_score, include/basic_pitch_amd_score.h) against bringing the events home and
scoring them on the host; the numbers of profiles/note_scores.md.

    python tools/bench_note_scores.py --out note_scores.json             every job, route and S; REPS repetitions each
    python tools/bench_note_scores.py --only-yardstick --lib PATH         route (a) alone, on another build of the library
    python tools/bench_note_scores.py --one-score [--S N]                 ONE scored sweep of the segments and nothing else (for a kernel trace)

Jobs (those of tools/bench_note_sweep.py): 512 one-window segments (142 rows) held in device memory, and 512 one-window int16
clips in host memory; S = 8 and 64 sets that differ in frame_threshold only, include_pitch_bends = 0 in all.  The refs of a
segment are its events under the middle set.  Routes:
  a        the sweep call that brings the events home (bp_note_events_sweep / bp_infer_clips_events_sweep), the native call alone
           with every argument and output buffer made beforehand: the cost of getting the events to the host before any scoring
  b        the scoring call on the same job, likewise the native call alone
  c1, c8   a, then bp_score_note_events over all decodes on one host thread and on eight (native calls; the binding's work —
           slicing the events per decode — is made beforehand)
  d        a through the Python binding, then score.score_note_events per decode
Before anything is timed the counts of b are compared with those of c (equal in every decode).  A repetition runs the routes
one after the other in an order that rotates from repetition to repetition; a route's figure is the median of its
repetitions, with their range.  Every call returns after its stream has been waited for: the host clock around a call is the
call."""
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

REPS = 5
SETS = (8, 64)


def param_sets(S):
    from basic_pitch_amd import note_creation as NC

    return [NC._note_params(0.5, 0.2 + 0.25 * k / max(1, S - 1), 11, True, None, None, True, NC.ENERGY_TOLERANCE, False)
            for k in range(S)]


class Job:
    """One job: head = the arguments of its sweep calls before n_sets (segments in device memory, or PCM clips)."""

    def __init__(self, model, name, head, sweep_fn, score_fn, n_seg, py_sweep):
        from basic_pitch_amd import _native, score, sweep as SW

        self.m, self.nat, self.SC, self.SW = model, _native, score, SW
        self.lib = SW.bind(model._lib)
        if hasattr(self.lib, score_fn):  # (--lib: a library from before the scoring calls runs route a alone)
            score.bind(self.lib)
        self.name, self.head, self.n_seg, self.py_sweep = name, head, n_seg, py_sweep
        self.sweep_name, self.sweep_fn, self.score_fn = sweep_fn, getattr(self.lib, sweep_fn), getattr(self.lib, score_fn, None)

    def prepare(self, sets):
        """Buffers of both calls sized once, the refs, the per-decode slices for the host routes."""
        p64 = C.POINTER(C.c_int64)
        S, n = len(sets), len(sets) * self.n_seg
        self.sets, self.arr, self.n = sets, self.SW.sets_array(sets), n
        events, bends, ev_offs, status = self.py_sweep(sets, None)
        n_ev = int(ev_offs[-1])
        assert not status.any()
        mid = S // 2
        rows = lambda lo, hi: np.array([(e.start_s, e.end_s, e.pitch_midi) for e in events[lo:hi]], np.float64).reshape(-1, 3)  # noqa: E731
        self.refs = [rows(int(ev_offs[mid * self.n_seg + i]), int(ev_offs[mid * self.n_seg + i + 1])) for i in range(self.n_seg)]
        self.ref_offs, self.flat = self.SC.refs_table(self.refs)
        self.prm = self.SC.score_params()
        self.room = (max(1, n_ev), 1)
        self.events, self.bends = (self.nat.bp_note_event * self.room[0])(), np.empty(1, np.int32)
        self.ev_offs, self.status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
        self.scores, self.sc_status = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
        self.host_scores = (self.nat.bp_note_score * n)()
        mid_args = (S, C.addressof(self.arr), n, None)
        self.a_args = self.head + mid_args + (C.addressof(self.events), self.room[0], self.bends.ctypes.data, 1,
                                              self.ev_offs.ctypes.data_as(p64), self.status.ctypes.data)
        self.b_args = self.head + mid_args + (self.ref_offs.ctypes.data_as(p64), self.flat.ctypes.data, C.addressof(self.prm),
                                              self.scores.ctypes.data, self.sc_status.ctypes.data)
        assert self.a() == 0 and self.b() == 0
        size = C.sizeof(self.nat.bp_note_event)
        base, ref0, out0 = C.addressof(self.events), self.flat.ctypes.data, C.addressof(self.host_scores)
        self.host_args = [(base + int(self.ev_offs[j]) * size, int(self.ev_offs[j + 1] - self.ev_offs[j]),
                           ref0 + int(self.ref_offs[j % self.n_seg]) * 24, int(self.ref_offs[j % self.n_seg + 1] - self.ref_offs[j % self.n_seg]),
                           C.addressof(self.prm), out0 + 16 * j) for j in range(n)]
        self.c(1)
        host = np.array([(s.n_ref, s.n_est, s.matched_onset, s.matched_offset) for s in self.host_scores], np.int32)
        assert not self.sc_status.any() and np.array_equal(host, self.scores), "the device's counts are not the checker's"
        return n_ev, int(self.scores[:, 2].sum()), int(self.scores[:, 3].sum())

    def a(self):
        return self.sweep_fn(*self.a_args)

    def b(self):
        return self.score_fn(*self.b_args)

    def c(self, threads):
        assert self.a() == 0
        fn = self.lib.bp_score_note_events
        if threads == 1:
            for args in self.host_args:
                fn(*args)
            return
        chunks = [self.host_args[k::threads] for k in range(threads)]
        with ThreadPoolExecutor(max_workers=threads) as pool:  # (ctypes releases the interpreter lock around a call)
            list(pool.map(lambda chunk: [fn(*args) for args in chunk], chunks))

    def d(self):
        events, _, ev_offs, _ = self.py_sweep(self.sets, self.room)
        return [self.SC.score_note_events([(e.start_s, e.end_s, e.pitch_midi) for e in events[int(ev_offs[j]):int(ev_offs[j + 1])]],
                                          self.refs[j % self.n_seg]) for j in range(self.n)]


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


def jobs(model, skip_pcm):
    import torch

    from basic_pitch_amd import _native, clips as CL, sweep as SW
    from bench_note_sweep import synthetic

    p64 = C.POINTER(C.c_int64)
    rng = np.random.default_rng(11)
    segs = [synthetic(142, rng) for _ in range(512)]
    offs = np.concatenate([[0], np.cumsum([s["note"].shape[0] for s in segs])]).astype(np.int64)
    dev = {k: torch.from_numpy(np.concatenate([s[k] for s in segs])).cuda() for k in ("note", "onset", "contour")}
    torch.cuda.synchronize()
    ptr = [dev[k].data_ptr() for k in ("note", "onset", "contour")]
    keep = [offs, dev]
    head = (model._handle, 512, offs.ctypes.data_as(p64), *ptr, _native.BP_MEM_DEVICE)
    yield Job(model, "512 one-window segments", head, "bp_note_events_sweep", "bp_note_events_sweep_score", 512,
              lambda sets, room: SW.note_events_sweep(model, offs, *ptr, _native.BP_MEM_DEVICE, sets, None, room)), keep
    if skip_pcm:
        return
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import clip_files as CF

    n = 36164 - 3840  # one window at the model's rate
    base = [np.clip(np.round(CF.tones(n, 1, 22050, seed) * 20000), -32768, 32767).astype(np.int16) for seed in range(16)]
    arrays = [CL.as_clip(base[i % 16], i) for i in range(512)]
    tab = CL.clip_table(arrays)
    head = (model._handle, 512, tab, 22050, _native.BP_MEM_HOST)
    yield Job(model, "512 one-window PCM clips", head, "bp_infer_clips_events_sweep", "bp_infer_clips_events_sweep_score", 512,
              lambda sets, room: SW.infer_clips_events_sweep(model, arrays, 22050, sets, None, room)), [arrays, tab]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's, for the yardstick)")
    ap.add_argument("--only-yardstick", action="store_true", help="route a alone: all that an older library can run")
    ap.add_argument("--one-score", action="store_true")
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--skip-pcm", action="store_true")
    ap.add_argument("--skip-python", action="store_true", help="leave out route d")
    args = ap.parse_args()
    if args.lib:
        os.environ["BASIC_PITCH_AMD_LIB"] = os.path.abspath(args.lib)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=64) as model:
        if args.only_yardstick:
            from basic_pitch_amd import sweep as SW

            for job, _keep in jobs(model, args.skip_pcm):
                for S in SETS:  # (an older library has no scoring call: the buffers are made here)
                    sets = param_sets(S)
                    events, _, ev_offs, _ = job.py_sweep(sets, None)
                    n, n_ev = S * 512, int(ev_offs[-1])
                    arr = SW.sets_array(sets)
                    out = (job.nat.bp_note_event * max(1, n_ev))()
                    bends, offs, status = np.empty(1, np.int32), np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
                    fn = job.sweep_fn
                    call = lambda: fn(*job.head, S, C.addressof(arr), n, None, C.addressof(out), max(1, n_ev), bends.ctypes.data, 1,  # noqa: E731
                                      offs.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data)
                    assert call() == 0
                    row = {"job": job.name, "S": S, "decodes": n, "events": n_ev, "library": args.lib or "built",
                           "a": summarise(repeat({"a": call})["a"])}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        elif args.one_score:
            job, _keep = next(jobs(model, True))
            job.prepare(param_sets(args.S))
            return
        else:
            for job, _keep in jobs(model, args.skip_pcm):
                for S in SETS:
                    n_ev, m_on, m_off = job.prepare(param_sets(S))
                    routes = {"a": job.a, "b": job.b, "c1": lambda: job.c(1), "c8": lambda: job.c(8)}
                    if not args.skip_python:
                        routes["d"] = job.d
                    samples = repeat(routes)
                    row = {"job": job.name, "S": S, "decodes": S * 512, "events": n_ev, "refs": int(job.ref_offs[-1]),
                           "matched_onset": m_on, "matched_offset": m_off, **{r: summarise(v) for r, v in samples.items()}}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
