"""Timings of a sweep scored at the note and the frame level (bp_note_events_sweep_frame_score,
include/basic_pitch_amd_frame_score.h) against the scoring call without the frame level and against the only route to all three
metrics without it; the numbers of profiles/frame_scores.md.

    python tools/bench_frame_scores.py --out frame_scores.json                 routes a, b (and c, d on this library); REPS repetitions each
    python tools/bench_frame_scores.py --yardstick --lib PARENT.so --out y.json   routes c and d with the device calls of another build (the parent commit's)
    python tools/bench_frame_scores.py --one-call [--S N] [--no-notes]          ONE frame-score call of the segments and nothing else (for a kernel trace)

Jobs and sets are those of tools/bench_note_scores.py: 512 one-window segments (142 rows) in device memory and 512 one-window
int16 clips in host memory, S = 8 and 64 sets that differ in frame_threshold only, include_pitch_bends = 0 in all; the refs of
a segment are its events under the middle set.  Routes, each the native call alone with every argument and buffer made before:
  a        the new call with scores and frames
  b        the new call with frames alone (scores NULL: no note-matching launch)
  c        bp_note_events_sweep_score / bp_infer_clips_events_sweep_score: the note level alone
  d1, d8   bp_note_events_sweep / bp_infer_clips_events_sweep (the events come home), then bp_score_note_events and
           bp_score_note_frames over all decodes on one host thread and on eight
The yardsticks are c and d on the PARENT commit's library (--yardstick --lib; the two host checkers, which need no device,
are taken from this build: the parent has no frame checker), run before and after the others in one sitting.  Before anything
is timed the counts of a and b are compared with those of d (equal in every decode).  A repetition runs the routes one after
the other in an order that rotates; a route's figure is the median of its repetitions, with their range."""
import argparse
import ctypes as C
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_note_scores as BN  # noqa: E402

SETS = BN.SETS


class FrameJob:
    """A job of tools/bench_note_scores.py with the buffers of the frame-score call and of the host route to the same counts."""

    def __init__(self, job, host_lib):
        from basic_pitch_amd import clips, frame_score, score

        self.rows = 142 if "segments" in job.name else clips.n_rows(36164 - 3840, 22050)  # (tools/bench_note_scores.py jobs)
        self.j, self.host = job, frame_score.bind(score.bind(host_lib))
        frame_fn = job.score_fn.__name__.replace("_score", "_frame_score") if job.score_fn is not None else None
        self.frame_fn = None
        if frame_fn and hasattr(job.lib, frame_fn):
            self.frame_fn = getattr(frame_score.bind(job.lib), frame_fn)

    def prepare(self, sets):
        j = self.j
        n_ev, m_on, m_off = j.prepare(sets)  # (also: the scoring call's counts are the note checker's)
        n = j.n
        self.scores, self.frames, self.status = np.zeros((n, 4), np.int32), np.zeros((n, 5), np.int64), np.zeros(n, np.int32)
        self.host_frames = np.zeros((n, 5), np.int64)
        head = j.b_args[:-2]
        self.a_args = head + (self.scores.ctypes.data, self.frames.ctypes.data, self.status.ctypes.data)
        self.b_args = head + (None, self.frames.ctypes.data, self.status.ctypes.data)
        self.frame_args = [args[:4] + (self.rows, args[4], self.host_frames.ctypes.data + 40 * k) for k, args in enumerate(j.host_args)]
        self.d(1)
        if self.frame_fn is not None:
            for with_notes in (True, False):
                self.frames[:] = -1
                assert (self.a() if with_notes else self.b()) == 0
                assert not self.status.any() and np.array_equal(self.frames, self.host_frames), "the device's counts are not the checker's"
            assert np.array_equal(self.scores, j.scores)
        f = self.host_frames.sum(axis=0)
        return n_ev, m_on, m_off, {k: int(v) for k, v in zip(("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub"), f)}

    def a(self):
        return self.frame_fn(*self.a_args)

    def b(self):
        return self.frame_fn(*self.b_args)

    def d(self, threads):
        assert self.j.a() == 0
        notes, frames = self.host.bp_score_note_events, self.host.bp_score_note_frames
        work = list(zip(self.j.host_args, self.frame_args))

        def run(chunk):
            for n_args, f_args in chunk:
                notes(*n_args)
                frames(*f_args)

        if threads == 1:
            return run(work)
        with ThreadPoolExecutor(max_workers=threads) as pool:  # (ctypes releases the interpreter lock around a call)
            list(pool.map(run, [work[k::threads] for k in range(threads)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library for the device calls (the parent commit's, for the yardstick)")
    ap.add_argument("--yardstick", action="store_true", help="routes c and d alone: all that an older library can run")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--no-notes", action="store_true")
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--skip-pcm", action="store_true")
    args = ap.parse_args()
    from basic_pitch_amd import build

    host_lib = C.CDLL(build.LIB_PATH)  # this build's host checkers, whatever library makes the device calls
    if args.lib:
        os.environ["BASIC_PITCH_AMD_LIB"] = os.path.abspath(args.lib)
    from basic_pitch_amd.inference import Model

    rows = []
    with Model(device=0, max_windows=64) as model:
        if args.one_call:
            job = FrameJob(next(BN.jobs(model, True))[0], host_lib)
            job.prepare(BN.param_sets(args.S))
            assert (job.b() if args.no_notes else job.a()) == 0
            return
        for base, _keep in BN.jobs(model, args.skip_pcm):
            job = FrameJob(base, host_lib)
            for S in SETS:
                n_ev, m_on, m_off, sums = job.prepare(BN.param_sets(S))
                routes = {"c": base.b, "d1": lambda: job.d(1), "d8": lambda: job.d(8)}
                if not args.yardstick:
                    routes = {"a": job.a, "b": job.b, **routes}
                samples = BN.repeat(routes)
                row = {"job": base.name, "S": S, "decodes": S * 512, "events": n_ev, "refs": int(base.ref_offs[-1]),
                       "library": args.lib or "built", "matched_onset": m_on, "matched_offset": m_off, **sums,
                       **{r: BN.summarise(v) for r, v in samples.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
