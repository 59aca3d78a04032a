"""Host glue of the clip-job sinks that have a file of their own (csrc/clips_sweep.hip, clips_multipitch.hip, clips_melody.hip,
clips_align.hip, clips_beat.hip): one small-job device route per sink, where host overhead is the largest share of a call; the
sink rows of profiles/clips_sinks.md.

    python tools/experiments/clips_sinks_time.py [--tree DIR] [--reps 30] [--warm 3]

The jobs and routes are the bench tools' own (tools/bench_note_sweep.py, bench_multipitch.py, bench_melody.py, bench_align.py,
bench_beat.py: their Job classes, which also check every route's result once) at each tool's smallest workload, 512 one-window
segments of 142 rows in device memory: the native call alone with every argument and buffer made before, the routes one after
the other in an order that rotates, host clock around calls that return after the stream has been waited for.  --tree: the
checkout whose package, tools and library are measured (default: this one), so that two trees can be run alternately.  Prints
one JSON line: the median of every route in ms."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    sys.path.insert(0, tree)

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(tree, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    import basic_pitch_amd
    from basic_pitch_amd import build
    from basic_pitch_amd.inference import Model

    assert os.path.abspath(basic_pitch_amd.__file__).startswith(tree), basic_pitch_amd.__file__
    name, rows = "512 one-window segments", [142] * 512
    with Model(device=0, max_windows=64) as m64, Model(device=0, max_windows=8) as m8:
        sweep = tool("bench_note_sweep")
        rng = np.random.default_rng(11)
        job = sweep.Job(m64, [sweep.synthetic(142, rng) for _ in rows])
        sets = sweep.param_sets("frame", 1)
        n_events, n_bends = sweep.rooms(job.sweep(sets))
        jobs = [job, tool("bench_multipitch").Job(m8, name, rows), tool("bench_melody").Job(m8, name, rows),
                tool("bench_align").Job(m8, name, rows, 8), tool("bench_beat").Job(m8, name, rows)]
        routes = {"note_sweep sweep_call_only S=1": job.call_only(sets, (max(1, n_events), max(1, n_bends)), True),
                  "multipitch a (points)": jobs[1].a, "multipitch s (64-set scored sweep)": jobs[1].s,
                  "melody a (records)": jobs[2].a, "melody s (64-set scored sweep)": jobs[2].s,
                  "align a (8 states a segment)": jobs[3].a, "beat a": jobs[4].a}
        names = list(routes)
        samples = {r: [] for r in names}
        for k in range(a.warm + a.reps):
            for r in names[k % len(names):] + names[: k % len(names)]:
                t0 = time.perf_counter()
                rc = routes[r]()
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0, (r, rc)
                if k >= a.warm:
                    samples[r].append(dt)
    print(json.dumps({"tree": tree, "lib": build.LIB_PATH, "reps": a.reps,
                      "median_ms": {r: round(statistics.median(v), 4) for r, v in samples.items()}}), flush=True)


if __name__ == "__main__":
    main()
