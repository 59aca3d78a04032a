#!/usr/bin/env python3
"""Files per second of the native file job on SHORT files, per-file route against batches (`transcribe_files(clip_batch=N)`).

One corpus per run: `--files` 16-bit stereo 44.1 kHz files of `--windows` windows each (1: 1.47 s, 4: 6.39 s), WAV or FLAC
(`--kind`; FLAC encoded here by tools/flac_synth.c, as bench.py does), 32 distinct signals and hard links to them, warm in
the page cache.  The same lanes and threads run the job with clip_batch = 0 (the per-file route: the baseline) and with
every value of `--batches`, `--reps` times each into fresh output directories, interleaved so that a drift of the machine
hits all of them alike.  Every job's outputs are compared with the baseline's bytes, and `bp_files_batched()` must count
every file of a batched job.  Prints one JSON line: per setting the median and all rates, the ratio of the medians to the
baseline's and the median of the ratios rep by rep (`vs_per_file_paired`: a drift of the machine cancels in it).

    python tools/bench_files_clip_batches.py --kind wav --windows 1
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, LEAD = 36164, 3840  # samples at 22,050 Hz a window advances by, and the first window's lead


def make_corpus(d, kind, windows, n_files, distinct=32):
    n = 2 * (windows * HOP - LEAD)  # frames at 44,100 Hz: the most that still are `windows` windows
    rng = np.random.default_rng(7)
    t = np.arange(n) / 44100.0
    synth = tools = None
    if kind == "flac":  # (the encoder is built in the system's temporary directory: `d` may be mounted noexec)
        tools = tempfile.TemporaryDirectory()
        synth = os.path.join(tools.name, "flac_synth")
        subprocess.run(["gcc", "-O2", "-o", synth, os.path.join(ROOT, "tools", "flac_synth.c"), "-lm"], check=True)
    paths = []
    for i in range(n_files):
        p = os.path.join(d, f"f{i}.{kind}")
        if i >= distinct:
            os.link(paths[i % distinct], p)
            paths.append(p)
            continue
        f0 = 110.0 * 2 ** (rng.integers(0, 36) / 12.0)
        x = 0.3 * np.sin(2 * np.pi * f0 * t) * (np.sin(2 * np.pi * 1.5 * t) > 0) + 0.01 * rng.standard_normal(n)
        pcm = (np.clip(np.stack([x, x[::-1]], 1), -1, 1) * 32767).astype("<i2")
        q = p if kind == "wav" else os.path.join(d, f"src{i}.wav")
        with wave.open(q, "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(44100)
            w.writeframes(pcm.tobytes())
        if kind == "flac":
            subprocess.run([synth, q, p], check=True, stderr=subprocess.DEVNULL)
            os.unlink(q)
        paths.append(p)
    if tools:
        tools.cleanup()
    return paths


def read_outputs(out_dir):
    return {name: open(os.path.join(out_dir, name), "rb").read() for name in sorted(os.listdir(out_dir))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=("wav", "flac"), default="wav")
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batches", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0, help="host worker threads (0: the usable cores, at most 16)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="where the corpus and the output directories are made (default: the system's)")
    args = ap.parse_args()

    from basic_pitch_amd import transcribe_files
    from basic_pitch_amd.inference import lane_models
    from basic_pitch_amd.sharding import usable_cpus

    threads = args.threads or min(16, usable_cpus())
    settings = [0] + list(args.batches)
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        paths = make_corpus(d, args.kind, args.windows, args.files)
        lanes = lane_models(lanes=args.lanes)
        lib = lanes[0]._lib
        try:
            kw = dict(models=lanes, threads=threads)

            def job(batch, tag):
                out = os.path.join(d, f"out_{batch}_{tag}")
                os.mkdir(out)
                before = lib.bp_files_batched()
                t0 = time.perf_counter()
                rep = transcribe_files(paths, out, clip_batch=batch, **kw)
                el = time.perf_counter() - t0
                bad = [r for r in rep if r["status"] != 0]
                if bad:
                    raise SystemExit(f"clip_batch={batch}: {len(bad)} files failed: {bad[0]}")
                return out, el, lib.bp_files_batched() - before, rep

            # warm-up: the files into the page cache, the lanes' buffers and filters, and the bytes every setting must write
            want = None
            for batch in settings:
                out, _, counted, _ = job(batch, "warm")
                got = read_outputs(out)
                if want is None:
                    want = got
                if got != want:
                    raise SystemExit(f"clip_batch={batch}: the outputs differ from the per-file route's")
                if counted != (len(paths) if batch else 0):
                    raise SystemExit(f"clip_batch={batch}: {counted} of {len(paths)} files came from batched calls")
            rates = {b: [] for b in settings}
            stage = {b: [] for b in settings}
            for r in range(args.reps):
                for batch in settings:
                    _, el, _, rep = job(batch, str(r))
                    rates[batch].append(len(paths) / el)
                    stage[batch].append({k: round(float(np.mean([x["ms"][k] for x in rep])), 4) for k in rep[0]["ms"]})
        finally:
            for m in lanes:
                m.close()
        base = float(np.median(rates[0]))
        print(json.dumps({
            "workload": f"{len(paths)} {args.kind.upper()} files, 16-bit stereo 44.1 kHz, {args.windows} window(s) each "
                        f"({os.path.getsize(paths[0])} bytes), {args.lanes} lanes, {threads} threads, warm page cache, files under "
                        f"{args.tmp or tempfile.gettempdir()}",
            "files_per_s": {str(b): {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v],
                                     "vs_per_file": round(float(np.median(v)) / base, 3),
                                     "vs_per_file_paired": round(float(np.median(np.array(v) / np.array(rates[0]))), 3)}
                            for b, v in rates.items()},
            "mean_stage_ms_per_file_by_rep": {str(b): s for b, s in stage.items()},
        }))


if __name__ == "__main__":
    main()
