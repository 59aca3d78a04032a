#!/usr/bin/env python3
"""What does IMA ADPCM cost the file job?  The WAV corpora of tools/bench_files_clip_batches.py (16-bit stereo 44.1 kHz files
of `--windows` windows, 32 distinct signals and hard links to them, warm in the page cache) encoded as IMA ADPCM WAV files
(format tag 0x11, blocks of 2048 bytes: a quarter of the bytes), and — the yardstick — the S16 WAV files of the samples those
IMA files DECODE to (the codec is lossy: only these hold the same samples), through `transcribe_files` with the same lanes and
threads at every `--batches` setting, `--reps` times each, the two interleaved so that a drift of the machine hits both
alike.  Before anything is timed the IMA job's outputs are compared with the WAV job's, byte for byte.  Prints one JSON line
per corpus, with the medians of the reports' `ms` stages of the last repetition.

    python tools/bench_files_adpcm.py --windows 1 4 [--files 4096] [--tmp /dev/shm]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adpcm_files as A  # noqa: E402  (the encoder and the writer of the tests)
from bench_files_clip_batches import make_corpus, read_outputs  # noqa: E402

BLOCK = 2048


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--batches", type=int, nargs="*", default=[0, 64])
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0, help="host worker threads (0: the usable cores, at most 16)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="where the corpora and the output directories are made (default: the system's)")
    args = ap.parse_args()

    from basic_pitch_amd import adpcm_clips, transcribe_files
    from basic_pitch_amd.inference import lane_models
    from basic_pitch_amd.sharding import usable_cpus

    threads = args.threads or min(16, usable_cpus())
    lanes = lane_models(lanes=args.lanes)
    lib = lanes[0]._lib
    try:
        for windows in args.windows:
            with tempfile.TemporaryDirectory(dir=args.tmp) as d:
                for kind in ("src", "ima", "wav"):
                    os.mkdir(os.path.join(d, kind))
                corpus = {"ima": [], "wav": []}
                made = {}
                for p in make_corpus(os.path.join(d, "src"), "wav", windows, args.files):
                    name = os.path.basename(p)
                    q, t = os.path.join(d, "ima", name), os.path.join(d, "wav", name)
                    first = made.setdefault(os.stat(p).st_ino, (q, t))
                    if first == (q, t):
                        with wave.open(p, "rb") as w:
                            pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
                        blob = A.ima_wav(pcm, 44100, BLOCK)
                        with open(q, "wb") as f:
                            f.write(blob)
                        decoded, _ = adpcm_clips.host_decode(lib, blob)
                        with wave.open(t, "wb") as w:
                            w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100)
                            w.writeframes(decoded.astype("<i2").tobytes())
                    else:
                        os.link(first[0], q), os.link(first[1], t)
                    corpus["ima"].append(q), corpus["wav"].append(t)

                def job(kind, batch, tag):
                    out = os.path.join(d, f"out_{kind}_{batch}_{tag}")
                    os.mkdir(out)
                    before = lib.bp_files_batched()
                    t0 = time.perf_counter()
                    rep = transcribe_files(corpus[kind], out, clip_batch=batch, models=lanes, threads=threads)
                    el = time.perf_counter() - t0
                    bad = [r for r in rep if r["status"] != 0]
                    if bad:
                        raise SystemExit(f"{kind}, clip_batch={batch}: {len(bad)} files failed: {bad[0]}")
                    if lib.bp_files_batched() - before != (len(rep) if batch else 0):
                        raise SystemExit(f"{kind}, clip_batch={batch}: not every file came from a batched call")
                    return out, el, rep

                want = None
                for batch in args.batches:  # warm-up, and the bytes every job must write
                    for kind in ("wav", "ima"):
                        got = read_outputs(job(kind, batch, "warm")[0])
                        want = want or got
                        if got != want:
                            raise SystemExit(f"{kind}, clip_batch={batch}: the outputs differ from the WAV per-file job's")
                rates = {(k, b): [] for k in ("wav", "ima") for b in args.batches}
                stages = {}
                for r in range(args.reps):
                    for batch in args.batches:
                        for kind in (("wav", "ima") if r % 2 == 0 else ("ima", "wav")):
                            _, el, rep = job(kind, batch, str(r))
                            rates[(kind, batch)].append(args.files / el)
                            stages[(kind, batch)] = {k: round(float(np.median([x["ms"][k] for x in rep])), 4) for k in rep[0]["ms"]}
                res = {}
                for batch in args.batches:
                    w, a = rates[("wav", batch)], rates[("ima", batch)]
                    res[str(batch)] = {"wav": [round(x, 1) for x in w], "ima": [round(x, 1) for x in a],
                                       "wav_spread": [round(min(w), 1), round(max(w), 1)],
                                       "ima_median_vs_wav_median": round(float(np.median(a) / np.median(w)), 3),
                                       "median_ms_per_file": {"wav": stages[("wav", batch)], "ima": stages[("ima", batch)]}}
                print(json.dumps({"workload": f"{args.files} files, stereo 44.1 kHz, {windows} window(s) each "
                                              f"({os.path.getsize(corpus['wav'][0])} bytes S16 WAV, {os.path.getsize(corpus['ima'][0])} bytes "
                                              f"IMA ADPCM WAV, blocks of {BLOCK} bytes), {args.lanes} lanes, {threads} threads, warm page "
                                              f"cache, files under {args.tmp or tempfile.gettempdir()}", "files_per_s": res}), flush=True)
    finally:
        for m in lanes:
            m.close()


if __name__ == "__main__":
    main()
