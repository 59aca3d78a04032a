#!/usr/bin/env python3
"""Does the container change the file job's rate?  The WAV corpora of tools/bench_files_clip_batches.py (16-bit stereo
44.1 kHz files of `--windows` windows, 32 distinct signals and hard links to them, warm in the page cache) and the same
samples rewritten as 16-bit AIFF (big-endian, converted on the device), through `transcribe_files` with the same lanes and
threads at every `--batches` setting, `--reps` times each, WAV and AIFF interleaved so that a drift of the machine hits both
alike.  The yardstick is the WAV job of the same run: its range over the repetitions is the spread, and the AIFF rates are
expected inside it (the bytes per file and the launches are the same).  Before anything is timed the AIFF job's outputs are
compared with the WAV job's, byte for byte.  Prints one JSON line per corpus.

    python tools/bench_files_containers.py --windows 1 4 [--files 4096] [--tmp /dev/shm]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_files_clip_batches import make_corpus, read_outputs  # noqa: E402


def aiff_from_wav(src, dst):
    """The 16-bit WAV file `src` as an AIFF file: the same samples, byte-swapped, behind COMM and SSND."""
    with wave.open(src, "rb") as w:
        ch, rate, n = w.getnchannels(), w.getframerate(), w.getnframes()
        assert w.getsampwidth() == 2
        data = np.frombuffer(w.readframes(n), "<i2").astype(">i2").tobytes()
    e = rate.bit_length() - 1
    comm = struct.pack(">HIHHQ", ch, n, 16, 16383 + e, rate << (63 - e))
    body = b"COMM" + struct.pack(">I", len(comm)) + comm + b"SSND" + struct.pack(">III", 8 + len(data), 0, 0) + data
    with open(dst, "wb") as f:
        f.write(b"FORM" + struct.pack(">I", 4 + len(body)) + b"AIFF" + body)


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

    from basic_pitch_amd import transcribe_files
    from basic_pitch_amd.inference import lane_models
    from basic_pitch_amd.sharding import usable_cpus

    threads = args.threads or min(16, usable_cpus())
    lanes = lane_models(lanes=args.lanes)
    lib = lanes[0]._lib
    try:
        for windows in args.windows:
            with tempfile.TemporaryDirectory(dir=args.tmp) as d:
                corpus = {}
                for kind in ("wav", "aiff"):
                    os.mkdir(os.path.join(d, kind))
                corpus["wav"] = make_corpus(os.path.join(d, "wav"), "wav", windows, args.files)
                corpus["aiff"], made = [], {}
                for p in corpus["wav"]:
                    q = os.path.join(d, "aiff", os.path.basename(p)[:-4] + ".aif")
                    first = made.setdefault(os.stat(p).st_ino, q)
                    if first == q:
                        aiff_from_wav(p, q)
                    else:
                        os.link(first, q)
                    corpus["aiff"].append(q)

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
                    return out, el

                want = None
                for batch in args.batches:  # warm-up, and the bytes every job must write
                    for kind in ("wav", "aiff"):
                        got = read_outputs(job(kind, batch, "warm")[0])
                        want = want or got
                        if got != want:
                            raise SystemExit(f"{kind}, clip_batch={batch}: the outputs differ from the WAV per-file job's")
                rates = {(k, b): [] for k in ("wav", "aiff") for b in args.batches}
                for r in range(args.reps):
                    for batch in args.batches:
                        for kind in (("wav", "aiff") if r % 2 == 0 else ("aiff", "wav")):
                            rates[(kind, batch)].append(args.files / job(kind, batch, str(r))[1])
                res = {}
                for batch in args.batches:
                    w, a = rates[("wav", batch)], rates[("aiff", batch)]
                    res[str(batch)] = {"wav": [round(x, 1) for x in w], "aiff": [round(x, 1) for x in a],
                                       "wav_spread": [round(min(w), 1), round(max(w), 1)],
                                       "aiff_inside_the_spread": [bool(min(w) <= x <= max(w)) for x in a],
                                       "aiff_median_vs_wav_median": round(float(np.median(a) / np.median(w)), 3)}
                print(json.dumps({"workload": f"{args.files} files, 16-bit stereo 44.1 kHz, {windows} window(s) each "
                                              f"({os.path.getsize(corpus['wav'][0])} bytes WAV, {os.path.getsize(corpus['aiff'][0])} bytes "
                                              f"AIFF), {args.lanes} lanes, {threads} threads, warm page cache, files under "
                                              f"{args.tmp or tempfile.gettempdir()}", "files_per_s": res}), flush=True)
    finally:
        for m in lanes:
            m.close()


if __name__ == "__main__":
    main()
