"""A NaN in the maps a stream keeps, through the A/B library's hook (run with BASIC_PITCH_AMD_LIB =
basic_pitch_amd/lib/libbasicpitch_amd_ab.so; the product library has no way to put one there: the front end turns a NaN
sample into finite posteriorgrams).  `bp_ab_stream_poison` makes one cell of the KEPT copy a NaN whenever its row is written
there.  The golden clip goes through a live StreamingTranscriber; at each listed prefix the status of an update, the events of
`transcript()` and the host decode of the one-shot maps of the prefix are saved as JSON for tests/test_gpu_stream_peek.py:

    python tools/experiments/stream_nan_ab.py OUT.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from basic_pitch_amd import Model, audio, inference as inf  # noqa: E402
from basic_pitch_amd._native import BP_PCM_S16  # noqa: E402
from basic_pitch_amd.streaming import StreamingTranscriber  # noqa: E402

DECODING = (0.5, 0.3, 127.70, None, None, False, True, 120)
ROW, BIN = 200, 40  # a row of window 1 (rows 142 ... 283)
# frames of the 44.1 kHz clip pushed before each update: no row yet; row 200 in the tail; row 200 final, twice
PREFIXES = (66_150, 110_250, 264_600, 330_750)


def plain(events):
    return [[float(e[0]), float(e[1]), int(e[2]), float(e[3]), [int(b) for b in e[4]]] for e in events]


raw, tag, bits, channels, sr = audio.wav_raw(os.path.join(ROOT, "tests", "golden", "vocadito_10.wav"))
clip = np.frombuffer(raw, dtype=np.int16)
model = Model(max_windows=8)
out = {"row": ROW, "updates": []}
with StreamingTranscriber(model, sr, channels, BP_PCM_S16, live=True) as t:
    poison = t.stream._lib.bp_ab_stream_poison  # AttributeError: not the A/B library
    poison.restype, poison.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int]
    at = 0
    for i, n in enumerate(PREFIXES):
        t.push(clip[at:n])
        at = n
        if i == 1:  # after the first, clean update
            assert poison(t.stream._s, 1, ROW, BIN) == 0
        note, cand, bend = np.zeros((1024, 88), np.float32), np.zeros((1024, 12), np.uint8), np.zeros((1024, 88), np.int8)
        T, status = t.stream.candidates(note, cand, bend, 0)
        _, events = t.transcript()
        ref = inf._output_to_notes(model.predict_pcm_raw(clip[:n], BP_PCM_S16, n, channels, sr), *DECODING)[1]
        out["updates"].append({"frames": n, "final_rows": t.stream.rows, "rows": T, "status": status,
                               "transcript": plain(events), "host_decode": plain(ref)})
model.close()
with open(sys.argv[1], "w") as f:
    json.dump(out, f)
print("saved", sys.argv[1], [(u["frames"], u["final_rows"], u["rows"], u["status"], len(u["transcript"])) for u in out["updates"]])
