"""A NaN in the ring a rolling stream keeps, through the A/B library's hook (run with BASIC_PITCH_AMD_LIB =
basic_pitch_amd/lib/libbasicpitch_amd_ab.so; the product library cannot put one there).  `bp_ab_stream_poison` makes onset
cell (ROW, BIN) of the kept copy a NaN whenever its row is written to its slot.  The melody of
tests/test_gpu_stream_rolling.py goes through StreamingTranscriber(horizon_seconds=...) with a horizon of 300 rows; at each
listed prefix the status of an update, the events of `transcript()` and what they must be are saved as JSON for that test:
while the row is inside the horizon, the host decode of the one-shot maps' slice with that cell a NaN (status 1); once it has
left, the plain decode of the slice (status 0).

    python tools/experiments/stream_rolling_nan_ab.py OUT.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from basic_pitch_amd import Model, note_creation as nc  # noqa: E402
from basic_pitch_amd._native import BP_PCM_F32  # noqa: E402
from basic_pitch_amd.streaming import StreamingTranscriber  # noqa: E402
from test_gpu_stream_rolling import H, MAPS, melody  # noqa: E402

ROW, BIN = 200, 40  # a row of window 1 (rows 142 ... 283), of block 3 of the stream's table (rows 192 ... 255)
# samples pushed before each update: row 200 in the tail; final, its block whole inside the slice; outside the horizon, twice
PREFIXES = (60_000, 100_000, 160_000, 250_000)


def plain(events):
    return [[float(e[0]), float(e[1]), int(e[2]), float(e[3]), [int(b) for b in e[4]]] for e in events]


def expected(maps, a, T, poisoned):
    sl = {m: np.ascontiguousarray(maps[m][a:T]).copy() for m in MAPS}
    if poisoned:
        sl["onset"][ROW - a, BIN] = np.nan
    ev, bends, n = nc._decode(sl["note"], sl["onset"], sl["contour"], 0.5, 0.3, 11, True, None, None, True, 11, True)
    times = nc.model_frames_to_time(T + 1)
    return [(times[e.start_frame + a], times[e.end_frame + a], e.pitch_midi, e.amplitude,
             bends[e.bend_offset : e.bend_offset + e.n_bends].tolist()) for e in ev[:n]]


x = melody()
model = Model(max_windows=8)
out = {"row": ROW, "updates": []}
with StreamingTranscriber(model, 22050, live=True, horizon_seconds=3.48) as t:
    assert t.horizon_rows == H
    poison = t.stream._lib.bp_ab_stream_poison  # AttributeError: not the A/B library
    poison.restype, poison.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int]
    assert poison(t.stream._s, 1, ROW, BIN) == 0
    at = 0
    for n in PREFIXES:
        t.push(x[at:n])
        at = n
        note, cand, bend = np.zeros((H + 284, 88), np.float32), np.zeros((H + 284, 12), np.uint8), np.zeros((H + 284, 88), np.int8)
        a, T, status = t.stream.candidates_rolling(note, cand, bend, 0)
        _, events = t.transcript()
        ref = model.predict_pcm_raw(x[:n], BP_PCM_F32, n, 1, 22050)
        inside = a <= ROW < T
        a2, kept = t.stream.rolling_maps()
        want = {m: ref[m][a:T].copy() for m in MAPS}
        differs = [m for m in MAPS if not np.array_equal(kept[m].view(np.uint32), want[m].view(np.uint32))]
        if inside:
            want["onset"][ROW - a, BIN] = np.nan
        same_but_cell = inside and differs == ["onset"] and all(np.array_equal(kept[m].view(np.uint32), want[m].view(np.uint32)) for m in MAPS)
        assert inside or not differs, (n, differs)
        out["updates"].append({"frames": n, "final_rows": t.stream.rows, "first_row": a, "rows": T, "status": status,
                               "transcript": plain(events), "expected": plain(expected(ref, a, T, inside)),
                               "maps_equal_but_for_the_cell": bool(same_but_cell)})
model.close()
with open(sys.argv[1], "w") as f:
    json.dump(out, f)
print("saved", sys.argv[1], [(u["frames"], u["final_rows"], u["first_row"], u["rows"], u["status"], len(u["transcript"])) for u in out["updates"]])
