"""A NaN in one of three streams of a many-stream update, through the A/B library's hook (run with BASIC_PITCH_AMD_LIB =
basic_pitch_amd/lib/libbasicpitch_amd_ab.so; the product library cannot put one there), and the device memory of a handle over
repeated updates, which only that library counts (`bp_ab_live_device_bytes`).  Three streams of the melody of
tests/test_gpu_streams_update.py on one handle — rolling (H = 300), keeping, rolling (H = 150) — the middle one with onset cell
(ROW, BIN) of its kept copy poisoned by `bp_ab_stream_poison`.  At each listed prefix `bp_streams_candidates` runs on all
three, then the single call of each; the statuses and whether the contractual bytes agree are saved as JSON for that test, and
so are the library's byte count and every stream's `bp_stream_state_bytes` after each of 20 more updates.

    python tools/experiments/streams_update_nan_ab.py OUT.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from basic_pitch_amd import Model, note_creation as nc, streaming  # noqa: E402
from test_gpu_streams_update import melody, unwrap  # noqa: E402

ROW, BIN = 200, 40
PREFIXES = (60_000, 100_000)  # row 200 in the tail (142 final rows); then among the 284 final rows

x = melody()
model = Model(max_windows=8)
prm = nc._note_params(0.5, 0.3, 11, True, None, None, True, 11, True)
streams = [model.open_stream(22050) for _ in range(3)]
streams[0].keep_rolling(prm, 300)
streams[1].keep(prm, 1500)
streams[2].keep_rolling(prm, 150)
ring_rows = (584, 1784, 434)
lib = streams[0]._lib
lib.bp_ab_stream_poison.restype, lib.bp_ab_stream_poison.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int]  # AttributeError: not the A/B library
lib.bp_ab_live_device_bytes.restype, lib.bp_ab_live_device_bytes.argtypes = C.c_int64, []
assert lib.bp_ab_stream_poison(streams[1]._s, 1, ROW, BIN) == 0

out = {"updates": [], "live_device_bytes": [], "state_bytes": []}
at = 0
for n in PREFIXES:
    for s in streams:
        s.push(x[at:n])
    at = n
    tab, note, bend, bits = streaming.streams_candidates(model, streams, [0, 0, 0])
    up = {"frames": n, "final_rows": [s.rows for s in streams], "status": [], "single_status": [], "rows": [], "fields_equal": [],
          "note_equal": [], "bytes_equal": []}
    for i, (s, u) in enumerate(zip(streams, tab)):
        rn, rb, rd = np.zeros((ring_rows[i], 88), np.float32), np.zeros((ring_rows[i], 12), np.uint8), np.zeros((ring_rows[i], 88), np.int8)
        if i == 1:
            (T, status), a = s.candidates(rn, rb, rd, 0), 0
        else:
            a, T, status = s.candidates_rolling(rn, rb, rd, 0)
        k = u.n_rows - u.new_row
        note_eq = note[u.note_offset : u.note_offset + k].tobytes() == unwrap(rn, a, T).tobytes()
        rest_eq = (bend[u.note_offset : u.note_offset + k].tobytes() == unwrap(rd, a, T).tobytes()
                   and bits[u.bits_offset : u.bits_offset + T - a].tobytes() == unwrap(rb, a, T).tobytes())
        up["status"].append(int(u.status)), up["single_status"].append(int(status)), up["rows"].append([int(u.first_row), int(u.n_rows)])
        up["fields_equal"].append((u.first_row, u.n_rows, u.new_row) == (a, T, a))
        up["note_equal"].append(bool(note_eq)), up["bytes_equal"].append(bool(note_eq and rest_eq))
    out["updates"].append(up)
for _ in range(20):
    streaming.streams_candidates(model, streams, [0, 0, 0])
    out["live_device_bytes"].append(int(lib.bp_ab_live_device_bytes()))
    out["state_bytes"].append([s.state_bytes() for s in streams])
for s in streams:
    s.close()
model.close()
with open(sys.argv[1], "w") as f:
    json.dump(out, f)
print("saved", sys.argv[1], [(u["frames"], u["status"], u["bytes_equal"]) for u in out["updates"]], out["live_device_bytes"][::19])
