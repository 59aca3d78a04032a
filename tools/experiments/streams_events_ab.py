"""The tracker's forms on hand-made maps and a NaN in one of four streams of bp_streams_events, through the A/B library's
hooks (run with BASIC_PITCH_AMD_LIB = basic_pitch_amd/lib/libbasicpitch_amd_ab.so; the product library has neither).

Forms: `bp_ab_note_events_from_maps_forms` — bp_note_events_from_maps with one parameter set per segment and the tracker form
(0: as the product chooses, 2: scratch) — on the 16 fixture cases of tests/note_cases.py, the edge shapes of
tests/test_gpu_clips_events.py (restated), 64 seeded random maps of 2 ... 600 rows in packs of 8 segments with a parameter set
each, two segments with different sets, a frame threshold of 0 without melodia and a tolerance of 1; every segment against
bp_note_candidates + bp_notes_decode_candidates on its maps alone.  NaN: `bp_ab_stream_poison` on the second of four streams,
the events call against every stream's single route.  What was compared is saved as JSON for tests/test_gpu_stream_events.py.

    python tools/experiments/streams_events_ab.py OUT.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import note_cases  # noqa: E402
from basic_pitch_amd import Model, _native, note_creation as nc  # noqa: E402
from test_gpu_stream_events import Sess, device_route, melody, note_params, records, single_route  # noqa: E402

model = Model(max_windows=8)
lib = model._lib
_pi64 = C.POINTER(C.c_int64)
hook = lib.bp_ab_note_events_from_maps_forms  # AttributeError: not the A/B library
hook.restype = C.c_int
hook.argtypes = [C.c_void_p, C.c_int64, _pi64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                 C.c_int64, _pi64, C.c_void_p]
lib.bp_ab_stream_poison.restype, lib.bp_ab_stream_poison.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int]


def prm_of(args):
    return nc._note_params(args.get("onset_thresh", 0.5), args.get("frame_thresh", 0.3), args.get("min_note_len", 11),
                           args.get("infer_onsets", True), args.get("max_freq"), args.get("min_freq"), args.get("melodia_trick", True),
                           args.get("energy_tol", nc.ENERGY_TOLERANCE), args.get("include_pitch_bends", True))


def host(maps, prm):
    """bp_note_candidates + bp_notes_decode_candidates on one segment's maps: (records, status)."""
    if maps["note"].shape[0] == 0:
        return [], 0
    note, bits, bend, status = model.note_candidates(maps, prm)
    T = note.shape[0]
    if status:
        return [], status
    args = (note.ctypes.data, bits.ctypes.data, bend.ctypes.data if bend is not None else None, T)
    events, bends, n = nc._grow_and_call(lib.bp_notes_decode_candidates, args + (C.byref(prm),), T, "bp_notes_decode_candidates")
    return records(events, bends, 0, n, bool(prm.include_pitch_bends)), 0


def device(segs, prms, form):
    """One hook call on the segments' maps, one after the other, segment i with prms[i]: (records per segment, status)."""
    cat = {k: np.ascontiguousarray(np.concatenate([np.asarray(o[k], np.float32).reshape(-1, w) for o in segs]))
           for k, w in (("note", 88), ("onset", 88), ("contour", 264))}
    offs = np.concatenate([[0], np.cumsum([o["note"].shape[0] for o in segs])]).astype(np.int64)
    n, T = len(segs), int(offs[-1])
    tab = (_native.bp_note_params * n)(*prms)
    events, bends = (_native.bp_note_event * (88 * T))(), np.zeros(88 * T, np.int32)  # every region's capacity at min_note_len 0
    ev_offs, status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
    rc = hook(model._handle, n, offs.ctypes.data_as(_pi64), cat["note"].ctypes.data, cat["onset"].ctypes.data, cat["contour"].ctypes.data,
              C.addressof(tab), form, C.addressof(events), 88 * T, bends.ctypes.data, 88 * T, ev_offs.ctypes.data_as(_pi64),
              status.ctypes.data)
    _native.check(lib, model._handle, rc, "bp_ab_note_events_from_maps_forms")
    return [records(events, bends, int(ev_offs[i]), int(ev_offs[i + 1]), bool(prms[i].include_pitch_bends)) for i in range(n)], status.tolist()


def group(name, calls):
    """calls: (label, segments, parameter sets) — every call through forms 0 and 2 against the host per segment."""
    g = {"name": name, "mismatches": [], "forms": [], "statuses": set(), "events": 0, "segments": 0, "rows": [1 << 30, 0],
         "rows_list": [], "lengths": set()}
    for label, segs, prms in calls:
        want = [host(s, p) for s, p in zip(segs, prms)]
        g["segments"] += len(segs)
        for s, (w, st) in zip(segs, want):
            T = s["note"].shape[0]
            g["rows"] = [min(g["rows"][0], T), max(g["rows"][1], T)]
            g["rows_list"].append(T)
            g["events"] += len(w)
            g["lengths"] |= {r[1] - r[0] for r in w}
            g["statuses"].add(int(st))
        for form in (0, 2):
            got, status = device(segs, prms, form)
            g["forms"].append(form)
            g["statuses"] |= set(status)
            for i, (gi, (w, _)) in enumerate(zip(got, want)):
                if gi != w:
                    g["mismatches"].append(f"{label} segment {i} form {form}: {len(gi)} events against {len(w)}")
    g["forms"], g["statuses"], g["lengths"] = sorted(set(g["forms"])), sorted(g["statuses"]), sorted(g["lengths"])
    print(name, g["segments"], "segments", g["events"], "events", len(g["mismatches"]), "mismatches", "statuses", g["statuses"])
    return g


# ---- the edge shapes of tests/test_gpu_clips_events.py, restated
H = dict(onset_thresh=0.5, frame_thresh=0.3, min_note_len=3, energy_tol=5, infer_onsets=False)


def blank(rng, T):
    return {"note": rng.uniform(0, 0.02, (T, 88)).astype(np.float32), "onset": np.zeros((T, 88), np.float32),
            "contour": rng.uniform(0, 1, (T, 264)).astype(np.float32)}


def put(rng, m, t0, t1, f, peak=True, lo=0.5, hi=0.9):
    m["note"][t0:t1, f] = rng.uniform(lo, hi, t1 - t0).astype(np.float32)
    if peak:
        m["onset"][t0, f] = 0.9


def edge_shapes():
    rng = np.random.default_rng(77)
    clips = [blank(rng, T) for T in (0, 1, 2, 3)]
    clips[2]["onset"][0, 5] = 0.9
    clips[3]["onset"][1, 5] = 0.9
    clips[3]["note"][1:3, 5] = 0.8
    a = blank(rng, 60)
    put(rng, a, 58, 60, 10), put(rng, a, 50, 60, 12), put(rng, a, 5, 8, 20), put(rng, a, 5, 9, 24)
    put(rng, a, 20, 30, 30), put(rng, a, 34, 40, 30, peak=False)
    put(rng, a, 20, 30, 34), put(rng, a, 35, 41, 34, peak=False)
    put(rng, a, 10, 18, 0), put(rng, a, 30, 44, 87)
    clips.append(a)
    b = blank(rng, 64)
    put(rng, b, 10, 14, 41), put(rng, b, 10, 25, 40), put(rng, b, 30, 40, 61), put(rng, b, 30, 45, 60)
    put(rng, b, 30, 40, 70), put(rng, b, 28, 45, 69)
    clips.append(b)
    c = blank(rng, 50)
    for f in (50, 60):
        put(rng, c, 20, 35, f, peak=False, hi=0.8)
        c["note"][27, f] = 0.95
    put(rng, c, 5, 15, 70, peak=False, hi=0.8), put(rng, c, 30, 45, 20, peak=False, hi=0.8)
    c["note"][12, 70] = c["note"][40, 20] = 0.93
    put(rng, c, 0, 12, 5, peak=False), put(rng, c, 38, 50, 80, peak=False)
    clips.append(c)
    d = blank(rng, 142)
    for k, n in enumerate((7, 8, 127)):
        put(rng, d, 3 + k, 3 + k + n, 10 + 4 * k)
    put(rng, d, 20, 60, 70, peak=False)
    clips.append(d)
    e = blank(rng, 142)
    for k, n in enumerate((128, 129, 131)):
        put(rng, e, 2 + k, 2 + k + n, 30 + 4 * k)
    clips.append(e)
    g = blank(rng, 701)
    for k, n in enumerate((7, 8, 127, 128, 129, 131, 290)):
        put(rng, g, 5 + 3 * k, 5 + 3 * k + n, 4 + 6 * k)
    put(rng, g, 300, 699, 60), put(rng, g, 350, 700, 80, peak=False)
    put(rng, g, 640, 700, 87), put(rng, g, 500, 640, 0, peak=False)
    clips.append(g)
    return clips


def random_maps(rng, T, runs):
    out = {"note": rng.random((T, 88), dtype=np.float32) ** 3, "onset": rng.random((T, 88), dtype=np.float32) ** 4,
           "contour": rng.random((T, 264), dtype=np.float32)}
    if runs:  # note-like structure: runs along time
        out["note"] = np.repeat(out["note"][::7], 7, axis=0)[:T].copy()
    return out


out = {"forms": [], "poison": []}
strip = lambda args: {k: v for k, v in args.items() if k not in ("multiple_pitch_bends", "midi_tempo")}  # noqa: E731
fixture = [(name,) + note_cases.case_args(name) for name in note_cases.CASES]
out["forms"].append(group("fixture cases", [(name, [maps], [prm_of(strip(args))]) for name, maps, args in fixture]))
shapes = edge_shapes()
out["forms"].append(group("edge shapes", [(str(extra), shapes, [prm_of(dict(H, **extra))] * len(shapes))
                                          for extra in ({}, {"include_pitch_bends": False}, {"melodia_trick": False})]))
out["forms"][-1]["rows_list"] = out["forms"][-1]["rows_list"][: len(shapes)]
rng = np.random.default_rng(2024)
packs = []
for pack in range(8):
    # the dense half takes one set per call: onset threshold, inferred onsets, frequency limits, bends; the tracker's own differ
    dense = dict(onset_thresh=float(rng.choice([0.2, 0.5, 0.9])), infer_onsets=bool(rng.integers(0, 2)),
                 min_freq=float(rng.choice([0, 100.0])) or None, max_freq=float(rng.choice([0, 2000.0])) or None,
                 include_pitch_bends=bool(pack % 4 != 3))
    segs = [random_maps(rng, int(rng.integers(2, 601)), k % 3 == 0) for k in range(8)]
    sets = [prm_of(dict(dense, frame_thresh=float(rng.choice([0.1, 0.3, 0.45])), melodia_trick=bool(rng.integers(0, 2)),
                        min_note_len=int(rng.choice([0, 3, 11])), energy_tol=int(rng.choice([1, 5, 11])),
                        include_pitch_bends=dense["include_pitch_bends"] and bool(rng.integers(0, 4)))) for _ in segs]
    packs.append((f"pack {pack}", segs, sets))
out["forms"].append(group("random maps", packs))
two = [note_cases.synthetic(500, 31), note_cases.synthetic(640, 32, density=0.06)]
out["forms"].append(group("two parameter sets", [("two", two, [prm_of(dict(frame_thresh=0.3, min_note_len=11)),
                                                               prm_of(dict(frame_thresh=0.2, min_note_len=4, energy_tol=3,
                                                                           melodia_trick=False, include_pitch_bends=False))]),
                                                 ("swapped", two[::-1], [prm_of(dict(frame_thresh=0.3, min_note_len=11)),
                                                                         prm_of(dict(frame_thresh=0.2, min_note_len=4, energy_tol=3,
                                                                                     melodia_trick=False, include_pitch_bends=False))])]))
# a frame threshold of 0: the bit of a zeroed cell is 0.0 < 0.0, "not below" — sparse notes that stay under the capacity
rng = np.random.default_rng(9)
clean = []
for T in (40, 142, 450):
    c = blank(rng, T)
    for k in range(6):
        put(rng, c, 3 + 5 * k, 10 + 5 * k, 8 + 9 * k)
    clean.append(c)
zero = prm_of(dict(onset_thresh=0.5, frame_thresh=0.0, min_note_len=0, infer_onsets=False, melodia_trick=False))
out["forms"].append(group("frame threshold 0", [("clean", clean, [zero] * 3)]))
out["forms"].append(group("tolerance 1", [("tol 1", [shapes[4], shapes[9], two[0]], [prm_of(dict(H, energy_tol=1))] * 3)]))

# ---- a NaN in one stream of four
x = melody()
prms = note_params()
ROW = 300
specs = [("roll", 500, 22050, "a", (), False), ("roll", 450, 22050, "a", (), False), ("keep", 1500, 22050, "f", (), False),
         ("roll", 150, 22050, "d", (), False)]
ss = [Sess(model, _native, spec, prms, x) for spec in specs]
assert lib.bp_ab_stream_poison(ss[1].s._s, 1, ROW, 40) == 0
at = 0
for n in (90_000, 140_000):  # row 300 in the tail (284 final rows); then among the 426 final rows
    for s in ss:
        s.s.push(x[at:n])
    at = n
    got, want = device_route(model, ss), [single_route(model, s) for s in ss]
    out["poison"].append({"frames": n, "status": [g[2] for g in got], "single_status": [w[2] for w in want],
                          "equal": [g == w for g, w in zip(got, want)], "events": [len(w[3] or []) for w in want],
                          "rows": [[int(w[0]), int(w[1])] for w in want], "final_rows": [s.s.rows for s in ss]})
out["poison_row"] = ROW
for s in ss:
    s.close()
model.close()
with open(sys.argv[1], "w") as f:
    json.dump(out, f)
print("saved", sys.argv[1], [(u["frames"], u["status"], u["equal"]) for u in out["poison"]])
