"""Note events straight from the device for a job of many clips (include/basic_pitch_amd_events.h).

`bp_infer_clips_candidates` brings home 450 bytes per row for a host thread to run the sequential half of note decoding on.
`bp_infer_clips_events` runs that half on the device too (csrc/note_track.hip: one workgroup per clip) and brings home the
events and their bends alone; `bp_note_events_from_maps` does the same for posteriorgram segments the caller already holds.
Clip by clip the events are those of the host decoder (tests/test_gpu_clips_events.py).  `Model.transcribe_clips(...,
decode="device")` and `Model.note_events` are the public entries; this module binds the prototypes and holds the host side.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import clips as _clips
from . import jobs as _jobs
from . import note_creation as _notes

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_events.h declares them (tests/test_clips_events_cpu.py compares)
PROTOTYPES = {
    "bp_events_capacity": (_i64, [_i64, _int]),
    "bp_infer_clips_events": (_int, [_vp, _i64, _vp, _int, _int, _vp, _vp, _i64, _vp, _i64, _pi64, _vp]),
    "bp_note_events_from_maps": (_int, [_vp, _i64, _pi64, _vp, _vp, _vp, _int, _vp, _vp, _i64, _vp, _i64, _pi64, _vp]),
}

MAX_ROWS = 8192  # BP_EVENTS_MAX_ROWS


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_events.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def events_capacity(rows: int, min_note_len: int) -> int:
    """The pure-Python mirror of `bp_events_capacity`: the events a clip of `rows` rows may give before it gets status 2 —
    88 pitches times the disjoint notes of more than min_note_len frames that fit in its rows; none over MAX_ROWS rows."""
    if rows <= 0 or rows > MAX_ROWS:
        return 0
    shortest = max(int(min_note_len), 0) + 1
    return 88 * ((int(rows) + shortest - 1) // shortest)


def bends_capacity(rows: int) -> int:
    """The bends a clip of `rows` rows may give before it gets status 2: the size of its bend map."""
    return 88 * int(rows) if 0 < rows <= MAX_ROWS else 0


def _call(lib, handle, what: str, fn, fixed: tuple, n_clips: int, rows: int, room: Optional[Tuple[int, int]] = None):
    """`fn(*fixed, events, max_events, bends, max_bends, event_offsets, status)`, again with the sizes it asks for when the
    buffers are too small: (events, bends, event_offsets, status)."""
    offsets = np.zeros(n_clips + 1, np.int64)
    status = np.zeros(max(1, n_clips), np.int32)
    cap_ev, cap_b = room if room is not None else (max(256, rows // 2), max(4096, 8 * rows))
    while True:
        events = (_native.bp_note_event * max(1, cap_ev))()
        bends = np.empty(max(1, cap_b), np.int32)
        rc = fn(*fixed, C.addressof(events), cap_ev, bends.ctypes.data, cap_b, offsets.ctypes.data_as(_pi64), status.ctypes.data)
        if rc == _native.BP_ERR_INVALID_ARG and room is None:
            m = re.search(r"(\d+) events and (\d+) bends are needed", lib.bp_last_error(handle).decode(errors="replace"))
            if m and (int(m.group(1)) > cap_ev or int(m.group(2)) > cap_b):
                cap_ev, cap_b = max(cap_ev, int(m.group(1))), max(cap_b, int(m.group(2)))
                continue
        _native.check(lib, handle, rc, what)
        return events, bends, offsets, status[:n_clips]


def infer_clips_events(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, prm: Any,
                       room: Optional[Tuple[int, int]] = None):
    """One `bp_infer_clips_events` call for [n_frames, channels] arrays at one rate: (events, bends, event_offsets, status
    per clip), clip i's events at event_offsets[i]:event_offsets[i + 1].  `room`: (max_events, max_bends) to call with, once."""
    lib = bind(_clips.bind(model._lib))
    tab = _clips.clip_table(arrays)
    rows = int(_clips.clips_row_offsets(model, arrays, sample_rate)[-1])
    fixed = (model._handle, len(arrays), tab, int(sample_rate), _native.BP_MEM_HOST, C.addressof(prm))
    return _call(lib, model._handle, "bp_infer_clips_events", lib.bp_infer_clips_events, fixed, len(arrays), rows, room)


def note_events_from_maps(model: Any, row_offsets: Sequence[int], note: Any, onset: Any, contour: Any, mem_kind: int, prm: Any,
                          room: Optional[Tuple[int, int]] = None):
    """One `bp_note_events_from_maps` call: note / onset / contour are pointers (ints) to the maps of all segments, segment i
    at rows row_offsets[i]:row_offsets[i + 1]; returns as `infer_clips_events`."""
    lib = bind(model._lib)
    offs = np.ascontiguousarray(row_offsets, np.int64)
    n = len(offs) - 1
    fixed = (model._handle, n, offs.ctypes.data_as(_pi64), note, onset, contour, int(mem_kind), C.addressof(prm))
    return _call(lib, model._handle, "bp_note_events_from_maps", lib.bp_note_events_from_maps, fixed, n, int(offs[-1]), room)


def clip_events(events, bends: np.ndarray, offsets: np.ndarray, i: int, include_pitch_bends: bool) -> List["_notes.NoteEvent"]:
    """Clip i's events as the tuples `note_creation.decode_candidates` returns."""
    flat = bends
    return [(float(e.start_s), float(e.end_s), int(e.pitch_midi), np.float32(e.amplitude),
             flat[e.bend_offset : e.bend_offset + e.n_bends].tolist() if include_pitch_bends else None)
            for e in events[int(offsets[i]) : int(offsets[i + 1])]]


def stack_maps(outputs: Sequence[Any], what: str):
    """Posteriorgram dicts (numpy arrays or CUDA tensors, all of one kind) as the maps calls take them: (row offsets, the
    three maps of all segments one after the other, {map: pointer, or None without rows}, mem_kind).  The pointers are into
    the returned maps, which the caller holds until its call has returned."""
    return _jobs.stack(outputs, ("note", "onset", "contour"), what)


def note_events(model: Any, outputs: Sequence[Any], prm: Any) -> List[Tuple[Optional[List["_notes.NoteEvent"]], int]]:
    """`Model.note_events`: a list of posteriorgram dicts (numpy arrays or CUDA tensors, all of one kind) through one
    `bp_note_events_from_maps` call -> [(events, status)] per dict; events is None where the status is 1 or 2 (decode those
    maps with `note_creation.model_output_to_notes`)."""
    if not outputs:
        return []
    offs, maps, ptr, mem_kind = stack_maps(outputs, "note_events")
    events, bends, ev_offs, status = note_events_from_maps(model, offs, ptr["note"], ptr["onset"], ptr["contour"], mem_kind, prm)
    with_bends = bool(prm.include_pitch_bends)
    return [(clip_events(events, bends, ev_offs, i, with_bends) if not status[i] else None, int(status[i]))
            for i in range(len(outputs))]
