"""Forced alignment (include/basic_pitch_amd_align.h): reference notes that are not on the audio's time base — a MIDI score,
the annotations of another take, labels that sit off or drift — aligned to the note and onset posteriorgrams of a segment.

The score becomes a list of states in order (`states_from_notes`: a state spans two consecutive note boundaries and says which
pitches sound and which start), a monotone dynamic programme finds the first frame of every state (`align_rows` is the host
checker `bp_align_rows`; `Model.align` and `Model.transcribe_clips_align` run many segments on the device, csrc/align.hip),
and `notes_from_frames` turns the first frames back into notes on the audio's time base, which are `bp_ref_note`s again and
go into the score calls.  The definition is this project's own: unpinned against any third-party aligner.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import jobs as _jobs
from .note_creation import frames_to_time_at

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_align.h declares them (tests/test_align_cpu.py compares)
_TAIL = [_pi64, _vp, _vp, _vp, _i64, _pi64, _vp]  # state_offsets, states, p, first_frame, max_states, total, status
PROTOTYPES = {
    "bp_align_params_default": (None, [_vp]),
    "bp_align_rows": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _pi64, _vp]),
    "bp_align_from_maps": (_int, [_vp, _i64, _pi64, _vp, _vp, _int] + _TAIL),
    "bp_infer_clips_align": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

PITCHES = 88                 # BP_ALIGN_PITCHES
Q_ONE = 1024                 # BP_ALIGN_Q_ONE
MAX_ONSET_WEIGHT = 16        # BP_ALIGN_MAX_ONSET_WEIGHT
LANES = 1024                 # BP_ALIGN_LANES
SMALL_LANES = 256            # BP_ALIGN_SMALL_LANES
STATES_PER_LANE = 4          # BP_ALIGN_STATES_PER_LANE
MAX_STATES = 4096            # BP_ALIGN_MAX_STATES
MAX_CELLS = 268435456        # BP_ALIGN_MAX_CELLS
READ_AHEAD = 8               # BP_ALIGN_READ_AHEAD
READ_AHEAD_WIDE = 4          # BP_ALIGN_READ_AHEAD_WIDE
TILE_ROWS = 128              # BP_ALIGN_TILE_ROWS
EMIT_ROWS = 32               # BP_ALIGN_EMIT_ROWS
FREE = 2**31 - 1             # `latest` of a state without a window
# bp_align_state, 40 bytes
ALIGN_STATE = np.dtype([("active", np.uint64, (2,)), ("begins", np.uint64, (2,)), ("earliest", np.int32), ("latest", np.int32)])
_PARAM_FIELDS = ("threshold_q", "onset_weight", "reserved")
_STATE_FIELDS = ("lead", "tail", "max_shift_s")


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_align.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def align_params(params: Any = None, **fields: Any) -> "_native.bp_align_params":
    """`bp_align_params`: the defaults (`bp_align_params_default`: threshold_q 307, onset_weight 2), a given record as it is,
    or a dict / keyword fields on top of the defaults."""
    if isinstance(params, _native.bp_align_params):
        return params
    p = _native.bp_align_params()
    bind(_native.load_library()).bp_align_params_default(C.addressof(p))
    for k, v in dict(params or {}, **fields).items():
        if k not in _PARAM_FIELDS:
            raise TypeError(f"unknown field {k!r}: bp_align_params has {list(_PARAM_FIELDS)}")
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(v), 0) if np.isscalar(v) else (int(v[0]), int(v[1]))
        else:
            setattr(p, k, int(v))
    return p


def nearest_frame(times_s: Any, n_frames: int) -> np.ndarray:
    """The frame of 0 ... n_frames - 1 whose time is nearest to each of `times_s`, ties to the earlier frame: the
    nearest-sample rule of `melody.ref_track` with the roles exchanged."""
    x = np.asarray(times_s, np.float64).reshape(-1)
    if n_frames <= 1:
        return np.zeros(len(x), np.int64)
    at = frames_to_time_at(np.arange(int(n_frames)))
    right = np.clip(np.searchsorted(at, x, side="left"), 1, n_frames - 1)
    left = right - 1
    return np.where(np.abs(x - at[left]) <= np.abs(at[right] - x), left, right).astype(np.int64)


def _notes(ref_notes: Any) -> np.ndarray:
    return np.asarray(ref_notes, np.float64).reshape(-1, 3)


def states_from_notes(ref_notes: Any, n_frames: int, lead: bool = True, tail: bool = True,
                      max_shift_s: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The states of a score: `ref_notes` rows of (start_s, end_s, pitch_midi) -> (`ALIGN_STATE` records, and per note the
    index of its first state and of the state after its last).

    The boundaries are the distinct start_s / end_s values; a state spans two consecutive boundaries, `active` the notes
    that cover it and `begins` the notes that start at its left boundary.  Pitches are rounded to the nearest MIDI number; one
    outside 21 ... 108 is a ValueError that names the note.  `lead` / `tail`: a silence state before the first and after the
    last boundary.  With `max_shift_s` the first frame of a state is held to the frames nearest (`nearest_frame`) to its left
    boundary's own time -+ the shift, clipped to the segment; without it the states depend on the ORDER of the boundaries alone.
    A note that ends where it starts covers no state (its two indices are equal)."""
    notes = _notes(ref_notes)
    if not np.all(np.isfinite(notes)):
        raise ValueError("states_from_notes: a note with a field that is not finite")
    pitch = np.rint(notes[:, 2]).astype(np.int64)
    for i, (n, q) in enumerate(zip(notes, pitch)):
        if q < 21 or q > 108:
            raise ValueError(f"states_from_notes: note {i} has pitch {n[2]}, outside 21 ... 108")
        if n[1] < n[0]:
            raise ValueError(f"states_from_notes: note {i} ends before it starts")
    bounds = np.unique(np.concatenate([notes[:, 0], notes[:, 1]]))
    n_inner = max(0, len(bounds) - 1)
    first = int(bool(lead))
    states = np.zeros(first + n_inner + int(bool(tail)), ALIGN_STATE)
    states["latest"] = FREE
    start_at = np.searchsorted(bounds, notes[:, 0])
    end_at = np.searchsorted(bounds, notes[:, 1])
    for a, b, q in zip(start_at, end_at, pitch - 21):
        bit = np.uint64(1) << np.uint64(q & 63)
        if b > a:
            states["active"][first + a : first + b, q >> 6] |= bit
            states["begins"][first + a, q >> 6] |= bit
    if max_shift_s is not None and len(bounds):
        shift = float(max_shift_s)
        if not shift >= 0.0:
            raise ValueError("states_from_notes: max_shift_s must be >= 0")
        left = bounds[: len(states) - first]  # the left boundary of every state but the leading one
        states["earliest"][first:] = nearest_frame(left - shift, n_frames)
        states["latest"][first:] = nearest_frame(left + shift, n_frames)
        states["earliest"][0], states["latest"][0] = 0, FREE  # (the first state begins at frame 0 whatever its boundary)
    return states, (first + start_at).astype(np.int64), (first + end_at).astype(np.int64)


def notes_from_frames(ref_notes: Any, note_first: Any, note_after: Any, first_frame: Any, n_frames: int) -> np.ndarray:
    """The inverse: the notes on the audio's time base, rows of (start_s, end_s, pitch_midi).  start_s / end_s are the frame
    times (`frames_to_time_at`, the expression every event's start_s comes from) of the first frames of the note's first
    state and of the state after its last — of `n_frames` itself when no later state exists."""
    notes = _notes(ref_notes)
    ff = np.concatenate([np.asarray(first_frame, np.int64).reshape(-1), [int(n_frames)]])
    out = notes.copy()
    out[:, 0] = frames_to_time_at(ff[np.asarray(note_first, np.int64)])
    out[:, 1] = frames_to_time_at(ff[np.asarray(note_after, np.int64)])
    return out


def _maps(note: Any, onset: Any) -> Tuple[np.ndarray, np.ndarray]:
    n, o = np.require(note, np.float32, ["C"]), np.require(onset, np.float32, ["C"])
    if n.ndim != 2 or n.shape[1] != PITCHES or o.shape != n.shape:
        raise ValueError(f"note / onset: expected two (T, {PITCHES}) maps of one length")
    return n, o


def align_rows(note: Any, onset: Any, states: np.ndarray, params: Any = None, **fields: Any) -> Tuple[np.ndarray, int, int]:
    """The host checker (`bp_align_rows`) on one segment's (rows, 88) maps: (first_frame per state, total, status)."""
    lib = bind(_native.load_library())
    n, o = _maps(note, onset)
    st = np.ascontiguousarray(states, ALIGN_STATE)
    p = align_params(params, **fields)
    ff = np.full(max(1, len(st)), -1, np.int32)
    total, status = C.c_int64(0), C.c_int(0)
    rc = lib.bp_align_rows(n.ctypes.data if len(n) else None, o.ctypes.data if len(n) else None, len(n),
                           st.ctypes.data if len(st) else None, len(st), C.addressof(p), ff.ctypes.data, len(st), C.byref(total),
                           C.byref(status))
    if rc != _native.BP_OK:
        raise ValueError("bp_align_rows: rows without a state, more than 4096 states, a malformed bp_align_params (threshold_q "
                         "outside 0 ... 1024, onset_weight outside 0 ... 16, a non-zero reserved) or a malformed state (a bit at or "
                         "above 88, begins outside active, earliest below 0 or above latest)")
    return ff[: len(st)], int(total.value), int(status.value)


@dataclass
class Alignment:
    """The alignment of one segment.  `notes`: the reference notes on the audio's time base ((n, 3) rows of start_s, end_s,
    pitch_midi), None unless `status` is 0; `first_frame` per state (-1 unless status 0), `total` the path's gain; status 1: a
    NaN in the segment's maps, 2: infeasible (more states than rows, or windows that cannot be met)."""

    notes: Optional[np.ndarray]
    first_frame: np.ndarray
    total: int
    status: int
    states: np.ndarray
    note_first: np.ndarray
    note_after: np.ndarray


def _split_params(params: dict) -> Tuple[dict, dict]:
    for k in params:
        if k not in _PARAM_FIELDS + _STATE_FIELDS:
            raise TypeError(f"unknown parameter {k!r}: expected {list(_PARAM_FIELDS + _STATE_FIELDS)}")
    return {k: v for k, v in params.items() if k in _PARAM_FIELDS}, {k: v for k, v in params.items() if k in _STATE_FIELDS}


def _scores(ref_notes: Sequence[Any], rows: Sequence[int], how: dict):
    built = [states_from_notes(r, int(t), **how) for r, t in zip(ref_notes, rows)]
    flat = np.ascontiguousarray(np.concatenate([b[0] for b in built]) if built else np.zeros(0, ALIGN_STATE), ALIGN_STATE)
    return built, _jobs.offsets_of([len(b[0]) for b in built]), flat


def _align_call(model: Any, what: str, fixed: tuple, state_offsets: np.ndarray, states: np.ndarray, params: Any):
    """`what(*fixed, state_offsets, states, p, first_frame, max_states, total, status)` -> (first_frame, total, status)."""
    lib = bind(model._lib)
    p = align_params(params)
    n, n_states = len(state_offsets) - 1, int(state_offsets[-1])
    ff = np.full(max(1, n_states), -1, np.int32)
    total = np.zeros(max(1, n), np.int64)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, state_offsets.ctypes.data_as(_pi64), states.ctypes.data if n_states else None, C.addressof(p),
                            ff.ctypes.data, n_states, total.ctypes.data_as(_pi64), status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return ff[:n_states], total[:n], status[:n]


def align_from_maps(model: Any, row_offsets: Sequence[int], note: Any, onset: Any, mem_kind: int, state_offsets: Sequence[int],
                    states: np.ndarray, params: Any = None):
    """One `bp_align_from_maps` call: `note` / `onset` pointers (or None without rows) to the rows of all segments in host or
    device memory.  Returns (first_frame of all states, total per segment, status per segment)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (note, onset), mem_kind)
    return _align_call(model, "bp_align_from_maps", fixed, np.ascontiguousarray(state_offsets, np.int64),
                       np.ascontiguousarray(states, ALIGN_STATE), params)


def infer_clips_align(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, state_offsets: Sequence[int], states: np.ndarray,
                      params: Any = None):
    """One `bp_infer_clips_align` call for [n_frames, channels] arrays at one rate: (first_frame, total, status)."""
    return _align_call(model, "bp_infer_clips_align", _jobs.clips_source(model, arrays, sample_rate), np.ascontiguousarray(state_offsets, np.int64),
                       np.ascontiguousarray(states, ALIGN_STATE), params)


def _results(ref_notes, built, offs, rows, ff, total, status) -> List[Alignment]:
    out = []
    for i, (states, first, after) in enumerate(built):
        f = np.array(ff[int(offs[i]) : int(offs[i + 1])])
        ok = int(status[i]) == 0
        out.append(Alignment(notes_from_frames(ref_notes[i], first, after, f, int(rows[i])) if ok else None, f, int(total[i]),
                             int(status[i]), states, first, after))
    return out


def align(model: Any, outputs: Sequence[Any], ref_notes: Sequence[Any], **params: Any) -> List[Alignment]:
    """`Model.align`."""
    if len(outputs) != len(ref_notes):
        raise ValueError(f"align: {len(outputs)} segments but {len(ref_notes)} lists of reference notes")
    if not outputs:
        return []
    prm, how = _split_params(params)
    row_offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("note", "onset"), "align", mismatch="align: the note and onset maps of a "
                                                "segment must have one length and lie in one kind of memory")
    rows = np.diff(row_offs).tolist()
    built, offs, flat = _scores(ref_notes, rows, how)
    ff, total, status = align_from_maps(model, row_offs, ptr["note"], ptr["onset"], mem_kind, offs, flat, prm)
    return _results(ref_notes, built, offs, rows, ff, total, status)


def transcribe_clips_align(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], ref_notes: Sequence[Any],
                           **params: Any) -> List[Alignment]:
    """`Model.transcribe_clips_align`: the clips of each rate in one `bp_infer_clips_align` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    if len(arrays) != len(ref_notes):
        raise ValueError(f"transcribe_clips_align: {len(arrays)} clips but {len(ref_notes)} lists of reference notes")
    prm, how = _split_params(params)

    def run(ids, rate):
        mine = [arrays[i] for i in ids]
        rows = np.diff(_clips.clips_row_offsets(model, mine, rate))
        refs = [ref_notes[i] for i in ids]
        built, offs, flat = _scores(refs, rows, how)
        ff, total, status = infer_clips_align(model, mine, rate, offs, flat, prm)
        return _results(refs, built, offs, rows, ff, total, status)

    return _jobs.per_rate(_jobs.rates_of(arrays, sample_rates), run)
