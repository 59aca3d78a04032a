"""The same posteriorgrams decoded under many parameter sets in one device call (include/basic_pitch_amd_sweep.h).

Tuning thresholds, trying a frequency band, sweeping the minimum note length: the model's output does not change between
those decodes.  `bp_note_events_sweep` takes segments, parameter sets and a table of decodes (segment, set) and runs them all
in one call: the dense half of note decoding once per distinct dense key of the sets, the bend map once, the tracker as one
launch with a workgroup per decode (csrc/note_track.hip).  Decode by decode the results are those of
`bp_note_events_from_maps` on that segment alone with that set (tests/test_gpu_sweep.py).  `bp_infer_clips_events_sweep` is
the same behind the model, for PCM clips.  `Model.sweep_note_events` and `Model.transcribe_clips_sweep` are the public
entries; this module binds the prototypes and holds the host side.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import events as _events
from . import jobs as _jobs
from . import note_creation as _notes
from .jobs import cross_product, decode_table  # noqa: F401  (the decodes of a sweep, shared with the score calls)

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_sweep.h declares them (tests/test_sweep_cpu.py compares)
_OUT = [_vp, _i64, _vp, _i64, _pi64, _vp]  # events, max_events, bends, max_bends, event_offsets, status
PROTOTYPES = {
    "bp_note_events_sweep": (_int, [_vp, _i64, _pi64, _vp, _vp, _vp, _int, _i64, _vp, _i64, _vp] + _OUT),
    "bp_infer_clips_events_sweep": (_int, [_vp, _i64, _vp, _int, _int, _i64, _vp, _i64, _vp] + _OUT),
}

MAX_DECODES = 65536  # BP_SWEEP_MAX_DECODES
MAX_ROWS = 8388608   # BP_SWEEP_MAX_ROWS: rows over all decodes

Pair = Tuple[int, int]  # (segment, set)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_sweep.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def sets_array(params: Sequence[Any]):
    """The parameter sets as one `bp_note_params` array."""
    arr = (_native.bp_note_params * max(1, len(params)))()
    for i, p in enumerate(params):
        C.memmove(C.addressof(arr[i]), C.addressof(p), C.sizeof(_native.bp_note_params))
    return arr


def freq_limits(prm: Any) -> Tuple[int, int]:
    """The bins [lo, hi) `constrain_frequency` keeps (csrc/note_decode.cpp bp_internal_freq_limits): round-half-even of the
    frequency's MIDI number less 21, counted from the top when negative, clamped to 0 ... 88."""
    def norm(i: int) -> int:
        return max(0, i + 88) if i < 0 else min(i, 88)

    def index(hz: float) -> int:
        return round(12.0 * (math.log2(hz) - math.log2(440.0)) + 69.0 - 21)

    return (norm(index(prm.min_freq_hz)) if prm.min_freq_hz > 0.0 else 0,
            norm(index(prm.max_freq_hz)) if prm.max_freq_hz > 0.0 else 88)


def dense_key(prm: Any) -> Optional[Tuple[int, int, bool, float]]:
    """What the dense half of note decoding depends on: (lowest bin, end bin, infer_onsets, onset_threshold).  None for an
    onset threshold that is not above 0: such a set has no dense half (its decodes get status 1)."""
    if not prm.onset_threshold > 0.0:
        return None
    lo, hi = freq_limits(prm)
    return lo, hi, bool(prm.infer_onsets), float(prm.onset_threshold)


def dense_keys(params: Sequence[Any]) -> Tuple[List[Tuple[int, int, bool, float]], List[Optional[int]]]:
    """The distinct dense keys of `params`, in the order a sweep runs them (by band), and for each set the index of its key
    (None: no dense half).  The dense launches of a sweep grow with len(keys), not with the sets or the decodes."""
    of_set = [dense_key(p) for p in params]
    keys = sorted({k for k in of_set if k is not None})
    return keys, [keys.index(k) if k is not None else None for k in of_set]


def _call(model: Any, what: str, fixed: tuple, params: Sequence[Any], pairs: Optional[Sequence[Pair]], rows: Sequence[int],
          room: Optional[Tuple[int, int]]):
    """`what(*fixed, n_sets, sets, n_decodes, decodes, <outputs>)` with the grow-and-repeat loop of events._call: (events,
    bends, event_offsets, status per decode)."""
    lib = bind(model._lib)
    sets = sets_array(params)
    block, n_decodes = _jobs.decodes_block(sets, len(params), pairs, len(rows))
    total = sum(rows[s] for s, _ in pairs) if pairs is not None else len(params) * sum(rows)
    return _events._call(lib, model._handle, what, getattr(lib, what), fixed + block, n_decodes, int(total), room)


def note_events_sweep(model: Any, row_offsets: Sequence[int], note: Any, onset: Any, contour: Any, mem_kind: int,
                      params: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, room: Optional[Tuple[int, int]] = None):
    """One `bp_note_events_sweep` call: note / onset / contour are pointers (ints) to the maps of all segments, segment i at
    rows row_offsets[i]:row_offsets[i + 1]; `pairs` None is the cross product (`cross_product`).  Returns (events, bends,
    event_offsets, status per decode), decode j's events at event_offsets[j]:event_offsets[j + 1]."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (note, onset, contour), mem_kind)
    return _call(model, "bp_note_events_sweep", fixed, params, pairs, np.diff(offs).tolist(), room)


def infer_clips_events_sweep(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Sequence[Any],
                             pairs: Optional[Sequence[Pair]] = None, room: Optional[Tuple[int, int]] = None):
    """One `bp_infer_clips_events_sweep` call for [n_frames, channels] arrays at one rate; returns as `note_events_sweep`,
    a decode's segment being a clip."""
    rows = np.diff(_clips.clips_row_offsets(model, arrays, sample_rate)).tolist()
    return _call(model, "bp_infer_clips_events_sweep", _jobs.clips_source(model, arrays, sample_rate), params, pairs, rows, room)


def sweep_note_events(model: Any, outputs: Sequence[Dict[str, Any]], params: Sequence[Any],
                      pairs: Optional[Sequence[Pair]] = None):
    """`Model.sweep_note_events`: posteriorgram dicts (numpy arrays or CUDA tensors, all of one kind) under the sets `params`
    through one `bp_note_events_sweep` call.  Without `pairs`: result[set][segment] = (events | None, status); with `pairs`,
    a list of (segment, set): one such tuple per pair.  events is None where the status is 1 or 2."""
    n_seg, n_sets = len(outputs), len(params)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "sweep_note_events")
    flat: List[Tuple[Optional[List[Any]], int]] = []
    if todo:
        offs, maps, ptr, mem_kind = _events.stack_maps(outputs, "sweep_note_events")
        events, bends, ev_offs, status = note_events_sweep(model, offs, ptr["note"], ptr["onset"], ptr["contour"], mem_kind,
                                                           params, pairs)
        flat = [(_events.clip_events(events, bends, ev_offs, j, bool(params[p].include_pitch_bends)) if not status[j] else None,
                 int(status[j])) for j, (_, p) in enumerate(todo)]
    if pairs is not None:
        return flat
    return [flat[p * n_seg : (p + 1) * n_seg] for p in range(n_sets)]


def _host_events(model: Any, a: np.ndarray, rate: int, prm: Any) -> List["_notes.NoteEvent"]:
    """A clip under one set by the route that takes every input: the model, then the host decoder on its maps."""
    out = model.predict_pcm_raw(a, _clips.FORMATS[a.dtype], a.shape[0], a.shape[1], rate)
    return _jobs.host_decode([np.require(out[k], np.float32, ["C", "W"] if k != "contour" else ["C"])
                              for k in ("note", "onset", "contour")], prm)


def transcribe_clips_sweep(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Sequence[Any]
                           ) -> List[List[List["_notes.NoteEvent"]]]:
    """`Model.transcribe_clips_sweep`: result[set][clip] = the note events of that clip under that set.  The clips of a rate
    go through the model ONCE (`bp_infer_clips_events_sweep`) whatever the number of sets; a decode with a non-zero status is
    finished for that clip and set alone by the model and the host decoder, as `transcribe_clips(decode="device")` finishes
    such clips: the result is always complete."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    results: List[List[Any]] = [[None] * len(arrays) for _ in params]
    if not params:
        return results
    for rate, ids in _jobs.rate_groups(rates):
        group = [arrays[i] for i in ids]
        events, bends, ev_offs, status = infer_clips_events_sweep(model, group, rate, params)
        for j, (k, p) in enumerate(cross_product(len(params), len(ids))):
            with_bends = bool(params[p].include_pitch_bends)
            if not status[j]:
                results[p][ids[k]] = _events.clip_events(events, bends, ev_offs, j, with_bends)
                continue
            results[p][ids[k]] = _host_events(model, group[k], rate, params[p])  # 1: a NaN or no onset threshold; 2: capacity
    return results
