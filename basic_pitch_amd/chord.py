"""Chords and key (include/basic_pitch_amd_chord.h): which chord sounds in every row of a segment and what key it is in, from
the note posteriorgram alone.

The note rows become a chroma per frame, the chroma sums per unit (a frame, or the stretch between two boundaries such as
beats), the units a path over a table of chord templates by a Viterbi recurrence with one switching penalty, and the summed
chroma a key by profile correlation, all in exact integers (`chord_rows_raw` is the host checker `bp_chord_rows`; `Model.chords`
and `Model.transcribe_clips_chords` run many segments on the device, csrc/chord.hip).  The definition is this project's own:
unpinned against any third-party chord or key estimator.  The beats of `Model.beats` go in as they are:

    out = model.predict(audio)
    chords = model.chords([out], beats=model.beats([out]))[0]
    chord.write_lab("song.lab", chords)                    # start end name, one run a line
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

# name -> (restype, argtypes), as include/basic_pitch_amd_chord.h declares them (tests/test_chord_cpu.py compares)
_TAIL = [_vp, _pi64, _vp, _vp, _vp, _i64]  # p, bound_offsets, bounds, summaries, labels, max_labels
PROTOTYPES = {
    "bp_chord_params_default": (None, [_vp]),
    "bp_chord_templates": (_int, [_int, _vp]),
    "bp_chord_key_profiles": (_int, [_vp]),
    "bp_chord_rows": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "bp_chords_from_maps": (_int, [_vp, _i64, _pi64, _vp, _int] + _TAIL),
    "bp_infer_clips_chords": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

PITCHES = 88                 # BP_CHORD_PITCHES
CLASSES = 12                 # BP_CHORD_CLASSES
MAX_STATES = 64              # BP_CHORD_MAX_STATES
Q_ONE = 1024                 # BP_CHORD_Q_ONE
MAX_WEIGHT = 1024            # BP_CHORD_MAX_WEIGHT
MAX_PENALTY = 1024           # BP_CHORD_MAX_PENALTY
MAX_ROWS = 524288            # BP_CHORD_MAX_ROWS
CHROMA_ROWS = 32             # BP_CHORD_CHROMA_ROWS
TRACE_TILE = 512             # BP_CHORD_TRACE_TILE
PATH_WAVES = 4               # BP_CHORD_PATH_WAVES
# bp_chord_summary, 32 bytes
CHORD_SUMMARY = np.dtype([("status", np.int32), ("key", np.int32), ("n_units", np.int32), ("n_changes", np.int32),
                          ("score", np.int64), ("key_score", np.int64)])
_PARAM_FIELDS = ("threshold_q", "min_pitch", "max_pitch", "n_states", "switch_penalty", "reserved", "bias", "weights", "key_profile")
NOTE_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
# vocabulary -> (BP_CHORD_VOCAB_*, its qualities in the table's order)
VOCABULARIES = {"majmin": (0, ("maj", "min")), "triads": (1, ("maj", "min", "dim", "aug")), "sevenths": (2, ("maj", "min", "7", "maj7", "min7"))}
KEY_NAMES = tuple(f"{n} major" for n in NOTE_NAMES) + tuple(f"{n} minor" for n in NOTE_NAMES)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_chord.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def chord_names(vocabulary: str = "majmin") -> List[str]:
    """The names of a vocabulary's states in table order: N, then quality-major, root ascending from C ("C:maj", "A:min", "G:7")."""
    if vocabulary not in VOCABULARIES:
        raise ValueError(f"vocabulary: expected one of {list(VOCABULARIES)}")
    return ["N"] + [f"{root}:{quality}" for quality in VOCABULARIES[vocabulary][1] for root in NOTE_NAMES]


def chord_params(params: Any = None, **fields: Any) -> "_native.bp_chord_params":
    """`bp_chord_params`: the defaults (`bp_chord_params_default`: threshold_q 307, pitches 0 ... 87, switch_penalty 128, the
    majmin table, the Krumhansl-Kessler profiles), a given record as it is, or a dict / keyword fields on top of the defaults.
    `vocabulary`: "majmin", "triads" or "sevenths" (`bp_chord_templates`) instead of n_states / bias / weights.  The record
    carries the names of its states as `names` (a table of one's own: "N", "1", "2", ... unless `names` is given)."""
    if isinstance(params, _native.bp_chord_params):
        return params
    lib = bind(_native.load_library())
    p = _native.bp_chord_params()
    lib.bp_chord_params_default(C.addressof(p))
    given = dict(params or {}, **fields)
    for k in given:
        if k not in _PARAM_FIELDS + ("vocabulary", "names"):
            raise TypeError(f"unknown field {k!r}: bp_chord_params has {list(_PARAM_FIELDS)}, and 'vocabulary' names a table")
    own_table = any(k in given for k in ("n_states", "bias", "weights"))
    if "vocabulary" in given and own_table:
        raise TypeError("give a vocabulary or n_states / bias / weights, not both")
    vocabulary = given.pop("vocabulary", "majmin")
    names = given.pop("names", None)
    if vocabulary not in VOCABULARIES:
        raise ValueError(f"vocabulary: expected one of {list(VOCABULARIES)}")
    if lib.bp_chord_templates(VOCABULARIES[vocabulary][0], C.addressof(p)) != _native.BP_OK:
        raise ValueError("bp_chord_templates: unknown vocabulary")
    for k, v in given.items():
        if k == "reserved":
            for i, x in enumerate([int(v), 0, 0] if np.isscalar(v) else list(v)):
                p.reserved[i] = int(x)
        elif k in ("bias", "weights", "key_profile"):
            dst = np.ctypeslib.as_array(getattr(p, k))
            src = np.asarray(v, np.int64)
            part = dst[tuple(slice(0, n) for n in src.shape)] if src.ndim == dst.ndim else None
            if part is None or part.shape != src.shape:
                raise ValueError(f"{k}: expected at most {dst.shape} entries")
            dst[...] = 0
            part[...] = src
        else:
            setattr(p, k, int(v))
    p.names = list(names) if names is not None else (["N"] + [str(s) for s in range(1, 64)] if own_table else chord_names(vocabulary))
    return p


def _names(p: Any) -> List[str]:
    return list(getattr(p, "names", None) or ["N"] + [str(s) for s in range(1, 64)])


def _note(note: Any) -> np.ndarray:
    o = np.require(note, np.float32, ["C"])
    if o.ndim != 2 or o.shape[1] != PITCHES:
        raise ValueError(f"note: expected a (T, {PITCHES}) map")
    return o


def _boundaries(b: Any) -> np.ndarray:
    """The boundary frames of one segment as int32: a `beat.Beats` (its frames), an array, or None.  A beat at frame 0 is no
    boundary and is dropped."""
    if b is None:
        return np.zeros(0, np.int32)
    frames = np.ascontiguousarray(getattr(b, "frames", b), np.int32).reshape(-1)
    return np.ascontiguousarray(frames[frames != 0])


def chord_rows_raw(note: Any, params: Any = None, bounds: Any = None, **fields: Any) -> Tuple[np.ndarray, np.ndarray]:
    """The host checker (`bp_chord_rows`) on one segment's (rows, 88) note map: (the `CHORD_SUMMARY` record as an array of
    one, the labels as one uint8 per row).  `bounds`: the boundary frames, strictly ascending inside 0 < B < rows."""
    lib = bind(_native.load_library())
    o = _note(note)
    p = chord_params(params, **fields)
    b = np.ascontiguousarray(bounds if bounds is not None else [], np.int32).reshape(-1)
    labels = np.zeros(max(1, len(o)), np.uint8)
    summary = np.zeros(1, CHORD_SUMMARY)
    rc = lib.bp_chord_rows(o.ctypes.data if len(o) else None, len(o), C.addressof(p), b.ctypes.data if len(b) else None, len(b),
                           labels.ctypes.data, len(o), summary.ctypes.data)
    if rc != _native.BP_OK:
        raise ValueError("bp_chord_rows: more than 524288 rows, boundaries that are not strictly ascending inside 0 < B < rows, or a "
                         "malformed bp_chord_params (threshold_q outside 0 ... 1024, pitches outside 0 <= min_pitch <= max_pitch <= 87, "
                         "n_states outside 1 ... 64, switch_penalty outside 0 ... 1024, a bias, weight or profile entry outside "
                         "-1024 ... 1024, a non-zero reserved word)")
    return summary, labels[: len(o)].copy()


@dataclass
class Chords:
    """Chords and key of one segment.  `labels`: the state of every row (uint8); `runs`: the maximal runs of one state as
    (start_frame, end_frame, name), end exclusive; `times_s`: (runs, 2) start and end of every run in seconds (the expression
    every event's start_s comes from); `key`: "C major" ... "B minor", None unless `status` is 0; `key_index` 0 ... 23 or -1;
    `score` the final D and `key_score` K[key]; status 1: a NaN in the segment's note rows, 2: nothing sounds."""

    labels: np.ndarray
    runs: List[Tuple[int, int, str]]
    times_s: np.ndarray
    key: Optional[str]
    status: int
    key_index: int
    n_units: int
    n_changes: int
    score: int
    key_score: int

    @classmethod
    def of(cls, summary: Any, labels: np.ndarray, names: Sequence[str]) -> "Chords":
        labels = np.ascontiguousarray(labels, np.uint8)
        edges = np.concatenate([[0], np.flatnonzero(np.diff(labels)) + 1, [len(labels)]]).astype(np.int64) if len(labels) else np.zeros(1, np.int64)
        runs = [(int(s), int(e), names[int(labels[s])]) for s, e in zip(edges[:-1], edges[1:])]
        times = np.stack([frames_to_time_at(edges[:-1]), frames_to_time_at(edges[1:])], axis=1) if runs else np.zeros((0, 2))
        key = int(summary["key"])
        return cls(labels, runs, times, KEY_NAMES[key] if int(summary["status"]) == 0 and key >= 0 else None, int(summary["status"]), key,
                   int(summary["n_units"]), int(summary["n_changes"]), int(summary["score"]), int(summary["key_score"]))


def chord_rows(note: Any, params: Any = None, bounds: Any = None, **fields: Any) -> Chords:
    """The host checker on one segment's (rows, 88) note map, as a `Chords`."""
    p = chord_params(params, **fields)
    summary, labels = chord_rows_raw(note, p, _boundaries(bounds))
    return Chords.of(summary[0], labels, _names(p))


def write_lab(path: str, chords: Chords) -> None:
    """The runs as `start end name` lines, seconds with six decimals: the .lab format chord annotations come in."""
    with open(path, "w") as f:
        for (start, end), (_, _, name) in zip(chords.times_s, chords.runs):
            f.write(f"{start:.6f} {end:.6f} {name}\n")


def _bound_arrays(bounds: Optional[Sequence[Any]], n: int):
    """(bound_offsets as int64 [n + 1], bounds as int32) of per-segment boundary lists, or (None, None) without any."""
    if bounds is None:
        return None, None
    if len(bounds) != n:
        raise ValueError(f"bounds: expected one list of boundaries per segment ({n}), got {len(bounds)}")
    parts = [_boundaries(b) for b in bounds]
    flat = np.concatenate(parts + [np.zeros(0, np.int32)]).astype(np.int32)
    return _jobs.offsets_of([len(b) for b in parts]), (flat if len(flat) else np.zeros(1, np.int32))


def _chord_call(model: Any, what: str, fixed: tuple, rows: Sequence[int], params: Any, bounds: Optional[Sequence[Any]]):
    """`what(*fixed, p, bound_offsets, bounds, summaries, labels, max_labels)` -> (summaries, labels of all rows)."""
    lib = bind(model._lib)
    p = chord_params(params)
    n = len(rows)
    total = int(sum(int(r) for r in rows))
    summaries = np.zeros(max(1, n), CHORD_SUMMARY)
    labels = np.zeros(max(1, total), np.uint8)
    offs, flat = _bound_arrays(bounds, n)
    rc = getattr(lib, what)(*fixed, C.addressof(p), offs.ctypes.data_as(_pi64) if offs is not None else None,
                            flat.ctypes.data if flat is not None else None, summaries.ctypes.data, labels.ctypes.data, total)
    _native.check(lib, model._handle, rc, what)
    return summaries[:n], labels[:total]


def chords_from_maps(model: Any, row_offsets: Sequence[int], note: Any, mem_kind: int, params: Any = None,
                     bounds: Optional[Sequence[Any]] = None):
    """One `bp_chords_from_maps` call: `note` a pointer (or None without rows) to the note rows of all segments in host or
    device memory, `bounds` per segment its boundary frames (None: frame units everywhere).  Returns (`CHORD_SUMMARY` records
    per segment, the labels of all rows)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (note,), mem_kind)
    return _chord_call(model, "bp_chords_from_maps", fixed, np.diff(offs), params, bounds)


def infer_clips_chords(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Any = None,
                       bounds: Optional[Sequence[Any]] = None):
    """One `bp_infer_clips_chords` call for [n_frames, channels] arrays at one rate: (summaries, labels, row_offsets)."""
    offs = _clips.clips_row_offsets(model, arrays, sample_rate) if len(arrays) else np.zeros(1, np.int64)
    fixed = _jobs.clips_source(model, arrays, sample_rate)
    return _chord_call(model, "bp_infer_clips_chords", fixed, np.diff(offs), params, bounds) + (np.asarray(offs, np.int64),)


def _results(summaries: np.ndarray, labels: np.ndarray, offs: np.ndarray, names: Sequence[str]) -> List[Chords]:
    return [Chords.of(s, np.array(labels[int(offs[i]) : int(offs[i + 1])]), names) for i, s in enumerate(summaries)]


def chords(model: Any, outputs: Sequence[Any], params: Any = None, beats: Optional[Sequence[Any]] = None) -> List[Chords]:
    """`Model.chords`."""
    if not outputs:
        return []
    p = chord_params(params)
    offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("note",), "chords")
    return _results(*chords_from_maps(model, offs, ptr["note"], mem_kind, p, beats), offs, _names(p))


def transcribe_clips_chords(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None,
                            bounds: Optional[Sequence[Any]] = None) -> List[Chords]:
    """`Model.transcribe_clips_chords`: the clips of each rate in one `bp_infer_clips_chords` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    if bounds is not None and len(bounds) != len(arrays):
        raise ValueError(f"bounds: expected one list of boundaries per clip ({len(arrays)}), got {len(bounds)}")
    p = chord_params(params)

    def run(ids, rate):
        got = infer_clips_chords(model, [arrays[i] for i in ids], rate, p, None if bounds is None else [bounds[i] for i in ids])
        return _results(*got, _names(p))

    return _jobs.per_rate(rates, run)
