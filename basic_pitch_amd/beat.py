"""Tempo and beats (include/basic_pitch_amd_beat.h): where the pulse of a segment lies and how fast it is, from the onset
posteriorgram alone.

The onset rows become a strength per frame, the strengths one period by autocorrelation under a log-normal tempo prior, and the
period a beat path by a dynamic programme over frames, all in exact integers (`beat_rows` is the host checker `bp_beat_rows`;
`Model.beats` and `Model.transcribe_clips_beats` run many segments on the device, csrc/beat.hip).  The definition is this
project's own, after Ellis 2007: unpinned against librosa and mir_eval.  A `Beats.bpm` can be handed to the existing
`midi_tempo` arguments as it is:

    tempo = model.beats([output])[0]                       # `output`: the dict `predict` / `run_inference` returns
    midi, events = note_creation.model_output_to_notes(output, 0.5, 0.3, midi_tempo=tempo.bpm if tempo.status == 0 else 120)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, List, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import jobs as _jobs
from .note_creation import frames_to_time_at

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_beat.h declares them (tests/test_beat_cpu.py compares)
_TAIL = [_vp, _vp, _vp, _i64, _pi64]  # p, summaries, beats, max_beats, beat_offsets
PROTOTYPES = {
    "bp_beat_params_default": (None, [_vp]),
    "bp_beat_prior": (_int, [C.c_double, C.c_double, _vp]),
    "bp_beats_capacity": (_i64, [_i64, C.c_int32]),
    "bp_beat_rows": (_int, [_vp, _i64, _vp, _vp, _i64, _vp]),
    "bp_beats_from_maps": (_int, [_vp, _i64, _pi64, _vp, _int] + _TAIL),
    "bp_infer_clips_beats": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

PITCHES = 88                 # BP_BEAT_PITCHES
Q_ONE = 1024                 # BP_BEAT_Q_ONE
MAX_LAG = 256                # BP_BEAT_MAX_LAG
MAX_TIGHTNESS = 1024         # BP_BEAT_MAX_TIGHTNESS
MAX_ROWS = 524288            # BP_BEAT_MAX_ROWS
RING = 1024                  # BP_BEAT_RING
TEMPO_ROWS = 256             # BP_BEAT_TEMPO_ROWS
TEMPO_LAGS = 64              # BP_BEAT_TEMPO_LAGS
PATH_WAVES = 16              # BP_BEAT_PATH_WAVES
FRAMES_PER_MINUTE = 60.0 * 22050.0 / 256.0
# bp_beat_summary, 32 bytes
BEAT_SUMMARY = np.dtype([("status", np.int32), ("period", np.int32), ("n_beats", np.int64), ("score", np.int64),
                         ("period_refined", np.float64)])
_PARAM_FIELDS = ("threshold_q", "min_pitch", "max_pitch", "lag_min", "lag_max", "tightness", "reserved", "prior", "reserved_tail")
_PRIOR_FIELDS = ("start_bpm", "sd_octaves")


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_beat.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def beat_prior(start_bpm: float = 120.0, sd_octaves: float = 1.0) -> np.ndarray:
    """`bp_beat_prior`: the log-normal table prior[0 ... 256], int32 values 0 ... 1024."""
    table = np.zeros(MAX_LAG + 1, np.int32)
    if bind(_native.load_library()).bp_beat_prior(float(start_bpm), float(sd_octaves), table.ctypes.data) != _native.BP_OK:
        raise ValueError("bp_beat_prior: start_bpm and sd_octaves must be finite and above 0")
    return table


def beats_capacity(rows: int, lag_min: int) -> int:
    """`bp_beats_capacity`: the most beats a segment of `rows` rows can have, from the rows and lag_min alone."""
    cap = int(bind(_native.load_library()).bp_beats_capacity(int(rows), int(lag_min)))
    if cap < 0:
        raise ValueError("bp_beats_capacity: negative rows, or lag_min outside 2 ... 256")
    return cap


def beat_params(params: Any = None, **fields: Any) -> "_native.bp_beat_params":
    """`bp_beat_params`: the defaults (`bp_beat_params_default`: threshold_q 307, pitches 0 ... 87, lags 21 ... 172, tightness
    4, the prior of 120 beats a minute one octave wide), a given record as it is, or a dict / keyword fields on top of the
    defaults.  `prior`: the 257 table entries; `start_bpm` / `sd_octaves`: a table from `bp_beat_prior` instead."""
    if isinstance(params, _native.bp_beat_params):
        return params
    p = _native.bp_beat_params()
    bind(_native.load_library()).bp_beat_params_default(C.addressof(p))
    given = dict(params or {}, **fields)
    for k in given:
        if k not in _PARAM_FIELDS + _PRIOR_FIELDS:
            raise TypeError(f"unknown field {k!r}: bp_beat_params has {list(_PARAM_FIELDS)}, and {list(_PRIOR_FIELDS)} make a prior")
    if "prior" in given and any(k in given for k in _PRIOR_FIELDS):
        raise TypeError("give a prior table or start_bpm / sd_octaves, not both")
    if any(k in given for k in _PRIOR_FIELDS):
        given["prior"] = beat_prior(given.pop("start_bpm", 120.0), given.pop("sd_octaves", 1.0))
    for k, v in given.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(v), 0) if np.isscalar(v) else (int(v[0]), int(v[1]))
        elif k == "prior":
            table = np.asarray(v).reshape(-1)
            if len(table) != MAX_LAG + 1:
                raise ValueError(f"prior: expected {MAX_LAG + 1} entries")
            for i, x in enumerate(table):
                p.prior[i] = int(x)
        else:
            setattr(p, k, int(v))
    return p


def _onset(onset: Any) -> np.ndarray:
    o = np.require(onset, np.float32, ["C"])
    if o.ndim != 2 or o.shape[1] != PITCHES:
        raise ValueError(f"onset: expected a (T, {PITCHES}) map")
    return o


def beat_rows_raw(onset: Any, params: Any = None, **fields: Any) -> Tuple[np.ndarray, np.ndarray]:
    """The host checker (`bp_beat_rows`) on one segment's (rows, 88) onset map: (the `BEAT_SUMMARY` record as an array of one,
    the beats as int32 frames)."""
    lib = bind(_native.load_library())
    o = _onset(onset)
    p = beat_params(params, **fields)
    cap = int(lib.bp_beats_capacity(len(o), p.lag_min))
    beats = np.zeros(max(1, cap), np.int32)
    summary = np.zeros(1, BEAT_SUMMARY)
    rc = lib.bp_beat_rows(o.ctypes.data if len(o) else None, len(o), C.addressof(p), beats.ctypes.data, max(0, cap), summary.ctypes.data)
    if rc != _native.BP_OK:
        raise ValueError("bp_beat_rows: more than 524288 rows or a malformed bp_beat_params (threshold_q outside 0 ... 1024, pitches "
                         "outside 0 <= min_pitch <= max_pitch <= 87, lags outside 2 <= lag_min <= lag_max <= 256, tightness outside "
                         "0 ... 1024, a prior entry outside 0 ... 1024, a non-zero reserved word)")
    return summary, beats[: int(summary["n_beats"][0])].copy()


@dataclass
class Beats:
    """Tempo and beats of one segment.  `frames`: the beats as ascending int32 frame indices; `times_s` their times (the
    expression every event's start_s comes from); `period_frames` the refined period and `bpm` = 60 * 22050 / 256 / period_frames
    (0.0 both unless `status` is 0); `period` the integer period and `score` its S[P]; status 1: a NaN in the segment's onset
    rows, 2: no pulse (too few rows, silence, everything under the threshold)."""

    frames: np.ndarray
    times_s: np.ndarray
    period_frames: float
    bpm: float
    status: int
    period: int
    score: int

    @classmethod
    def of(cls, summary: Any, frames: np.ndarray) -> "Beats":
        frames = np.ascontiguousarray(frames, np.int32)
        refined = float(summary["period_refined"])
        return cls(frames, frames_to_time_at(frames), refined, FRAMES_PER_MINUTE / refined if refined > 0.0 else 0.0,
                   int(summary["status"]), int(summary["period"]), int(summary["score"]))


def beat_rows(onset: Any, params: Any = None, **fields: Any) -> Beats:
    """The host checker on one segment's (rows, 88) onset map, as a `Beats`."""
    summary, frames = beat_rows_raw(onset, params, **fields)
    return Beats.of(summary[0], frames)


def _beat_call(model: Any, what: str, fixed: tuple, rows: Sequence[int], params: Any) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`what(*fixed, p, summaries, beats, max_beats, beat_offsets)` -> (summaries, beats, beat_offsets)."""
    lib = bind(model._lib)
    p = beat_params(params)
    n = len(rows)
    room = sum(max(0, int(lib.bp_beats_capacity(int(r), p.lag_min))) for r in rows)
    summaries = np.zeros(max(1, n), BEAT_SUMMARY)
    beats = np.zeros(max(1, room), np.int32)
    offsets = np.zeros(n + 1, np.int64)
    rc = getattr(lib, what)(*fixed, C.addressof(p), summaries.ctypes.data, beats.ctypes.data, room, offsets.ctypes.data_as(_pi64))
    _native.check(lib, model._handle, rc, what)
    return summaries[:n], beats[: int(offsets[n])], offsets


def beats_from_maps(model: Any, row_offsets: Sequence[int], onset: Any, mem_kind: int, params: Any = None):
    """One `bp_beats_from_maps` call: `onset` a pointer (or None without rows) to the onset rows of all segments in host or
    device memory.  Returns (`BEAT_SUMMARY` records per segment, the beats of all segments, beat_offsets)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (onset,), mem_kind)
    return _beat_call(model, "bp_beats_from_maps", fixed, np.diff(offs), params)


def infer_clips_beats(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Any = None):
    """One `bp_infer_clips_beats` call for [n_frames, channels] arrays at one rate: (summaries, beats, beat_offsets)."""
    rows = np.diff(_clips.clips_row_offsets(model, arrays, sample_rate)) if len(arrays) else []
    return _beat_call(model, "bp_infer_clips_beats", _jobs.clips_source(model, arrays, sample_rate), rows, params)


def _results(summaries: np.ndarray, beats: np.ndarray, offsets: np.ndarray) -> List[Beats]:
    return [Beats.of(s, np.array(beats[int(offsets[i]) : int(offsets[i + 1])])) for i, s in enumerate(summaries)]


def beats(model: Any, outputs: Sequence[Any], params: Any = None) -> List[Beats]:
    """`Model.beats`."""
    if not outputs:
        return []
    offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("onset",), "beats")
    return _results(*beats_from_maps(model, offs, ptr["onset"], mem_kind, params))


def transcribe_clips_beats(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None) -> List[Beats]:
    """`Model.transcribe_clips_beats`: the clips of each rate in one `bp_infer_clips_beats` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    return _jobs.per_rate(_jobs.rates_of(arrays, sample_rates),
                          lambda ids, rate: _results(*infer_clips_beats(model, [arrays[i] for i in ids], rate, params)))
