"""The melody of the contour posteriorgram (include/basic_pitch_amd_melody.h): one f0 track with voiced / unvoiced decisions.

The track is the best path of a Viterbi recurrence over the frames of a segment: the states are the bins of a band and an
unvoiced state, moving costs a penalty per bin, switching between voiced and unvoiced a voicing penalty.  `melody_rows` is the
host checker (`bp_melody_rows`), `score_melody_frames` the counts the melody measures are formed from
(`bp_score_melody_frames`) and `measures` the five ratios; `Model.melody` and `Model.transcribe_clips_melody` decode many
segments on the device (csrc/melody.hip, a workgroup per decode), and `Model.sweep_melody_scores` /
`Model.transcribe_clips_sweep_melody_scores` score a sweep of parameter sets there, so that 52 bytes per decode come home.
The definition is this project's own and the measures restate `mir_eval.melody` for one time base: both are unpinned against
third-party code.  Hz are formed here, in numpy: the library produces MIDI pitches alone.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import jobs as _jobs
from . import score as _score
from .multipitch import BINS, midi_to_hz
from .note_creation import frames_to_time_at

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_melody.h declares them (tests/test_melody_cpu.py compares)
_OUT = [_vp, _vp, _i64, _vp]  # p, points, max_points, status
_TAIL = [_i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]  # n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status
PROTOTYPES = {
    "bp_melody_params_default": (None, [_vp]),
    "bp_melody_rows": (_int, [_vp, _i64, _vp, _vp, _i64, _vp]),
    "bp_score_melody_frames": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "bp_melody_from_maps": (_int, [_vp, _i64, _pi64, _vp, _int] + _OUT),
    "bp_infer_clips_melody": (_int, [_vp, _i64, _vp, _int, _int] + _OUT),
    "bp_melody_sweep_score": (_int, [_vp, _i64, _pi64, _vp, _int] + _TAIL),
    "bp_infer_clips_melody_sweep_score": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

MAX_JUMP = 16       # BP_MELODY_MAX_JUMP
READ_AHEAD = 8      # BP_MELODY_READ_AHEAD
TILE_ROWS = 128     # BP_MELODY_TILE_ROWS
PRED_STRIDE = 272   # BP_MELODY_PRED_STRIDE
MELODY_POINT = np.dtype([("bin", np.int32), ("salience", np.float32), ("pitch_midi", np.float64)])  # bp_melody_point, 16 bytes
_FIELDS = ("n_frames", "ref_voiced", "est_voiced", "both_voiced", "pitch_ok", "chroma_ok")  # bp_melody_score
MELODY_COUNTS = np.dtype([(name, np.int64) for name in _FIELDS] + [("status", np.int32)])

Pair = Tuple[int, int]  # (segment, set)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_melody.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def melody_params(params: Any = None, **fields: Any) -> "_native.bp_melody_params":
    """`bp_melody_params`: the defaults (`bp_melody_params_default`: threshold 0.3, jump penalty 0.05, voicing penalty 0.5,
    jumps of up to 4 bins, all 264 bins), a given record as it is, or a dict / keyword fields on top of the defaults."""
    if isinstance(params, _native.bp_melody_params):
        return params
    p = _native.bp_melody_params()
    bind(_native.load_library()).bp_melody_params_default(C.addressof(p))
    given = dict(params or {}, **fields)
    names = {n for n, _ in _native.bp_melody_params._fields_}
    for k, v in given.items():
        if k not in names:
            raise TypeError(f"unknown field {k!r}: bp_melody_params has {sorted(names)}")
        if k == "reserved":
            p.reserved[0], p.reserved[1] = (int(v), 0) if np.isscalar(v) else (int(v[0]), int(v[1]))
        else:
            setattr(p, k, float(v) if k in ("threshold", "jump_penalty", "voicing_penalty") else int(v))
    return p


def sets_array(params: Sequence[Any]):
    arr = (_native.bp_melody_params * max(1, len(params)))()
    for i, p in enumerate(params):
        q = melody_params(p)
        C.memmove(C.addressof(arr[i]), C.addressof(q), C.sizeof(_native.bp_melody_params))
    return arr


@dataclass
class Melody:
    """The melody of one segment: one entry per row.  Unvoiced rows have bin -1, pitch_midi, salience and freqs_hz 0.
    `status` 1: a NaN or a magnitude above 65536 in the segment's contour rows, and every row unvoiced."""

    bins: np.ndarray        # int32, -1 unvoiced
    times_s: np.ndarray     # float64, model_frames_to_time(rows)
    pitch_midi: np.ndarray  # float64, fractional
    salience: np.ndarray    # float32, the contour cell on the path
    freqs_hz: np.ndarray    # float64, midi_to_hz(pitch_midi) where voiced, 0.0 elsewhere
    voiced: np.ndarray      # bool
    status: int = 0

    @classmethod
    def from_points(cls, points: np.ndarray, status: int = 0) -> "Melody":
        bins = np.ascontiguousarray(points["bin"])
        pitch = np.ascontiguousarray(points["pitch_midi"])
        voiced = bins >= 0
        return cls(bins, frames_to_time_at(np.arange(len(bins))), pitch, np.ascontiguousarray(points["salience"]),
                   np.where(voiced, midi_to_hz(pitch), 0.0), voiced, int(status))


def melody_rows(contour: Any, params: Any = None) -> Tuple[np.ndarray, int]:
    """The host checker (`bp_melody_rows`) on one segment's (rows, 264) contour map: (`MELODY_POINT` record per row, status)."""
    lib = bind(_native.load_library())
    c = np.require(contour, np.float32, ["C"])
    if c.ndim != 2 or c.shape[1] != BINS:
        raise ValueError(f"contour: expected (T, {BINS})")
    p = melody_params(params)
    status = C.c_int(0)
    points = np.zeros(max(1, len(c)), MELODY_POINT)
    rc = lib.bp_melody_rows(c.ctypes.data, len(c), C.addressof(p), points.ctypes.data, len(c), C.byref(status))
    if rc != _native.BP_OK:
        raise ValueError("bp_melody_rows: a malformed bp_melody_params (a threshold that is not finite or beyond +-65536, a penalty "
                         "outside 0 ... 65536, max_jump outside 0 ... 16, a band outside 0 <= min_bin <= max_bin <= 263 or a non-zero "
                         "reserved)")
    return points[: len(c)], int(status.value)


def _counts_record(values: Sequence[int], status: int = 0) -> np.ndarray:
    return np.array(tuple(int(v) for v in values) + (int(status),), MELODY_COUNTS)


def score_melody_frames(points: np.ndarray, ref_pitch: Any, **tolerances: Any) -> np.ndarray:
    """The host checker (`bp_score_melody_frames`): the counts of one segment's `MELODY_POINT` records against `ref_pitch` (a
    MIDI pitch per row, 0.0 unvoiced), as one record of `MELODY_COUNTS`, status 0."""
    lib = bind(_native.load_library())
    pts = np.ascontiguousarray(points, MELODY_POINT)
    ref = np.ascontiguousarray(ref_pitch, np.float64)
    if ref.shape != (len(pts),):
        raise ValueError(f"ref_pitch: expected one entry per row ({len(pts)}), got {ref.shape}")
    p = _score.score_params(**tolerances)
    out = _native.bp_melody_score()
    rc = lib.bp_score_melody_frames(pts.ctypes.data if len(pts) else None, ref.ctypes.data if len(ref) else None, len(pts),
                                    C.addressof(p), C.addressof(out))
    if rc != _native.BP_OK:
        raise ValueError("bp_score_melody_frames: a ref_pitch entry that is negative or not finite, a voiced record with a non-finite "
                         "pitch, a negative or non-finite tolerance, or a non-zero reserved")
    return _counts_record([getattr(out, name) for name in _FIELDS])


def measures(counts: Any) -> Dict[str, Any]:
    """The melody measures from `MELODY_COUNTS` records (any shape): voicing_recall, voicing_false_alarm, raw_pitch_accuracy,
    raw_chroma_accuracy, overall_accuracy, float64; a zero denominator gives 0.0."""
    c = {name: np.asarray(counts[name], np.float64) for name in _FIELDS}

    def ratio(num, den):
        return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)

    return {
        "voicing_recall": ratio(c["both_voiced"], c["ref_voiced"]),
        "voicing_false_alarm": ratio(c["est_voiced"] - c["both_voiced"], c["n_frames"] - c["ref_voiced"]),
        "raw_pitch_accuracy": ratio(c["pitch_ok"], c["ref_voiced"]),
        "raw_chroma_accuracy": ratio(c["chroma_ok"], c["ref_voiced"]),
        "overall_accuracy": ratio(c["pitch_ok"] + c["n_frames"] - c["ref_voiced"] - c["est_voiced"] + c["both_voiced"], c["n_frames"]),
    }


def ref_track(times_s: Any, freqs_hz: Any, n_frames: int) -> np.ndarray:
    """A reference track on the model's frames from an annotation (times_s ascending, freqs_hz; <= 0 Hz unvoiced): per frame
    the annotation sample nearest in time, ties to the earlier sample; MIDI pitches (69 + 12 log2(f / 440), numpy float64), 0.0
    unvoiced.  Without samples every frame is unvoiced.  This project's own resampling rule: unpinned."""
    t = np.asarray(times_s, np.float64).reshape(-1)
    f = np.asarray(freqs_hz, np.float64).reshape(-1)
    if t.shape != f.shape:
        raise ValueError(f"ref_track: {len(t)} times but {len(f)} frequencies")
    if len(t) > 1 and np.any(np.diff(t) < 0):
        raise ValueError("ref_track: times_s must not decrease")
    out = np.zeros(int(n_frames), np.float64)
    if len(t) == 0 or n_frames <= 0:
        return out
    at = frames_to_time_at(np.arange(int(n_frames)))
    right = np.clip(np.searchsorted(t, at, side="left"), 1, len(t) - 1) if len(t) > 1 else np.zeros(len(at), np.int64)
    left = np.maximum(right - 1, 0)
    pick = np.where(np.abs(at - t[left]) <= np.abs(t[right] - at), left, right)
    hz = f[pick]
    voiced = hz > 0
    out[voiced] = 69.0 + 12.0 * np.log2(hz[voiced] / 440.0)
    return out


def _points_call(model: Any, what: str, fixed: tuple, row_offsets: np.ndarray, params: Any):
    """`what(*fixed, p, points, max_points, status)` -> (points of all rows, status per segment)."""
    lib = bind(model._lib)
    p = melody_params(params)
    n, total = len(row_offsets) - 1, int(row_offsets[-1])
    points = np.zeros(max(1, total), MELODY_POINT)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, C.addressof(p), points.ctypes.data, total, status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return points[:total], status[:n]


def melody_from_maps(model: Any, row_offsets: Sequence[int], contour: Any, mem_kind: int, params: Any = None) -> Tuple[np.ndarray, np.ndarray]:
    """One `bp_melody_from_maps` call: `contour` a pointer (or None without rows) to the rows of all segments in host or device
    memory.  Returns (`MELODY_POINT` record per row of all segments, status per segment)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (contour,), mem_kind)
    return _points_call(model, "bp_melody_from_maps", fixed, offs, params)


def infer_clips_melody(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Any = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One `bp_infer_clips_melody` call for [n_frames, channels] arrays at one rate: (records, status, row_offsets)."""
    offs = _clips.clips_row_offsets(model, arrays, sample_rate)
    points, status = _points_call(model, "bp_infer_clips_melody", _jobs.clips_source(model, arrays, sample_rate), offs, params)
    return points, status, offs


def _split(points: np.ndarray, offsets: np.ndarray, status: np.ndarray) -> List[Melody]:
    return [Melody.from_points(points[int(offsets[i]) : int(offsets[i + 1])], int(status[i])) for i in range(len(status))]


def melody(model: Any, outputs: Sequence[Any], params: Any = None) -> List[Melody]:
    """`Model.melody`."""
    if not outputs:
        return []
    offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("contour",), "melody", bare=True)
    points, status = melody_from_maps(model, offs, ptr["contour"], mem_kind, params)
    return _split(points, offs, status)


def transcribe_clips_melody(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None) -> List[Melody]:
    """`Model.transcribe_clips_melody`: the clips of each rate in one `bp_infer_clips_melody` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]

    def run(ids, rate):
        points, status, offs = infer_clips_melody(model, [arrays[i] for i in ids], rate, params)
        return _split(points, offs, status)

    return _jobs.per_rate(_jobs.rates_of(arrays, sample_rates), run)


def _flat_refs(ref_tracks: Sequence[Any], row_offsets: np.ndarray, what: str) -> np.ndarray:
    parts = [np.asarray(r, np.float64).reshape(-1) for r in ref_tracks]
    for i, r in enumerate(parts):
        if len(r) != int(row_offsets[i + 1] - row_offsets[i]):
            raise ValueError(f"{what}: segment {i} has {int(row_offsets[i + 1] - row_offsets[i])} rows but its reference track {len(r)} entries")
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), np.float64)


def _score_call(model: Any, what: str, fixed: tuple, sets: Sequence[Any], pairs: Optional[Sequence[Pair]], n_segments: int,
                ref_pitch: np.ndarray, tolerances: dict) -> np.ndarray:
    """`what(*fixed, n_sets, sets, n_decodes, decodes, ref_pitch, score_params, scores, status)` -> `MELODY_COUNTS` per decode."""
    lib = bind(model._lib)
    prm = _score.score_params(**tolerances)
    arr = sets_array(sets)
    block, n = _jobs.decodes_block(arr, len(sets), pairs, n_segments)
    scores = np.zeros((max(1, n), 6), np.int64)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, *block, ref_pitch.ctypes.data if len(ref_pitch) else None, C.addressof(prm), scores.ctypes.data,
                            status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return _jobs.records(MELODY_COUNTS, scores, status, n)


def melody_sweep_score(model: Any, row_offsets: Sequence[int], contour: Any, mem_kind: int, sets: Sequence[Any], ref_pitch: Any,
                       pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """One `bp_melody_sweep_score` call: `MELODY_COUNTS` per decode; `ref_pitch` one float64 per row of the segments."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (contour,), mem_kind)
    return _score_call(model, "bp_melody_sweep_score", fixed, sets, pairs, len(offs) - 1, np.ascontiguousarray(ref_pitch, np.float64), tolerances)


def infer_clips_melody_sweep_score(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, sets: Sequence[Any], ref_tracks: Sequence[Any],
                                   pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """One `bp_infer_clips_melody_sweep_score` call for [n_frames, channels] arrays at one rate."""
    ref = _flat_refs(ref_tracks, _clips.clips_row_offsets(model, arrays, sample_rate), "infer_clips_melody_sweep_score")
    return _score_call(model, "bp_infer_clips_melody_sweep_score", _jobs.clips_source(model, arrays, sample_rate), sets, pairs,
                       len(arrays), ref, tolerances)


def _result(counts: np.ndarray, shape: Optional[Tuple[int, int]]) -> np.ndarray:
    return counts.reshape(shape) if shape is not None else counts


def sweep_melody_scores(model: Any, outputs: Sequence[Any], sets: Sequence[Any], ref_tracks: Sequence[Any],
                        pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.sweep_melody_scores`."""
    n_seg, n_sets = len(outputs), len(sets)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "sweep_melody_scores", ref_tracks)
    counts = np.zeros(len(todo), MELODY_COUNTS)
    if todo:
        offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("contour",), "sweep_melody_scores", bare=True)
        counts = melody_sweep_score(model, offs, ptr["contour"], mem_kind, sets, _flat_refs(ref_tracks, offs, "sweep_melody_scores"), pairs, **tolerances)
    return _result(counts, (n_sets, n_seg) if pairs is None else None)


def transcribe_clips_sweep_melody_scores(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], sets: Sequence[Any],
                                         ref_tracks: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.transcribe_clips_sweep_melody_scores`: the clips of each rate in one `bp_infer_clips_melody_sweep_score` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    n_seg, n_sets = len(arrays), len(sets)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "transcribe_clips_sweep_melody_scores", ref_tracks)
    counts = np.zeros(len(todo), MELODY_COUNTS)

    def run(ids, rate, local_pairs):
        return infer_clips_melody_sweep_score(model, [arrays[i] for i in ids], rate, sets, [ref_tracks[i] for i in ids],
                                              local_pairs, **tolerances)

    for j, k, _, got in _jobs.per_rate_swept(todo, rates, run):
        counts[j] = got[k]
    return _result(counts, (n_sets, n_seg) if pairs is None else None)
