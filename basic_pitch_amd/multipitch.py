"""Multi-pitch estimates from the contour posteriorgram (include/basic_pitch_amd_multipitch.h).

A multi-pitch estimate is the set of f0 peaks of every contour row: the bins at or above a threshold that exceed both
neighbours (the rule of `scipy.signal.argrelmax`), each refined by a parabola through its three cells to a fractional MIDI
pitch.  `multipitch_rows` is the host checker (`bp_multipitch_rows`), `score_f0_frames` the frame-level counts with the
peaks as the estimate side (`bp_score_f0_frames`); `Model.multipitch` and `Model.transcribe_clips_multipitch` pick, refine
and compact the peaks of many segments on the device (csrc/multipitch.hip), and `Model.sweep_multipitch_frame_scores` /
`Model.transcribe_clips_sweep_multipitch_frame_scores` score a sweep of thresholds and bands there, so that 44 bytes per
decode come home.  Hz are formed here, in numpy: the library produces MIDI pitches alone.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import frame_score as _frames
from . import jobs as _jobs
from . import score as _score
from .note_creation import frames_to_time_at

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_multipitch.h declares them (tests/test_multipitch_cpu.py compares)
_OUT = [_vp, _vp, _i64, _pi64, _vp]  # p, points, max_points, point_offsets, status
_TAIL = [_i64, _vp, _i64, _vp, _pi64, _vp, _vp, _vp, _vp]  # n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status
PROTOTYPES = {
    "bp_mp_params_default": (None, [_vp]),
    "bp_multipitch_rows": (_int, [_vp, _i64, _vp, _vp, _i64, _pi64, _vp]),
    "bp_score_f0_frames": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "bp_multipitch_from_maps": (_int, [_vp, _i64, _pi64, _vp, _int] + _OUT),
    "bp_infer_clips_multipitch": (_int, [_vp, _i64, _vp, _int, _int] + _OUT),
    "bp_multipitch_sweep_frame_score": (_int, [_vp, _i64, _pi64, _vp, _int] + _TAIL),
    "bp_infer_clips_multipitch_sweep_frame_score": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

BINS = 264                # BP_MP_BINS
MAX_PEAKS_PER_ROW = 131   # BP_MP_MAX_PEAKS_PER_ROW
SCAN_TILE_ROWS = 1024     # BP_MP_SCAN_TILE_ROWS
F0_POINT = np.dtype([("frame", np.int32), ("salience", np.float32), ("pitch_midi", np.float64)])  # bp_f0_point, 16 bytes

Pair = Tuple[int, int]  # (segment, set)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_multipitch.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def mp_params(params: Any = None, **fields: Any) -> "_native.bp_mp_params":
    """`bp_mp_params`: the defaults (`bp_mp_params_default`: threshold 0.3, bins 1 ... 262), a given record as it is, or a
    dict / keyword fields on top of the defaults."""
    if isinstance(params, _native.bp_mp_params):
        return params
    p = _native.bp_mp_params()
    bind(_native.load_library()).bp_mp_params_default(C.addressof(p))
    given = dict(params or {}, **fields)
    names = {n for n, _ in _native.bp_mp_params._fields_}
    for k, v in given.items():
        if k not in names:
            raise TypeError(f"unknown field {k!r}: bp_mp_params has {sorted(names)}")
        setattr(p, k, float(v) if k == "threshold" else int(v))
    return p


def sets_array(params: Sequence[Any]):
    arr = (_native.bp_mp_params * max(1, len(params)))()
    for i, p in enumerate(params):
        q = mp_params(p)
        arr[i].threshold, arr[i].min_bin, arr[i].max_bin, arr[i].reserved = q.threshold, q.min_bin, q.max_bin, q.reserved
    return arr


def midi_to_hz(pitch_midi: np.ndarray) -> np.ndarray:
    """440 * 2^((m - 69) / 12), in numpy float64."""
    return 440.0 * np.exp2((np.asarray(pitch_midi, np.float64) - 69.0) / 12.0)


@dataclass
class MultiPitch:
    """The multi-pitch estimate of one segment: one entry per f0 peak, ordered by frame, then by pitch.  `status` 1: a NaN or
    an infinity in the segment's contour rows, and no points."""

    frames: np.ndarray      # int32, the row within the segment
    times_s: np.ndarray     # float64, model_frames_to_time(...)[frames]
    pitch_midi: np.ndarray  # float64, fractional
    salience: np.ndarray    # float32, the contour cell of the peak
    freqs_hz: np.ndarray    # float64, midi_to_hz(pitch_midi)
    status: int = 0

    @classmethod
    def from_points(cls, points: np.ndarray, status: int = 0) -> "MultiPitch":
        frames = np.ascontiguousarray(points["frame"])
        pitch = np.ascontiguousarray(points["pitch_midi"])
        return cls(frames, frames_to_time_at(frames), pitch, np.ascontiguousarray(points["salience"]), midi_to_hz(pitch), int(status))


def multipitch_rows(contour: Any, params: Any = None, max_points: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """The host checker (`bp_multipitch_rows`) on one segment's (rows, 264) contour map: (`F0_POINT` records, status).
    `max_points`: the room to offer (default: asked for first); too little raises ValueError naming the number needed."""
    lib = bind(_native.load_library())
    c = np.require(contour, np.float32, ["C"])
    if c.ndim != 2 or c.shape[1] != BINS:
        raise ValueError(f"contour: expected (T, {BINS})")
    p = mp_params(params)
    n, status = C.c_int64(0), C.c_int(0)
    room = max_points
    if room is None:
        rc = lib.bp_multipitch_rows(c.ctypes.data, len(c), C.addressof(p), None, 0, C.byref(n), C.byref(status))
        if rc != _native.BP_OK and n.value == 0:
            raise ValueError("bp_multipitch_rows: a malformed bp_mp_params (non-finite threshold, min_bin < 1, max_bin > 262, "
                             "min_bin > max_bin or a non-zero reserved)")
        room = n.value
    points = np.zeros(max(1, room), F0_POINT)
    rc = lib.bp_multipitch_rows(c.ctypes.data, len(c), C.addressof(p), points.ctypes.data, int(room), C.byref(n), C.byref(status))
    if rc != _native.BP_OK:
        raise ValueError(f"bp_multipitch_rows: refused ({n.value} points are needed, room for {room}; or a malformed bp_mp_params)")
    return points[: n.value], int(status.value)


def score_f0_frames(points: np.ndarray, refs: Any, n_frames: int, **tolerances: Any) -> np.ndarray:
    """The host checker (`bp_score_f0_frames`): the frame-level counts of `F0_POINT` records against `refs` ((start_s, end_s,
    pitch_midi) rows) over the frames 0 ... n_frames - 1, as one record of `frame_score.FRAME_COUNTS`, status 0."""
    lib = bind(_native.load_library())
    pts = np.ascontiguousarray(points, F0_POINT)
    _, flat = _score.refs_table([refs])
    p = _score.score_params(**tolerances)
    out = _native.bp_frame_score()
    rc = lib.bp_score_f0_frames(pts.ctypes.data if len(pts) else None, len(pts), flat.ctypes.data if len(flat) else None, len(flat),
                                int(n_frames), C.addressof(p), C.addressof(out))
    if rc != _native.BP_OK:
        raise ValueError("bp_score_f0_frames: a negative n_frames, a point with a non-finite pitch, a ref with a non-finite field or "
                         "end_s < start_s, a negative or non-finite tolerance, or a non-zero reserved")
    return np.array(tuple(getattr(out, name) for name in _frames._FIELDS) + (0,), _frames.FRAME_COUNTS)


def _points_call(model: Any, what: str, fixed: tuple, n_segments: int, params: Any, room: Optional[int]):
    """`what(*fixed, p, points, max_points, point_offsets, status)` -> (points, point_offsets, status).  room None: asked for
    with a first call without room (the capacity protocol: the refusal leaves the total in point_offsets[n])."""
    lib = bind(model._lib)
    p = mp_params(params)
    offsets = np.zeros(n_segments + 1, np.int64)
    status = np.zeros(max(1, n_segments), np.int32)
    fn = getattr(lib, what)

    def call(points, max_points):
        return fn(*fixed, C.addressof(p), points, max_points, offsets.ctypes.data_as(_pi64), status.ctypes.data)

    if room is None:
        rc = call(None, 0)
        if rc == _native.BP_OK:  # no points at all
            return np.zeros(0, F0_POINT), offsets, status[:n_segments]
        room = int(offsets[n_segments])
        if rc != _native.BP_ERR_INVALID_ARG or room <= 0:
            _native.check(lib, model._handle, rc, what)
    points = np.zeros(max(1, room), F0_POINT)
    _native.check(lib, model._handle, call(points.ctypes.data, int(room)), what)
    return points[: int(offsets[n_segments])], offsets, status[:n_segments]


def multipitch_from_maps(model: Any, row_offsets: Sequence[int], contour: Any, mem_kind: int, params: Any = None,
                         max_points: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One `bp_multipitch_from_maps` call: `contour` a pointer (or None without rows) to the rows of all segments in host or
    device memory.  Returns (`F0_POINT` records of all segments, point_offsets, status per segment)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (contour,), mem_kind)
    return _points_call(model, "bp_multipitch_from_maps", fixed, len(offs) - 1, params, max_points)


def infer_clips_multipitch(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Any = None,
                           max_points: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One `bp_infer_clips_multipitch` call for [n_frames, channels] arrays at one rate; returns as `multipitch_from_maps`."""
    return _points_call(model, "bp_infer_clips_multipitch", _jobs.clips_source(model, arrays, sample_rate), len(arrays), params,
                        max_points)


def _split(points: np.ndarray, offsets: np.ndarray, status: np.ndarray) -> List[MultiPitch]:
    return [MultiPitch.from_points(points[int(offsets[i]) : int(offsets[i + 1])], int(status[i])) for i in range(len(status))]


def multipitch(model: Any, outputs: Sequence[Any], params: Any = None) -> List[MultiPitch]:
    """`Model.multipitch`."""
    if not outputs:
        return []
    offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("contour",), "multipitch", bare=True)
    return _split(*multipitch_from_maps(model, offs, ptr["contour"], mem_kind, params))


def transcribe_clips_multipitch(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]],
                                params: Any = None) -> List[MultiPitch]:
    """`Model.transcribe_clips_multipitch`: the clips of each rate in one `bp_infer_clips_multipitch` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    return _jobs.per_rate(_jobs.rates_of(arrays, sample_rates),
                          lambda ids, rate: _split(*infer_clips_multipitch(model, [arrays[i] for i in ids], rate, params)))


def _score_call(model: Any, what: str, fixed: tuple, sets: Sequence[Any], pairs: Optional[Sequence[Pair]], n_segments: int,
                refs: Sequence[Any], tolerances: dict) -> np.ndarray:
    """`what(*fixed, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, frames, status)` ->
    `frame_score.FRAME_COUNTS` per decode, as the device left them."""
    lib = bind(model._lib)
    ref_offs, flat = _score.refs_table(refs)
    prm = _score.score_params(**tolerances)
    arr = sets_array(sets)
    block, n = _jobs.decodes_block(arr, len(sets), pairs, n_segments)
    frames = np.zeros((max(1, n), 5), np.int64)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, *block, ref_offs.ctypes.data_as(_pi64), flat.ctypes.data if len(flat) else None,
                            C.addressof(prm), frames.ctypes.data, status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return _jobs.records(_frames.FRAME_COUNTS, frames, status, n)


def multipitch_sweep_frame_score(model: Any, row_offsets: Sequence[int], contour: Any, mem_kind: int, sets: Sequence[Any],
                                 refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """One `bp_multipitch_sweep_frame_score` call: `frame_score.FRAME_COUNTS` per decode as the device left them — a decode
    with a non-zero status has {n_frames, 0, 0, 0, 0}."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (contour,), mem_kind)
    return _score_call(model, "bp_multipitch_sweep_frame_score", fixed, sets, pairs, len(offs) - 1, refs, tolerances)


def infer_clips_multipitch_sweep_frame_score(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, sets: Sequence[Any],
                                             refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None,
                                             **tolerances: Any) -> np.ndarray:
    """One `bp_infer_clips_multipitch_sweep_frame_score` call for [n_frames, channels] arrays at one rate."""
    return _score_call(model, "bp_infer_clips_multipitch_sweep_frame_score", _jobs.clips_source(model, arrays, sample_rate), sets,
                       pairs, len(arrays), refs, tolerances)


def _on_the_host(contour: np.ndarray, params: Any, refs: Any, status: int, tolerances: dict) -> np.ndarray:
    """Both checkers on a decode the device left for too many refs (status 3); the status stays."""
    points, _ = multipitch_rows(contour, params)
    rec = score_f0_frames(points, refs, len(contour), **tolerances)
    rec["status"] = status
    return rec


def _result(frame: np.ndarray, shape: Optional[Tuple[int, int]]) -> np.ndarray:
    return frame.reshape(shape) if shape is not None else frame


def sweep_multipitch_frame_scores(model: Any, outputs: Sequence[Any], sets: Sequence[Any], refs: Sequence[Any],
                                  pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.sweep_multipitch_frame_scores`."""
    n_seg, n_sets = len(outputs), len(sets)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "sweep_multipitch_frame_scores", refs)
    frame = np.zeros(len(todo), _frames.FRAME_COUNTS)
    if todo:
        offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("contour",), "sweep_multipitch_frame_scores", bare=True)
        frame = multipitch_sweep_frame_score(model, offs, ptr["contour"], mem_kind, sets, refs, pairs, **tolerances)
        for j in np.flatnonzero(frame["status"] == 3):  # too many refs for the device: finished here.  1 stays as it is
            s, p = todo[j]
            rows = maps["contour"][int(offs[s]) : int(offs[s + 1])]
            rows = rows if isinstance(rows, np.ndarray) else rows.cpu().numpy()
            frame[j] = _on_the_host(rows, sets[p], refs[s], 3, tolerances)
    return _result(frame, (n_sets, n_seg) if pairs is None else None)


def transcribe_clips_sweep_multipitch_frame_scores(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]],
                                                   sets: Sequence[Any], refs: Sequence[Any],
                                                   pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.transcribe_clips_sweep_multipitch_frame_scores`: the clips of each rate in one
    `bp_infer_clips_multipitch_sweep_frame_score` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    n_seg, n_sets = len(arrays), len(sets)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "transcribe_clips_sweep_multipitch_frame_scores", refs)
    frame = np.zeros(len(todo), _frames.FRAME_COUNTS)

    def run(ids, rate, local_pairs):
        return infer_clips_multipitch_sweep_frame_score(model, [arrays[i] for i in ids], rate, sets, [refs[i] for i in ids],
                                                        local_pairs, **tolerances)

    for j, k, rate, got in _jobs.per_rate_swept(todo, rates, run):
        rec = got[k]
        if rec["status"] == 3:  # the clip's contour rows through the model once more, then both checkers
            s, p = todo[j]
            rows = model.predict_pcm(arrays[s], rate)["contour"]
            rec = _on_the_host(rows, sets[p], refs[s], 3, tolerances)
        frame[j] = rec
    return _result(frame, (n_sets, n_seg) if pairs is None else None)
