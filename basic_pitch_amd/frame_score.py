"""Frame-level precision / recall / accuracy and error rates of decoded events against reference notes
(include/basic_pitch_amd_frame_score.h).

The definition restates `mir_eval.multipitch.evaluate` on the segment's own frames: per frame the refs sounding there are
matched to the distinct pitches of the events sounding there, and the counts are sums over the frames.
`score_note_frames` is the host checker (`bp_score_note_frames`); `Model.sweep_frame_scores` and
`Model.transcribe_clips_sweep_frame_scores` run a sweep of parameter sets and score every decode on the device at the note
and the frame level (csrc/note_score.hip, csrc/note_frames.hip: one workgroup per decode each), so that 60 bytes per decode
come home instead of the events.  Decode by decode the counts are those of the two checkers on the events the sweep calls
return (tests/test_gpu_frame_score.py).  This module binds the prototypes and holds the host side; what it shares with the
note level it takes from `score`.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import events as _events
from . import jobs as _jobs
from . import score as _score
from . import sweep as _sweep

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_frame_score.h declares them (tests/test_frame_score_cpu.py compares)
_TAIL = [_i64, _vp, _i64, _vp, _pi64, _vp, _vp, _vp, _vp, _vp]  # n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status
PROTOTYPES = {
    "bp_score_note_frames": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "bp_note_events_sweep_frame_score": (_int, [_vp, _i64, _pi64, _vp, _vp, _vp, _int] + _TAIL),
    "bp_infer_clips_events_sweep_frame_score": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

_FIELDS = ("n_frames", "ref_frames", "est_frames", "true_pos", "e_sub")
FRAME_COUNTS = np.dtype([(name, np.int64) for name in _FIELDS] + [("status", np.int32)])

Pair = Tuple[int, int]  # (segment, set)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_frame_score.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def score_note_frames(events: Any, refs: Any, n_frames: int, n_events: Optional[int] = None, **tolerances: Any) -> np.ndarray:
    """The host checker (`bp_score_note_frames`): the frame-level counts of `events` (see `score.events_array`; `n_events`:
    the first so many) against `refs` ((start_s, end_s, pitch_midi) rows) over the frames 0 ... n_frames - 1, as one record of
    `FRAME_COUNTS`, status 0.  Of `tolerances` (the fields of `bp_score_params`) the frame level reads `pitch_tolerance_cents`
    and `strict`."""
    lib = bind(_native.load_library())
    est, n = _score.events_array(events)
    n = n if n_events is None else int(n_events)
    _, flat = _score.refs_table([refs])
    p = _score.score_params(**tolerances)
    out = _native.bp_frame_score()
    rc = lib.bp_score_note_frames(C.addressof(est), n, flat.ctypes.data, len(flat), int(n_frames), C.addressof(p), C.addressof(out))
    if rc != _native.BP_OK:
        raise ValueError("bp_score_note_frames: a negative n_frames, a ref with a non-finite field or end_s < start_s, a negative "
                         "or non-finite tolerance, or a non-zero reserved")
    return np.array(tuple(getattr(out, name) for name in _FIELDS) + (0,), FRAME_COUNTS)


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def frame_metrics(counts: np.ndarray) -> Dict[str, np.ndarray]:
    """`FRAME_COUNTS` records -> precision, recall, accuracy and the error rates e_sub, e_miss, e_fa, e_tot of
    mir_eval.multipitch, elementwise; every rate is 0 where its denominator is 0."""
    counts = np.asarray(counts)
    ref, est, tp, sub = (counts[name].astype(np.float64) for name in ("ref_frames", "est_frames", "true_pos", "e_sub"))
    miss, fa = ref - tp - sub, est - tp - sub
    return {"precision": _ratio(tp, est), "recall": _ratio(tp, ref), "accuracy": _ratio(tp, ref + est - tp),
            "e_sub": _ratio(sub, ref), "e_miss": _ratio(miss, ref), "e_fa": _ratio(fa, ref), "e_tot": _ratio(sub + miss + fa, ref)}


def best_set_by_accuracy(counts: np.ndarray) -> int:
    """The set with the highest accuracy over the summed counts of all segments of a (sets, segments) array; ties to the
    lowest index (as `score.best_set`)."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[0] == 0:
        raise ValueError("best_set_by_accuracy: counts must be shaped (sets, segments) with at least one set")
    total = np.zeros(counts.shape[0], FRAME_COUNTS)
    for name in _FIELDS:
        total[name] = counts[name].sum(axis=1)
    return int(np.argmax(frame_metrics(total)["accuracy"]))  # argmax: the first of equals


def _call(model: Any, what: str, fixed: tuple, params: Sequence[Any], pairs: Optional[Sequence[Pair]], n_segments: int,
          refs: Sequence[Any], notes: bool, tolerances: dict) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """`what(*fixed, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, frames, status)` ->
    (`score.COUNTS` per decode, or None without `notes`; `FRAME_COUNTS` per decode), as the device left them."""
    lib = bind(model._lib)
    ref_offs, flat = _score.refs_table(refs)
    prm = _score.score_params(**tolerances)
    sets = _sweep.sets_array(params)
    block, n = _jobs.decodes_block(sets, len(params), pairs, n_segments)
    scores = np.zeros((max(1, n), 4), np.int32)
    frames = np.zeros((max(1, n), 5), np.int64)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, *block, ref_offs.ctypes.data_as(_pi64), flat.ctypes.data if len(flat) else None,
                            C.addressof(prm), scores.ctypes.data if notes else None, frames.ctypes.data, status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return (_jobs.records(_score.COUNTS, scores, status, n) if notes else None), _jobs.records(FRAME_COUNTS, frames, status, n)


def note_events_sweep_frame_score(model: Any, row_offsets: Sequence[int], note: Any, onset: Any, contour: Any, mem_kind: int,
                                  params: Sequence[Any], refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None,
                                  notes: bool = True, **tolerances: Any) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """One `bp_note_events_sweep_frame_score` call (the maps as for `sweep.note_events_sweep`): (`score.COUNTS`,
    `FRAME_COUNTS`) per decode as the device left them — a decode with a non-zero status has {n_ref, 0, 0, 0} and {n_frames, 0,
    0, 0, 0}.  notes False: `scores` is NULL, the note-matching launch is skipped and the first of the pair is None."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (note, onset, contour), mem_kind)
    return _call(model, "bp_note_events_sweep_frame_score", fixed, params, pairs, len(offs) - 1, refs, notes, tolerances)


def infer_clips_events_sweep_frame_score(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Sequence[Any],
                                         refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, notes: bool = True,
                                         **tolerances: Any) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """One `bp_infer_clips_events_sweep_frame_score` call for [n_frames, channels] arrays at one rate; returns as
    `note_events_sweep_frame_score`, a decode's segment being a clip."""
    return _call(model, "bp_infer_clips_events_sweep_frame_score", _jobs.clips_source(model, arrays, sample_rate), params, pairs,
                 len(arrays), refs, notes, tolerances)


def _on_the_host(events: Any, refs: Any, n_frames: int, status: int, notes: bool, tolerances: dict):
    """Both checkers on the events the host decoder gave for a decode the device left; the status stays."""
    frame = score_note_frames(events, refs, n_frames, **tolerances)
    frame["status"] = status
    note = None
    if notes:
        note = _score.score_note_events(events, refs, **tolerances)
        note["status"] = status
    return note, frame


def _result(note: np.ndarray, frame: np.ndarray, notes: bool, shape: Optional[Tuple[int, int]]):
    if shape is not None:
        note, frame = note.reshape(shape), frame.reshape(shape)
    return (note, frame) if notes else frame


def sweep_frame_scores(model: Any, outputs: Sequence[Any], params: Sequence[Any], refs: Sequence[Any],
                       pairs: Optional[Sequence[Pair]] = None, notes: bool = True, **tolerances: Any):
    """`Model.sweep_frame_scores`."""
    n_seg, n_sets = len(outputs), len(params)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "sweep_frame_scores", refs)
    note, frame = np.zeros(len(todo), _score.COUNTS), np.zeros(len(todo), FRAME_COUNTS)
    if todo:
        offs, maps, ptr, mem_kind = _events.stack_maps(outputs, "sweep_frame_scores")
        got, frame = note_events_sweep_frame_score(model, offs, ptr["note"], ptr["onset"], ptr["contour"], mem_kind, params, refs,
                                                   pairs, notes, **tolerances)
        note = got if notes else note
        for j in np.flatnonzero(frame["status"]):  # 1: a NaN or no onset threshold; 2: capacity; 3: too many notes
            s, p = todo[j]
            host = _on_the_host(_score._host_events_from_maps(outputs[s], params[p]), refs[s], int(frame["n_frames"][j]),
                                int(frame["status"][j]), notes, tolerances)
            frame[j] = host[1]
            if notes:
                note[j] = host[0]
    return _result(note, frame, notes, (n_sets, n_seg) if pairs is None else None)


def transcribe_clips_sweep_frame_scores(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]],
                                        params: Sequence[Any], refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None,
                                        notes: bool = True, **tolerances: Any):
    """`Model.transcribe_clips_sweep_frame_scores`: the clips of each rate in one `bp_infer_clips_events_sweep_frame_score` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    n_seg, n_sets = len(arrays), len(params)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "transcribe_clips_sweep_frame_scores", refs)
    note, frame = np.zeros(len(todo), _score.COUNTS), np.zeros(len(todo), FRAME_COUNTS)

    def run(ids, rate, local_pairs):
        return infer_clips_events_sweep_frame_score(model, [arrays[i] for i in ids], rate, params, [refs[i] for i in ids],
                                                    local_pairs, notes, **tolerances)

    for j, k, rate, got in _jobs.per_rate_swept(todo, rates, run):
        n_rec, f_rec = got[0][k] if notes else None, got[1][k]
        if f_rec["status"]:
            s, p = todo[j]
            n_rec, f_rec = _on_the_host(_sweep._host_events(model, arrays[s], rate, params[p]), refs[s], int(f_rec["n_frames"]),
                                        int(f_rec["status"]), notes, tolerances)
        frame[j] = f_rec
        if notes:
            note[j] = n_rec
    return _result(note, frame, notes, (n_sets, n_seg) if pairs is None else None)
