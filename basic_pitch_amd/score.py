"""Note-level precision / recall / F-measure of decoded events against reference notes (include/basic_pitch_amd_score.h).

The definition restates `mir_eval.transcription.match_notes` (onset, pitch and optionally offset within tolerances; the
counts are the sizes of maximum bipartite matchings).  `score_note_events` is the host checker (`bp_score_note_events`);
`Model.sweep_note_scores` and `Model.transcribe_clips_sweep_scores` run a sweep of parameter sets and score every decode on
the device where its events lie (csrc/note_score.hip: one workgroup per decode), so that 20 bytes per decode come home
instead of the events.  Decode by decode the counts are those of the checker on the events the sweep calls return
(tests/test_gpu_score.py).  This module binds the prototypes and holds the host side.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import clips as _clips
from . import events as _events
from . import jobs as _jobs
from . import note_creation as _notes
from . import sweep as _sweep

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes), as include/basic_pitch_amd_score.h declares them (tests/test_score_cpu.py compares)
_TAIL = [_i64, _vp, _i64, _vp, _pi64, _vp, _vp, _vp, _vp]  # n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, status
PROTOTYPES = {
    "bp_score_params_default": (None, [_vp]),
    "bp_score_note_events": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "bp_note_events_sweep_score": (_int, [_vp, _i64, _pi64, _vp, _vp, _vp, _int] + _TAIL),
    "bp_infer_clips_events_sweep_score": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

MAX_NOTES = 16384  # BP_SCORE_MAX_NOTES
STATUS_TOO_MANY_NOTES = 3

COUNTS = np.dtype([("n_ref", np.int32), ("n_est", np.int32), ("matched_onset", np.int32), ("matched_offset", np.int32),
                   ("status", np.int32)])

Pair = Tuple[int, int]  # (segment, set)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_score.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def score_params(**tolerances: Any) -> "_native.bp_score_params":
    """`bp_score_params` with mir_eval's defaults (`bp_score_params_default`) and the given fields on top."""
    p = _native.bp_score_params()
    bind(_native.load_library()).bp_score_params_default(C.addressof(p))
    names = {n for n, _ in _native.bp_score_params._fields_}
    for k, v in tolerances.items():
        if k not in names:
            raise TypeError(f"unknown tolerance {k!r}: bp_score_params has {sorted(names)}")
        setattr(p, k, int(v) if k in ("strict", "reserved") else float(v))
    return p


def refs_table(refs: Sequence[Any]) -> Tuple[np.ndarray, np.ndarray]:
    """Per segment a sequence of (start_s, end_s, pitch_midi) or an (n, 3) array -> (ref_offsets, the `bp_ref_note` records
    of all segments as one (N, 3) float64 array)."""
    parts = [np.asarray(r, np.float64).reshape(-1, 3) for r in refs]
    flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 3)), np.float64)
    return _jobs.offsets_of([len(p) for p in parts]), flat


def events_array(events: Any):
    """`bp_note_event` records (a ctypes array is taken as it is) of note events given as tuples that begin (start_s, end_s,
    pitch_midi, ...) — what `Model.note_events` and `transcribe_clips` return — or an (n, 3) array."""
    if isinstance(events, C.Array) and events._type_ is _native.bp_note_event:
        return events, len(events)
    arr = (_native.bp_note_event * max(1, len(events)))()
    for i, e in enumerate(events):
        arr[i].start_s, arr[i].end_s, arr[i].pitch_midi = float(e[0]), float(e[1]), int(e[2])
    return arr, len(events)


def score_note_events(events: Any, refs: Any, n_events: Optional[int] = None, **tolerances: Any) -> np.ndarray:
    """The host checker (`bp_score_note_events`): the counts of `events` (see `events_array`; `n_events`: the first so many)
    against `refs` ((start_s, end_s, pitch_midi) rows) as one record of `COUNTS`, status 0."""
    lib = bind(_native.load_library())
    est, n = events_array(events)
    n = n if n_events is None else int(n_events)
    _, flat = refs_table([refs])
    p = score_params(**tolerances)
    out = _native.bp_note_score()
    rc = lib.bp_score_note_events(C.addressof(est), n, flat.ctypes.data, len(flat), C.addressof(p), C.addressof(out))
    if rc != _native.BP_OK:
        raise ValueError("bp_score_note_events: a ref with a non-finite field or end_s < start_s, a negative or non-finite "
                         "tolerance, or a non-zero reserved")
    return np.array((out.n_ref, out.n_est, out.matched_onset, out.matched_offset, 0), COUNTS)


def precision_recall_f1(counts: np.ndarray, offsets: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(precision, recall, F) of `COUNTS` records, elementwise: matched / n_est, matched / n_ref and their harmonic mean,
    all 0 where either side is empty (as mir_eval).  offsets False: the onset-and-pitch criterion."""
    counts = np.asarray(counts)
    m = counts["matched_offset" if offsets else "matched_onset"].astype(np.float64)
    n_est, n_ref = counts["n_est"].astype(np.float64), counts["n_ref"].astype(np.float64)
    both = (n_est > 0) & (n_ref > 0)
    precision = np.where(both, m / np.where(both, n_est, 1.0), 0.0)
    recall = np.where(both, m / np.where(both, n_ref, 1.0), 0.0)
    s = precision + recall
    return precision, recall, np.where(s > 0, 2.0 * precision * recall / np.where(s > 0, s, 1.0), 0.0)


def best_set(counts: np.ndarray, offsets: bool = True) -> int:
    """The set with the highest F over the summed counts of all segments of a (sets, segments) array; ties to the lowest index."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[0] == 0:
        raise ValueError("best_set: counts must be shaped (sets, segments) with at least one set")
    total = np.zeros(counts.shape[0], COUNTS)
    for name in ("n_ref", "n_est", "matched_onset", "matched_offset"):
        total[name] = counts[name].sum(axis=1)
    return int(np.argmax(precision_recall_f1(total, offsets)[2]))  # argmax: the first of equals


def _call(model: Any, what: str, fixed: tuple, params: Sequence[Any], pairs: Optional[Sequence[Pair]], n_segments: int,
          ref_offs: np.ndarray, flat: np.ndarray, prm: Any) -> np.ndarray:
    """`what(*fixed, n_sets, sets, n_decodes, decodes, ref_offsets, refs, score_params, scores, status)` -> `COUNTS` per decode."""
    lib = bind(model._lib)
    sets = _sweep.sets_array(params)
    block, n = _jobs.decodes_block(sets, len(params), pairs, n_segments)
    scores = np.zeros((max(1, n), 4), np.int32)
    status = np.zeros(max(1, n), np.int32)
    rc = getattr(lib, what)(*fixed, *block, ref_offs.ctypes.data_as(_pi64), flat.ctypes.data if len(flat) else None,
                            C.addressof(prm), scores.ctypes.data, status.ctypes.data)
    _native.check(lib, model._handle, rc, what)
    return _jobs.records(COUNTS, scores, status, n)


def note_events_sweep_score(model: Any, row_offsets: Sequence[int], note: Any, onset: Any, contour: Any, mem_kind: int,
                            params: Sequence[Any], refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None,
                            **tolerances: Any) -> np.ndarray:
    """One `bp_note_events_sweep_score` call (the maps as for `sweep.note_events_sweep`): `COUNTS` per decode, as the device
    left them — a decode with a non-zero status has {n_ref, 0, 0, 0}."""
    ref_offs, flat = refs_table(refs)
    fixed, offs = _jobs.maps_source(model, row_offsets, (note, onset, contour), mem_kind)
    return _call(model, "bp_note_events_sweep_score", fixed, params, pairs, len(offs) - 1, ref_offs, flat, score_params(**tolerances))


def infer_clips_events_sweep_score(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, params: Sequence[Any],
                                   refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """One `bp_infer_clips_events_sweep_score` call for [n_frames, channels] arrays at one rate; returns as
    `note_events_sweep_score`, a decode's segment being a clip."""
    ref_offs, flat = refs_table(refs)
    return _call(model, "bp_infer_clips_events_sweep_score", _jobs.clips_source(model, arrays, sample_rate), params, pairs,
                 len(arrays), ref_offs, flat, score_params(**tolerances))


def _host_events_from_maps(out: Any, prm: Any) -> List["_notes.NoteEvent"]:
    """A segment's maps under one set by the host decoder (`bp_notes_decode`), on copies."""
    from . import inference as _inf

    return _jobs.host_decode([np.array(out[k].cpu().numpy() if _inf._is_torch_cuda(out[k]) else out[k], np.float32, order="C")
                              for k, _ in _inf._MAPS], prm)


def sweep_note_scores(model: Any, outputs: Sequence[Any], params: Sequence[Any], refs: Sequence[Any],
                      pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.sweep_note_scores`."""
    n_seg, n_sets = len(outputs), len(params)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "sweep_note_scores", refs)
    counts = np.zeros(len(todo), COUNTS)
    if todo:
        offs, maps, ptr, mem_kind = _events.stack_maps(outputs, "sweep_note_scores")
        counts = note_events_sweep_score(model, offs, ptr["note"], ptr["onset"], ptr["contour"], mem_kind, params, refs, pairs,
                                         **tolerances)
        for j in np.flatnonzero(counts["status"]):  # 1: a NaN or no onset threshold; 2: capacity; 3: too many notes
            s, p = todo[j]
            host = score_note_events(_host_events_from_maps(outputs[s], params[p]), refs[s], **tolerances)
            host["status"] = counts["status"][j]
            counts[j] = host
    return counts if pairs is not None else counts.reshape(n_sets, n_seg)


def transcribe_clips_sweep_scores(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Sequence[Any],
                                  refs: Sequence[Any], pairs: Optional[Sequence[Pair]] = None, **tolerances: Any) -> np.ndarray:
    """`Model.transcribe_clips_sweep_scores`: the clips of each rate in one `bp_infer_clips_events_sweep_score` call."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    n_seg, n_sets = len(arrays), len(params)
    todo = _jobs.pairs_checked(pairs, n_seg, n_sets, "transcribe_clips_sweep_scores", refs)
    counts = np.zeros(len(todo), COUNTS)

    def run(ids, rate, local_pairs):
        return infer_clips_events_sweep_score(model, [arrays[i] for i in ids], rate, params, [refs[i] for i in ids], local_pairs,
                                              **tolerances)

    for j, k, rate, got in _jobs.per_rate_swept(todo, rates, run):
        rec = got[k]
        if rec["status"]:
            s, p = todo[j]
            host = score_note_events(_sweep._host_events(model, arrays[s], rate, params[p]), refs[s], **tolerances)
            host["status"] = rec["status"]
            rec = host
        counts[j] = rec
    return counts if pairs is not None else counts.reshape(n_sets, n_seg)
