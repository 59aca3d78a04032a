"""Two recordings against each other (include/basic_pitch_amd_sync.h): which stretch of one segment sounds with which stretch
of another, from the note posteriorgrams alone.

The note rows become a chroma per frame, the chroma sums per unit of `hop` frames, the sums one feature byte a class, two units
a gain, and the best monotone path from the first units of both segments to their last is the synchronisation, all in exact
integers (`sync_rows` is the host checker `bp_sync_rows`; `Model.sync`, `Model.sync_pairs` and `Model.transcribe_clips_sync`
run many pairs on the device, csrc/sync.hip).  The definition is this project's own: unpinned against any third-party
time-warping implementation.  Labels of one take move onto another:

    a, b = model.predict(take_a), model.predict(take_b)
    s = model.sync([a], [b])[0]
    notes_on_b = s.transfer_notes(notes_on_a)              # rows of (start_s, end_s, pitch_midi), ready for Model.align
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

# name -> (restype, argtypes), as include/basic_pitch_amd_sync.h declares them (tests/test_sync_cpu.py compares)
_TAIL = [_i64, _vp, _vp, _vp, _vp, _i64]  # n_pairs, pairs, p, summaries, path, max_path
PROTOTYPES = {
    "bp_sync_params_default": (None, [_vp]),
    "bp_sync_rows": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "bp_sync_from_maps": (_int, [_vp, _i64, _pi64, _vp, _int] + _TAIL),
    "bp_infer_clips_sync": (_int, [_vp, _i64, _vp, _int, _int] + _TAIL),
}

PITCHES = 88                 # BP_SYNC_PITCHES
CLASSES = 12                 # BP_SYNC_CLASSES
MAX_UNITS = 8192             # BP_SYNC_MAX_UNITS
MAX_HOP = 64                 # BP_SYNC_MAX_HOP
MAX_GAIN = 65025             # BP_SYNC_MAX_GAIN
MAX_CELLS = 1 << 28          # BP_SYNC_MAX_CELLS
MAX_PRED_BYTES = 1 << 28     # BP_SYNC_MAX_PRED_BYTES
TRACE_TILE = 64              # BP_SYNC_TRACE_TILE
# bp_sync_summary, 32 bytes
SYNC_SUMMARY = np.dtype([("status", np.int32), ("units_a", np.int32), ("units_b", np.int32), ("n_path", np.int32),
                         ("path_first", np.int64), ("total", np.int64)])
SYNC_PAIR = np.dtype([("a", np.int32), ("b", np.int32)])  # bp_sync_pair, 8 bytes
_PARAM_FIELDS = ("threshold_q", "min_pitch", "max_pitch", "hop", "band", "reserved")
_REFUSED = ("a segment of more than 8192 units, or a malformed bp_sync_params (threshold_q outside 0 ... 1024, pitches outside "
            "0 <= min_pitch <= max_pitch <= 87, hop outside 1 ... 64, band outside 0 ... 8192, a non-zero reserved word)")


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_sync.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def sync_params(params: Any = None, **fields: Any) -> "_native.bp_sync_params":
    """`bp_sync_params`: the defaults (`bp_sync_params_default`: threshold_q 307, pitches 0 ... 87, hop 4, band 0), a given
    record as it is, or a dict / keyword fields on top of the defaults."""
    if isinstance(params, _native.bp_sync_params):
        return params
    lib = bind(_native.load_library())
    p = _native.bp_sync_params()
    lib.bp_sync_params_default(C.addressof(p))
    for k, v in dict(params or {}, **fields).items():
        if k not in _PARAM_FIELDS:
            raise TypeError(f"unknown field {k!r}: bp_sync_params has {list(_PARAM_FIELDS)}")
        if k == "reserved":
            for i, x in enumerate([int(v), 0, 0] if np.isscalar(v) else list(v)):
                p.reserved[i] = int(x)
        else:
            setattr(p, k, int(v))
    return p


def units_of(rows: Any, hop: int) -> np.ndarray:
    """U = ceil(rows / hop), per segment."""
    return (np.asarray(rows, np.int64) + int(hop) - 1) // int(hop)


def _note(note: Any) -> np.ndarray:
    o = np.require(note, np.float32, ["C"])
    if o.ndim != 2 or o.shape[1] != PITCHES:
        raise ValueError(f"note: expected a (T, {PITCHES}) map")
    return o


def pair_table(pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
    """The `bp_sync_pair` array of (a, b) pairs."""
    tab = np.zeros(len(pairs), SYNC_PAIR)
    for j, (a, b) in enumerate(pairs):
        tab[j] = (int(a), int(b))
    return tab


def path_room(rows: Sequence[int], pairs: np.ndarray, hop: int) -> int:
    """The entries of path the pairs own: N + M - 1 a pair, 0 where either segment has no rows (a pair outside the segments
    counts nothing: the call refuses it)."""
    u = units_of(rows, hop)
    ok = [(int(a), int(b)) for a, b in zip(pairs["a"], pairs["b"]) if 0 <= a < len(u) and 0 <= b < len(u)]
    return int(sum(int(u[a] + u[b] - 1) for a, b in ok if u[a] > 0 and u[b] > 0))


def sync_rows(note_a: Any, note_b: Any, params: Any = None, **fields: Any) -> Tuple[np.ndarray, np.ndarray]:
    """The host checker (`bp_sync_rows`) on the (rows, 88) note maps of two segments: (the `SYNC_SUMMARY` record as an array of
    one, the pair's region of path as (N + M - 1, 2) int32, the tail past n_path (-1, -1))."""
    lib = bind(_native.load_library())
    a, b = _note(note_a), _note(note_b)
    p = sync_params(params, **fields)
    room = path_room([len(a), len(b)], pair_table([(0, 1)]), p.hop) if 1 <= p.hop <= MAX_HOP else 0
    path = np.zeros((max(1, room), 2), np.int32)
    summary = np.zeros(1, SYNC_SUMMARY)
    rc = lib.bp_sync_rows(a.ctypes.data if len(a) else None, len(a), b.ctypes.data if len(b) else None, len(b), C.addressof(p),
                          path.ctypes.data, room, summary.ctypes.data)
    if rc != _native.BP_OK:
        raise ValueError("bp_sync_rows: " + _REFUSED)
    return summary, path[:room].copy()


def _frame_time(frames: np.ndarray) -> np.ndarray:
    """Seconds of fractional frames: `frames_to_time_at` of the whole frames around them, joined linearly (float64)."""
    f = np.asarray(frames, np.float64)
    lo = np.floor(f).astype(np.int64)
    t0, t1 = frames_to_time_at(lo), frames_to_time_at(lo + 1)
    return t0 + (f - lo) * (t1 - t0)


@dataclass
class Sync:
    """The synchronisation of one pair (a, b).  `path`: (n_path, 2) int32 unit pairs (i, j) in ascending order, empty unless
    `status` is 0; `total`: D at the end; `units_a`, `units_b`: the units of the two segments; `hop`: frames a unit; status 1:
    a NaN in the note rows of either segment, 2: a segment without rows."""

    status: int
    total: int
    path: np.ndarray
    units_a: int
    units_b: int
    hop: int

    @classmethod
    def of(cls, summary: Any, path: np.ndarray, hop: int) -> "Sync":
        first, n = int(summary["path_first"]), int(summary["n_path"])
        return cls(int(summary["status"]), int(summary["total"]), np.array(path[first : first + n], np.int32).reshape(-1, 2),
                   int(summary["units_a"]), int(summary["units_b"]), int(hop))

    def _curve(self, to: str) -> Tuple[np.ndarray, np.ndarray]:
        """(the centres of the units of the side times are given on, per unit the mean of the centres of the run of the other
        side's units it is matched with), in seconds."""
        if to not in ("a", "b"):
            raise ValueError("to: expected 'a' or 'b'")
        if self.status != 0 or not len(self.path):
            raise ValueError(f"no path: status {self.status}")
        src, dst = (0, 1) if to == "b" else (1, 0)
        n = self.units_a if to == "b" else self.units_b
        centres = _frame_time((self.path[:, dst].astype(np.float64) + 0.5) * self.hop)
        count = np.bincount(self.path[:, src], minlength=n)  # (a path visits every unit of both sides)
        mean = np.bincount(self.path[:, src], weights=centres, minlength=n) / count
        return _frame_time((np.arange(n, dtype=np.float64) + 0.5) * self.hop), mean

    def map_times(self, t: Any, to: str = "b") -> np.ndarray:
        """Times in seconds on a's time base as times on b's (`to="a"`: the other way).  Unit centres are (u + 0.5) hop frames;
        a unit maps to the mean of the centres of the run it is matched with; linear between units, clamped at the ends,
        float64 on the host.  Monotone: the runs of successive units ascend."""
        xs, ys = self._curve(to)
        return np.interp(np.asarray(t, np.float64), xs, ys)

    def transfer_notes(self, notes: Any, to: str = "b") -> np.ndarray:
        """Rows of (start_s, end_s, pitch_midi) moved to the other time base as an (n, 3) float64 array: what `Model.align`
        and the score calls take.  Pitches stay; end >= start stays because the map is monotone."""
        rows = np.asarray(notes, np.float64).reshape(-1, 3)
        return np.stack([self.map_times(rows[:, 0], to), self.map_times(rows[:, 1], to), rows[:, 2]], axis=1)


def _sync_call(model: Any, what: str, fixed: tuple, rows: Sequence[int], pairs: Sequence[Tuple[int, int]], params: Any):
    """`what(*fixed, n_pairs, pairs, p, summaries, path, max_path)` -> (summaries, path of all pairs as (entries, 2))."""
    lib = bind(model._lib)
    p = sync_params(params)
    tab = pairs if isinstance(pairs, np.ndarray) and pairs.dtype == SYNC_PAIR else pair_table(pairs)
    room = path_room(rows, tab, p.hop) if 1 <= p.hop <= MAX_HOP else 0
    summaries = np.zeros(max(1, len(tab)), SYNC_SUMMARY)
    path = np.zeros((max(1, room), 2), np.int32)
    rc = getattr(lib, what)(*fixed, len(tab), tab.ctypes.data if len(tab) else None, C.addressof(p), summaries.ctypes.data,
                            path.ctypes.data, room)
    _native.check(lib, model._handle, rc, what)
    return summaries[: len(tab)], path[:room]


def sync_from_maps(model: Any, row_offsets: Sequence[int], note: Any, mem_kind: int, pairs: Sequence[Tuple[int, int]],
                   params: Any = None):
    """One `bp_sync_from_maps` call: `note` a pointer (or None without rows) to the note rows of all segments in host or
    device memory, `pairs` (a, b) segment indices.  Returns (`SYNC_SUMMARY` records per pair, the path of all pairs)."""
    fixed, offs = _jobs.maps_source(model, row_offsets, (note,), mem_kind)
    return _sync_call(model, "bp_sync_from_maps", fixed, np.diff(offs), pairs, params)


def infer_clips_sync(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, pairs: Sequence[Tuple[int, int]], params: Any = None):
    """One `bp_infer_clips_sync` call for [n_frames, channels] arrays at one rate: (summaries, path)."""
    offs = _clips.clips_row_offsets(model, arrays, sample_rate) if len(arrays) else np.zeros(1, np.int64)
    fixed = _jobs.clips_source(model, arrays, sample_rate)
    return _sync_call(model, "bp_infer_clips_sync", fixed, np.diff(offs), pairs, params)


def _results(summaries: np.ndarray, path: np.ndarray, hop: int) -> List[Sync]:
    return [Sync.of(s, path, hop) for s in summaries]


def sync_pairs(model: Any, outputs: Sequence[Any], pairs: Sequence[Tuple[int, int]], **params: Any) -> List[Sync]:
    """`Model.sync_pairs`."""
    if not len(pairs):
        return []
    p = sync_params(params)
    if any(not (0 <= a < len(outputs) and 0 <= b < len(outputs)) for a, b in pairs):
        raise ValueError(f"sync_pairs: a pair names an output outside 0..{len(outputs) - 1}")
    offs, maps, ptr, mem_kind = _jobs.stack(outputs, ("note",), "sync")
    return _results(*sync_from_maps(model, offs, ptr["note"], mem_kind, pairs, p), p.hop)


def sync(model: Any, outputs_a: Sequence[Any], outputs_b: Sequence[Any], **params: Any) -> List[Sync]:
    """`Model.sync`: the i-th of `outputs_a` against the i-th of `outputs_b`, stacked as 2 n segments with pairs (i, n + i)."""
    n = len(outputs_a)
    if len(outputs_b) != n:
        raise ValueError(f"sync: {n} outputs against {len(outputs_b)}")
    return sync_pairs(model, list(outputs_a) + list(outputs_b), [(i, n + i) for i in range(n)], **params)


def transcribe_clips_sync(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], pairs: Sequence[Tuple[int, int]],
                          **params: Any) -> List[Sync]:
    """`Model.transcribe_clips_sync`: the clips of each rate through the model once (`bp_infer_clips_sync`), with the pairs
    among them."""
    arrays = [_clips.as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    p = sync_params(params)
    for j, (a, b) in enumerate(pairs):
        if not (0 <= a < len(arrays) and 0 <= b < len(arrays)):
            raise ValueError(f"transcribe_clips_sync: pair {j} names a clip outside 0..{len(arrays) - 1}")
        if rates[a] != rates[b]:
            raise ValueError(f"transcribe_clips_sync: pair {j} = ({a}, {b}) joins clips of {rates[a]} Hz and {rates[b]} Hz, which no one "
                             "call takes: use Model.sync on the outputs of predict_pcm")
    results: List[Any] = [None] * len(pairs)
    for rate, ids in _jobs.rate_groups(rates):
        local = {i: k for k, i in enumerate(ids)}
        mine = [j for j, (a, _) in enumerate(pairs) if a in local]
        if not mine:
            continue
        got = infer_clips_sync(model, [arrays[i] for i in ids], rate, [(local[pairs[j][0]], local[pairs[j][1]]) for j in mine], p)
        for j, res in zip(mine, _results(*got, p.hop)):
            results[j] = res
    return results
