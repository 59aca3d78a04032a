"""Streaming sessions: audio that arrives over time -> posteriorgram rows as they become final.

The reference has no such interface (its `predict` takes a finished file); this is the library's `bp_stream_*` family
(include/basic_pitch_amd.h, csrc/stream_api.hip) behind `Model.open_stream`, `Model.push_streams` and
`StreamingTranscriber`.  The rows a stream emits, concatenated, are bit for bit what `Model.predict_pcm_raw` returns for
the concatenated input, for any chunking.

Live use: `Stream.peek()` returns the rows a finish would emit now and commits nothing, so emitted rows + peeked rows are
`predict_pcm_raw` of the audio so far at any moment; `StreamingTranscriber(live=True).transcript()` decodes the notes of the
audio so far from what the device keeps (`bp_stream_keep`, `bp_stream_candidates`; include/basic_pitch_amd_live.h).

Many live sessions: `transcripts(model, transcribers)` is `transcript()` of every one of them behind ONE device step
(`bp_streams_candidates`; include/basic_pitch_amd_update.h), the host half of the decoding on a thread pool.

Many live sessions, decoded on the device: `transcripts(..., decode="device")` takes the events themselves from ONE native
call (`bp_streams_events`; include/basic_pitch_amd_stream_events.h): the sequential half of the decoding runs on the device,
a workgroup per session, and only events and bends come home.

Endless use: `StreamingTranscriber(live=True, horizon_seconds=H)` keeps the last H seconds in a ring on the device
(`bp_stream_keep_rolling`, `bp_stream_candidates_rolling`; include/basic_pitch_amd_rolling.h) and `transcript()` is the exact
decode of those rows in absolute stream time: device memory, host memory and the work of an update do not grow with the session.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import inference as _inf
from . import note_creation as _notes

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)
# name -> (restype, argtypes), as include/basic_pitch_amd.h declares them (tests/test_stream_geometry_cpu.py compares)
PROTOTYPES = {
    "bp_stream_open": (_int, [_vp, _int, _int, _int, C.POINTER(_vp)]),
    "bp_stream_push": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _i64, _int, _pi64]),
    "bp_stream_finish": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _pi64]),
    "bp_streams_push": (_int, [_vp, _i64, C.POINTER(_vp), C.POINTER(_vp), _pi64, _int, C.POINTER(_vp), C.POINTER(_vp),
                               C.POINTER(_vp), _pi64, _int, _pi64]),
    "bp_stream_close": (None, [_vp]),
    "bp_stream_rows_bound": (_i64, [_vp, _i64]),
    "bp_stream_state_bytes": (_i64, [_vp]),
    "bp_stream_rows_after": (_i64, [_i64, _int]),
}
# the same for include/basic_pitch_amd_live.h (tests/test_stream_peek_cpu.py compares)
LIVE_PROTOTYPES = {
    "bp_stream_peek": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _pi64]),
    "bp_streams_peek": (_int, [_vp, _i64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _pi64, _int, _pi64]),
    "bp_stream_keep": (_int, [_vp, _vp, _i64]),
    "bp_stream_candidates": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _i64, _pi64, _vp]),
}
# the same for include/basic_pitch_amd_rolling.h (tests/test_stream_rolling_cpu.py compares)
ROLLING_PROTOTYPES = {
    "bp_stream_keep_rolling": (_int, [_vp, _vp, _i64]),
    "bp_stream_horizon_first_row": (_i64, [_i64, _i64]),
    "bp_stream_candidates_rolling": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _i64, _pi64, _pi64, _vp]),
    "bp_stream_rolling_maps": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _pi64, _pi64]),
    "bp_notes_decode_candidates_at": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _pi64, _pi64]),
}
# the same for include/basic_pitch_amd_update.h (tests/test_streams_update_cpu.py compares)
UPDATE_PROTOTYPES = {
    "bp_streams_update_layout": (_int, [_vp, _i64, _vp, _int, _pi64, _pi64]),
    "bp_streams_candidates": (_int, [_vp, _i64, _vp, _int, _vp, _vp, _vp, _i64, _i64]),
}
# the same for include/basic_pitch_amd_stream_events.h (tests/test_stream_events_cpu.py compares)
STREAM_EVENTS_PROTOTYPES = {
    "bp_streams_events_layout": (_int, [_vp, _i64, _vp, _int, _pi64, _pi64]),
    "bp_streams_events": (_int, [_vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _pi64]),
}
TAIL_ROWS = 2 * 142  # the rows a peek can have: what a rolling stream's ring holds beyond its horizon

# the numpy type a chunk of each format is made of (packed 24-bit and G.711: bytes)
_DTYPES = {_native.BP_PCM_F32: np.float32, _native.BP_PCM_S16: np.int16, _native.BP_PCM_S24: np.uint8,
           _native.BP_PCM_S32: np.int32, _native.BP_PCM_U8: np.uint8, _native.BP_PCM_F64: np.float64,
           _native.BP_PCM_S16_BE: np.dtype(">i2"), _native.BP_PCM_S24_BE: np.uint8, _native.BP_PCM_S32_BE: np.dtype(">i4"),
           _native.BP_PCM_F32_BE: np.dtype(">f4"), _native.BP_PCM_F64_BE: np.dtype(">f8"), _native.BP_PCM_S8: np.int8,
           _native.BP_PCM_ULAW: np.uint8, _native.BP_PCM_ALAW: np.uint8}


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the streaming family's prototypes (the five headers) on a loaded library."""
    return _native.bind(lib, {**PROTOTYPES, **LIVE_PROTOTYPES, **ROLLING_PROTOTYPES, **UPDATE_PROTOTYPES, **STREAM_EVENTS_PROTOTYPES})


def horizon_first_row(n_rows: int, horizon_rows: int) -> int:
    """The first row of a rolling transcript of `n_rows` rows, max(0, n_rows - horizon_rows) (`bp_stream_horizon_first_row`; no GPU)."""
    return int(bind(_native.load_library()).bp_stream_horizon_first_row(int(n_rows), int(horizon_rows)))


def rows_after(n_samples: int, finished: bool = False) -> int:
    """Rows a stream has emitted once its 22.05 kHz signal has `n_samples` samples (`bp_stream_rows_after`; no GPU)."""
    return int(bind(_native.load_library()).bp_stream_rows_after(int(n_samples), int(bool(finished))))


class Stream:
    """One streaming session of a `Model` (`Model.open_stream`).  `push(chunk)` returns the rows that became final,
    `finish()` the rest; afterwards only `close()` is valid.  A context manager: leaving it closes the stream."""

    def __init__(self, model: "_inf.Model", sample_rate: int, channels: int = 1, fmt: int = _native.BP_PCM_F32):
        self._model = model
        self._lib = bind(model._lib)
        self.sample_rate, self.channels, self.fmt = int(sample_rate), int(channels), int(fmt)
        self._s = C.c_void_p()
        rc = self._lib.bp_stream_open(model._handle, self.fmt, self.channels, self.sample_rate, C.byref(self._s))
        _native.check(self._lib, model._handle, rc, "bp_stream_open")
        self._frame_bytes = self.channels * _native.BP_PCM_WIDTH[self.fmt]
        self.rows = 0  # rows emitted so far

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_s", None) is not None and self._s.value:
            if self._model._handle.value:  # a stream does not outlive its handle
                self._lib.bp_stream_close(self._s)
            self._s = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "Stream":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    # -- the calls --------------------------------------------------------------------------------
    def _chunk(self, chunk: Any) -> Tuple[np.ndarray, int]:
        """`chunk` as the contiguous bytes the library reads and its frame count.  Arrays of the format's own type (or, for
        float32 streams, anything numeric) shaped [n_frames] / [n_frames, channels]; bytes-like objects as they are."""
        if isinstance(chunk, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(chunk, dtype=np.uint8)
        else:
            a = np.asarray(chunk)
            want = _DTYPES[self.fmt]
            if a.dtype != want:
                if self.fmt != _native.BP_PCM_F32:
                    raise ValueError(f"a chunk of this stream is {np.dtype(want).name} (or bytes), got {a.dtype}")
                a = a.astype(np.float32)
            buf = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if buf.size % self._frame_bytes:
            raise ValueError(f"a chunk must hold whole frames of {self._frame_bytes} bytes, got {buf.size} bytes")
        return buf, buf.size // self._frame_bytes

    def rows_bound(self, n_frames: int) -> int:
        return int(self._lib.bp_stream_rows_bound(self._s, int(n_frames)))

    def state_bytes(self) -> int:
        return int(self._lib.bp_stream_state_bytes(self._s))

    def _taken(self, out: Dict[str, np.ndarray], rows: int) -> Dict[str, np.ndarray]:
        self.rows += rows
        return {k: v[:rows] for k, v in out.items()}

    def push(self, chunk: Any) -> Dict[str, np.ndarray]:
        """Append a chunk; {"note","onset","contour"} of the rows that became final — (0, 88) / (0, 264) is a normal answer."""
        buf, n = self._chunk(chunk)
        out = _inf._empty_maps((self.rows_bound(n),))
        rows = C.c_int64(0)
        rc = self._lib.bp_stream_push(self._s, buf.ctypes.data if n else None, n, _native.BP_MEM_HOST,
                                      *[_inf._ptr(out[k]) for k, _ in _inf._MAPS], out["note"].shape[0], _native.BP_MEM_HOST,
                                      C.byref(rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_push")
        return self._taken(out, int(rows.value))

    def finish(self) -> Dict[str, np.ndarray]:
        """The end of the signal: the remaining rows, up to the row count of the one-shot call."""
        out = _inf._empty_maps((self.rows_bound(0),))
        rows = C.c_int64(0)
        rc = self._lib.bp_stream_finish(self._s, *[_inf._ptr(out[k]) for k, _ in _inf._MAPS], out["note"].shape[0],
                                        _native.BP_MEM_HOST, C.byref(rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_finish")
        return self._taken(out, int(rows.value))

    def peek(self) -> Dict[str, np.ndarray]:
        """The rows `finish()` would return now, with nothing committed (`bp_stream_peek`): the rows emitted so far followed
        by these are bit for bit `predict_pcm_raw` of the audio so far, and later pushes are unaffected."""
        out = _inf._empty_maps((self.rows_bound(0),))
        rows = C.c_int64(0)
        rc = self._lib.bp_stream_peek(self._s, *[_inf._ptr(out[k]) for k, _ in _inf._MAPS], out["note"].shape[0],
                                      _native.BP_MEM_HOST, C.byref(rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_peek")
        return {k: v[: int(rows.value)] for k, v in out.items()}

    def keep(self, prm: Any, max_rows: int) -> None:
        """Keep the maps of every emitted row on the device for `candidates` (`bp_stream_keep`; before the first row leaves).
        `prm`: `note_creation._note_params`, fixed from here on; `max_rows`: the rows reserved, 1,760 bytes each."""
        rc = self._lib.bp_stream_keep(self._s, C.addressof(prm), int(max_rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_keep")

    def candidates(self, note: np.ndarray, bits: np.ndarray, bend: Optional[np.ndarray], first_row: int,
                   with_tail: bool = True) -> Tuple[int, int]:
        """`bp_stream_candidates` into the caller's host arrays (note (cap, 88) float32, bits (cap, 12) uint8, bend (cap, 88)
        int8 or None): rows from `first_row` on of note / bend, all rows of bits.  Returns (T, status)."""
        n_rows, status = C.c_int64(0), C.c_int(0)
        rc = self._lib.bp_stream_candidates(self._s, int(bool(with_tail)), note.ctypes.data, bits.ctypes.data,
                                            bend.ctypes.data if bend is not None else None, int(first_row), note.shape[0],
                                            C.byref(n_rows), C.addressof(status))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_candidates")
        return int(n_rows.value), int(status.value)

    def keep_rolling(self, prm: Any, horizon_rows: int) -> None:
        """Keep the last `horizon_rows` rows of the maps in a ring on the device for `candidates_rolling`
        (`bp_stream_keep_rolling`; before the first row leaves, instead of `keep`): horizon_rows + 284 rows of 1,760 bytes
        and a small table of records, whatever the age of the stream."""
        rc = self._lib.bp_stream_keep_rolling(self._s, C.addressof(prm), int(horizon_rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_keep_rolling")
        self.horizon_rows = int(horizon_rows)

    def candidates_rolling(self, note: np.ndarray, bits: np.ndarray, bend: Optional[np.ndarray], held_rows: int,
                           with_tail: bool = True) -> Tuple[int, int, int]:
        """`bp_stream_candidates_rolling` into the caller's host RINGS (note (R, 88) float32, bits (R, 12) uint8, bend (R, 88)
        int8 or None; R >= horizon_rows + 284; absolute row r at index r % R): the note / bend rows from max(held_rows, a) on,
        the bits of all rows of [a, T).  Returns (a, T, status)."""
        first, n_rows, status = C.c_int64(0), C.c_int64(0), C.c_int(0)
        rc = self._lib.bp_stream_candidates_rolling(self._s, int(bool(with_tail)), note.ctypes.data, bits.ctypes.data,
                                                    bend.ctypes.data if bend is not None else None, note.shape[0], int(held_rows),
                                                    C.byref(first), C.byref(n_rows), C.addressof(status))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_candidates_rolling")
        return int(first.value), int(n_rows.value), int(status.value)

    def rolling_maps(self, with_tail: bool = True) -> Tuple[int, Dict[str, np.ndarray]]:
        """`bp_stream_rolling_maps`: (a, the kept, frequency-constrained maps of rows [a, T), linear)."""
        out = _inf._empty_maps((min(self.horizon_rows, self.rows + self.rows_bound(0)),))
        first, n_rows = C.c_int64(0), C.c_int64(0)
        rc = self._lib.bp_stream_rolling_maps(self._s, int(bool(with_tail)), *[_inf._ptr(out[k]) for k, _ in _inf._MAPS],
                                              out["note"].shape[0], C.byref(first), C.byref(n_rows))
        _native.check(self._lib, self._model._handle, rc, "bp_stream_rolling_maps")
        a, T = int(first.value), int(n_rows.value)
        return a, {k: v[: T - a] for k, v in out.items()}


def _unwrapped(ring: np.ndarray, a: int, T: int) -> np.ndarray:
    """Rows [a, T) of a host ring (row r at index r % len(ring)), linear: a view, or one copy where they wrap."""
    lo, n = a % ring.shape[0], T - a
    if lo + n <= ring.shape[0]:
        return ring[lo : lo + n]
    return np.concatenate((ring[lo:], ring[: lo + n - ring.shape[0]]))


def _step_arrays(n: int):
    return lambda vals: (C.c_void_p * n)(*vals)


def peek_streams(model: "_inf.Model", streams: Sequence[Stream]) -> List[Dict[str, np.ndarray]]:
    """`Stream.peek` for several streams of `model` in one step (`bp_streams_peek`): their tail windows run in full batches."""
    n = len(streams)
    if n == 0:
        return []
    lib = bind(model._lib)
    outs = [_inf._empty_maps((s.rows_bound(0),)) for s in streams]
    arr = _step_arrays(n)
    rows = (C.c_int64 * n)()
    rc = lib.bp_streams_peek(model._handle, n, arr([s._s.value for s in streams]),
                             *[arr([_inf._ptr(o[k]) for o in outs]) for k, _ in _inf._MAPS],
                             (C.c_int64 * n)(*[o["note"].shape[0] for o in outs]), _native.BP_MEM_HOST, rows)
    _native.check(lib, model._handle, rc, "bp_streams_peek")
    return [{k: v[: int(r)] for k, v in o.items()} for o, r in zip(outs, rows)]


def push_streams(model: "_inf.Model", streams: Sequence[Stream], chunks: Sequence[Any]) -> List[Dict[str, np.ndarray]]:
    """One step for several streams of `model` (`bp_streams_push`): each stream's chunk is ingested, the newly complete
    windows of all of them run in full batches.  Returns each stream's new rows, exactly what `Stream.push` would return."""
    n = len(streams)
    if n != len(chunks):
        raise ValueError("one chunk per stream")
    if n == 0:
        return []
    lib = bind(model._lib)
    parts = [s._chunk(c) for s, c in zip(streams, chunks)]
    outs = [_inf._empty_maps((s.rows_bound(k),)) for s, (_, k) in zip(streams, parts)]
    arr = _step_arrays(n)
    rows = (C.c_int64 * n)()
    rc = lib.bp_streams_push(
        model._handle, n, arr([s._s.value for s in streams]), arr([b.ctypes.data if k else None for b, k in parts]),
        (C.c_int64 * n)(*[k for _, k in parts]), _native.BP_MEM_HOST,
        *[arr([_inf._ptr(o[k]) for o in outs]) for k, _ in _inf._MAPS],
        (C.c_int64 * n)(*[o["note"].shape[0] for o in outs]), _native.BP_MEM_HOST, rows,
    )
    _native.check(lib, model._handle, rc, "bp_streams_push")
    return [s._taken(o, int(r)) for s, o, r in zip(streams, outs, rows)]


def update_table(streams: Sequence[Stream], held_rows: Sequence[int]):
    """The `bp_stream_update` array of `bp_streams_update_layout` / `bp_streams_candidates` for these streams."""
    tab = (_native.bp_stream_update * max(1, len(streams)))()
    for i, (s, held) in enumerate(zip(streams, held_rows)):
        tab[i].stream, tab[i].held_rows = s._s.value, int(held)
    return tab


def streams_candidates(model: "_inf.Model", streams: Sequence[Stream], held_rows: Sequence[int], with_tail: bool = True,
                       bends: bool = True):
    """One `bp_streams_candidates` call: (the `bp_stream_update` array, note (rows, 88) float32, bend (rows, 88) int8 or None,
    bits (rows, 12) uint8), packed: stream i's note / bend rows [new_row, n_rows) at `note_offset`, its bitmap rows
    [first_row, n_rows) at `bits_offset`."""
    lib = bind(model._lib)
    n = len(streams)
    tab = update_table(streams, held_rows)
    note_rows, bits_rows = C.c_int64(0), C.c_int64(0)
    rc = lib.bp_streams_update_layout(model._handle, n, C.addressof(tab), int(bool(with_tail)), C.byref(note_rows), C.byref(bits_rows))
    _native.check(lib, model._handle, rc, "bp_streams_update_layout")
    note = np.empty((note_rows.value, 88), np.float32)
    bend = np.empty((note_rows.value, 88), np.int8) if bends else None
    bits = np.empty((bits_rows.value, 12), np.uint8)
    rc = lib.bp_streams_candidates(model._handle, n, C.addressof(tab), int(bool(with_tail)), note.ctypes.data,
                                   bend.ctypes.data if bends else None, bits.ctypes.data, note.shape[0], bits.shape[0])
    _native.check(lib, model._handle, rc, "bp_streams_candidates")
    return tab, note, bend, bits


def events_table(streams: Sequence[Stream]):
    """The `bp_stream_events` array of `bp_streams_events_layout` / `bp_streams_events` for these streams."""
    tab = (_native.bp_stream_events * max(1, len(streams)))()
    for i, s in enumerate(streams):
        tab[i].stream = s._s.value
    return tab


def slice_first_row(rows_out: int, tail_rows: int, horizon_rows: Optional[int]) -> Tuple[int, int]:
    """The pure-Python mirror of the layout's arithmetic: (first_row, n_rows) of a stream that has emitted `rows_out` rows and
    whose peek would add `tail_rows`; `horizon_rows` None for a stream that keeps all its rows."""
    T = int(rows_out) + int(tail_rows)
    return (0 if horizon_rows is None else max(0, T - int(horizon_rows))), T


def streams_events_capacity(slices: Sequence[Tuple[int, int, bool]]) -> Tuple[int, int]:
    """The pure-Python mirror of `bp_streams_events_layout`'s totals for (slice rows, min_note_len, pitch bends) per stream:
    the events and the bends with which `bp_streams_events` cannot fail for room."""
    from . import events as _events

    return (sum(_events.events_capacity(r, m) for r, m, _ in slices),
            sum(_events.bends_capacity(r) for r, _, b in slices if b))


def streams_events_layout(model: "_inf.Model", streams: Sequence[Stream], with_tail: bool = True):
    """`bp_streams_events_layout`: (the `bp_stream_events` array with first_row / n_rows, events capacity, bends capacity)."""
    lib = bind(model._lib)
    tab = events_table(streams)
    cap_e, cap_b = C.c_int64(0), C.c_int64(0)
    rc = lib.bp_streams_events_layout(model._handle, len(streams), C.addressof(tab), int(bool(with_tail)), C.byref(cap_e), C.byref(cap_b))
    _native.check(lib, model._handle, rc, "bp_streams_events_layout")
    return tab, int(cap_e.value), int(cap_b.value)


def streams_events(model: "_inf.Model", streams: Sequence[Stream], with_tail: bool = True, room: Optional[Tuple[int, int]] = None):
    """One `bp_streams_events` call: (the `bp_stream_events` array, events, bends, event_offsets), stream i's events at
    event_offsets[i]:event_offsets[i + 1] where its status is 0.  `room`: (max_events, max_bends) to call with, once; without it
    the call is repeated with the sizes it asks for when the first guess was too small."""
    from . import events as _events

    lib = bind(model._lib)
    n = len(streams)
    tab = events_table(streams)
    fixed = (model._handle, n, C.addressof(tab), int(bool(with_tail)))
    rows = sum(min(s.rows + TAIL_ROWS, getattr(s, "horizon_rows", None) or s.rows + TAIL_ROWS) for s in streams)  # a first guess
    call = lambda *a: lib.bp_streams_events(*a[:-1])  # noqa: E731  (status lives in the array)
    events, bends, offsets, _ = _events._call(lib, model._handle, "bp_streams_events", call, fixed, n, rows, room)
    return tab, events, bends, offsets


def scatter_rows(ring: np.ndarray, packed: np.ndarray, r0: int, r1: int) -> None:
    """Packed rows (row 0 is absolute row r0) into a host ring, absolute row r at index r % len(ring): one slice assignment,
    two where the rows wrap.  An array that never wraps is a ring longer than r1."""
    R, at = ring.shape[0], 0
    while r0 + at < r1:
        lo = (r0 + at) % R
        k = min(r1 - r0 - at, R - lo)
        ring[lo : lo + k] = packed[at : at + k]
        at += k


def _transcripts_device(model: "_inf.Model", ts: List["StreamingTranscriber"], workers: Optional[int], midi: bool) -> List[Any]:
    """`transcripts(decode="device")`: the events of every session from one `bp_streams_events` call; a session with status 1 or
    2 takes the host route.  No transcriber's host arrays or `_held` are touched for a session the device decodes."""
    from . import events as _events

    results: List[Any] = [None] * len(ts)
    ids = [i for i, t in enumerate(ts) if t._prm.onset_threshold > 0]  # the others: status 1 whatever the maps hold
    if ids:
        tab, events, bends, offsets = streams_events(model, [ts[i].stream for i in ids])
        for k, i in enumerate(ids):
            if tab[k].status == 0:
                ev = _events.clip_events(events, bends, offsets, k, True)
                results[i] = (_notes.note_events_to_midi(ev, ts[i]._decoding[5], ts[i]._decoding[7]) if midi else None, ev)
    rest = [i for i, r in enumerate(results) if r is None]
    for i, r in zip(rest, transcripts(model, [ts[i] for i in rest], workers, "host", midi)):
        results[i] = r
    return results


def transcripts(model: "_inf.Model", transcribers: Sequence["StreamingTranscriber"], workers: Optional[int] = None,
                decode: str = "host", midi: bool = True) -> List[Any]:
    """`t.transcript()` for every live transcriber of `model`, of either mode, in order — behind one native call
    (`bp_streams_candidates`): the tails' windows of all sessions run in shared batches, each session's packed rows are
    scattered into its own host arrays, and the sequential half of the decoding runs per session on a pool of `workers`
    threads (default 8; the native decoder releases the GIL).  A transcriber whose onset threshold is <= 0 or whose slice holds
    a NaN takes the fallback `transcript()` takes.

    `decode="device"`: the same list from one `bp_streams_events` call — the sequential half runs on the device, a workgroup
    per session, and only the events and bends come home; sessions the device leaves out (a NaN, a slice of more than 8,192
    rows) take the route above.  `midi=False` returns `(None, note_events)` and skips `note_events_to_midi`, which holds the
    interpreter lock."""
    from concurrent.futures import ThreadPoolExecutor

    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    ts = list(transcribers)
    for t in ts:
        if not t.live:
            raise ValueError("transcripts() needs StreamingTranscriber(live=True)")
    if not ts:
        return []
    if decode == "device":
        return _transcripts_device(model, ts, workers, bool(midi))
    results: List[Any] = [None] * len(ts)
    ids = [i for i, t in enumerate(ts) if t._prm.onset_threshold > 0]  # the others: status 1 whatever the maps hold
    if ids:
        tab, note, bend, bits = streams_candidates(model, [ts[i].stream for i in ids], [ts[i]._held for i in ids])
    with ThreadPoolExecutor(max_workers=max(1, int(workers or 8))) as pool:
        pending = []
        for k, i in enumerate(ids):
            t, u = ts[i], tab[k]
            a, T, n0 = int(u.first_row), int(u.n_rows), int(u.new_row)
            if t.horizon_rows is None:
                t._room(T)
            scatter_rows(t._note, note[u.note_offset : u.note_offset + T - n0], n0, T)
            scatter_rows(t._bend, bend[u.note_offset : u.note_offset + T - n0], n0, T)
            scatter_rows(t._bits, bits[u.bits_offset : u.bits_offset + T - a], a, T)
            t._held = t.stream.rows  # rows at or after it were a tail's: sent again next time
            if u.status == 0:
                pending.append((i, pool.submit(t._decoded, a, T, midi)))
        decoding = {i for i, _ in pending}
        for i, t in enumerate(ts):  # the fallbacks use the handle: on this thread, after the native call
            if i not in decoding:
                results[i] = t._host_decoded() if midi else (None, t._host_decoded()[1])
        for i, fut in pending:
            results[i] = fut.result()
    return results


class StreamingTranscriber:
    """`predict()` for audio that arrives in chunks: `push(chunk)` feeds a stream and keeps the emitted rows on the host,
    `finish()` returns `(model_output, midi_data, note_events)` exactly as `predict()` does for the same audio.

    With `live=True`, `transcript()` returns `(midi_data, note_events)` for the audio pushed so far — exactly what `predict()`
    returns for that prefix — at any moment between pushes.  The stream then keeps its maps on the device
    (`bp_stream_keep`; `max_rows` rows of 1,760 bytes are reserved in device memory when the transcriber is made — the
    default, 52,200 rows, is ten minutes of audio and 92 MB; an hour is 313,200 rows and 551 MB — and a push past them
    raises), an update sends only the note and
    bend rows that are new since the last one plus the 12-byte-per-row peak bitmap, and the sequential half of the decoder
    runs on the host (`bp_notes_decode_candidates`).  Events are NOT final until `finish()`: `get_infered_onsets` scales the
    note-map differences by two maxima taken over the whole track and the melodia pass walks the whole posteriorgram, so an
    event of an earlier transcript can move or vanish when later audio arrives.  What is exact at every update is the answer
    to "what if the audio ended now".

    With `horizon_seconds` as well (it needs `live=True`; `max_rows` is then ignored), the session can stay open for ever:
    the stream keeps the last ceil(horizon_seconds * 22050 / 256) rows in a ring on the device (`bp_stream_keep_rolling`),
    `transcript()` returns `(midi_data, note_events)` of exactly those rows decoded as a whole track, in absolute stream time
    (`horizon_first_time`: where they start), `push()` hands out the rows and retains none, the host arrays are rings of a
    fixed size, and `finish()` returns `(the rows finish emitted, midi_data, note_events)` for the final slice.  While the
    session is shorter than the horizon the transcripts are those of the mode without it."""

    def __init__(
        self,
        model_or_model_path: Any = _inf.ICASSP_2022_MODEL_PATH,
        sample_rate: int = _inf.AUDIO_SAMPLE_RATE,
        channels: int = 1,
        fmt: int = _native.BP_PCM_F32,
        onset_threshold: float = _inf.DEFAULT_ONSET_THRESHOLD,
        frame_threshold: float = _inf.DEFAULT_FRAME_THRESHOLD,
        minimum_note_length: float = _inf.DEFAULT_MINIMUM_NOTE_LENGTH_MS,
        minimum_frequency: Optional[float] = None,
        maximum_frequency: Optional[float] = None,
        multiple_pitch_bends: bool = False,
        melodia_trick: bool = True,
        midi_tempo: float = _inf.DEFAULT_MINIMUM_MIDI_TEMPO,
        live: bool = False,
        max_rows: int = 600 * 87,
        horizon_seconds: Optional[float] = None,
    ):
        if horizon_seconds is not None and not live:
            raise ValueError("horizon_seconds needs StreamingTranscriber(live=True)")
        self._decoding = (onset_threshold, frame_threshold, minimum_note_length, minimum_frequency, maximum_frequency,
                          multiple_pitch_bends, melodia_trick, midi_tempo)
        self.stream = Stream(_inf._model_from(model_or_model_path), sample_rate, channels, fmt)
        self._rows: List[Dict[str, np.ndarray]] = []
        self.live = bool(live)
        self.horizon_rows = None if horizon_seconds is None else int(np.ceil(horizon_seconds * _inf.AUDIO_SAMPLE_RATE / _inf.FFT_HOP))
        if self.horizon_rows is not None:
            self._prm = _notes._note_params(onset_threshold, frame_threshold, _inf._min_note_len_frames(minimum_note_length), True,
                                            maximum_frequency, minimum_frequency, melodia_trick, _notes.ENERGY_TOLERANCE, True)
            self.stream.keep_rolling(self._prm, self.horizon_rows)
            self._held = 0  # final rows of the note and bend rings already on the host
            ring = self.horizon_rows + TAIL_ROWS
            self._note = np.empty((ring, _inf.N_FREQ_BINS_NOTES), np.float32)
            self._bend = np.empty((ring, _inf.N_FREQ_BINS_NOTES), np.int8)
            self._bits = np.empty((ring, 12), np.uint8)
        elif self.live:
            # the parameters model_output_to_notes decodes with (note_creation.py:52-116 defaults: inferred onsets, pitch bends)
            self._prm = _notes._note_params(onset_threshold, frame_threshold, _inf._min_note_len_frames(minimum_note_length), True,
                                            maximum_frequency, minimum_frequency, melodia_trick, _notes.ENERGY_TOLERANCE, True)
            self.stream.keep(self._prm, max_rows)
            self._held = 0  # final rows of the note and bend maps already on the host
            self._note = np.empty((0, _inf.N_FREQ_BINS_NOTES), np.float32)
            self._bend = np.empty((0, _inf.N_FREQ_BINS_NOTES), np.int8)
            self._bits = np.empty((0, 12), np.uint8)

    def push(self, chunk: Any) -> Dict[str, np.ndarray]:
        out = self.stream.push(chunk)
        if self.horizon_rows is None:
            self._rows.append(out)
        return out

    @property
    def horizon_first_time(self) -> float:
        """The absolute time of the first row of the rolling transcript the stream would give now."""
        s = self.stream
        tail = 0 if not s._s.value else s.rows_bound(0)
        return float(_notes.frames_to_time_at(np.array([horizon_first_row(s.rows + tail, self.horizon_rows)]))[0])

    def _decoded(self, a: int, T: int, midi: bool = True):
        """Status 0: the host half of the decoding on rows [a, T) of the host arrays (rings, for a rolling horizon)."""
        multiple_pitch_bends, midi_tempo = self._decoding[5], self._decoding[7]
        if self.horizon_rows is None:
            events = _notes.decode_candidates(self._note[:T], self._bits[:T], self._bend[:T], self._prm)
        else:
            events = _notes.decode_candidates(_unwrapped(self._note, a, T), _unwrapped(self._bits, a, T),
                                              _unwrapped(self._bend, a, T), self._prm, first_frame=a)
        return (_notes.note_events_to_midi(events, multiple_pitch_bends, midi_tempo) if midi else None), events

    def _host_decoded(self):
        """Status 1 — a NaN in the maps or an onset threshold <= 0: numpy's rules, the host decodes the maps themselves."""
        s = self.stream
        multiple_pitch_bends, midi_tempo = self._decoding[5], self._decoding[7]
        if self.horizon_rows is None:
            # (After a NaN the tail's windows run a second time here: the update wrote them behind the kept rows,
            # frequency-constrained, and the decoder needs the rows as the caller gets them.  The price of a broken input, not
            # of an update.)
            parts = self._rows + [s.peek()]
            model_output = {k: np.ascontiguousarray(np.concatenate([r[k] for r in parts])) for k, _ in _inf._MAPS}
            return _inf._output_to_notes(model_output, *self._decoding)
        a, maps = s.rolling_maps()  # the kept maps of the slice
        p = self._prm
        ev, bends, n = _notes._decode(maps["note"], maps["onset"], maps["contour"], self._decoding[0], self._decoding[1],
                                      p.min_note_len, True, self._decoding[4], self._decoding[3], bool(p.melodia_trick),
                                      _notes.ENERGY_TOLERANCE, True)
        flat = bends.tolist()
        frames = np.array([[e.start_frame, e.end_frame] for e in ev[:n]], dtype=np.int64).reshape(n, 2) + a
        times = _notes.frames_to_time_at(frames)
        events = [(float(t[0]), float(t[1]), int(e.pitch_midi), np.float32(e.amplitude), flat[e.bend_offset : e.bend_offset + e.n_bends])
                  for e, t in zip(ev[:n], times)]
        return _notes.note_events_to_midi(events, multiple_pitch_bends, midi_tempo), events

    def _rolling_transcript(self):
        s = self.stream
        status = 1  # an onset threshold <= 0 is status 1 whatever the maps hold: no device work for it
        if self._prm.onset_threshold > 0:
            a, T, status = s.candidates_rolling(self._note, self._bits, self._bend, self._held)
            self._held = s.rows  # rows at or after it were a tail's: sent again next time
        return self._decoded(a, T) if status == 0 else self._host_decoded()

    def _room(self, rows: int) -> None:
        """Host note / bend / bitmap arrays of at least `rows` rows, the held final rows carried over."""
        if rows <= self._note.shape[0]:
            return
        cap = max(rows, 2 * self._note.shape[0], 1024)
        for name in ("_note", "_bend", "_bits"):
            old = getattr(self, name)
            new = np.empty((cap, old.shape[1]), old.dtype)
            new[: self._held] = old[: self._held]
            setattr(self, name, new)

    def transcript(self):
        """`(midi_data, note_events)` of the audio pushed so far, as `predict()` returns them for that audio."""
        if not self.live:
            raise ValueError("transcript() needs StreamingTranscriber(live=True)")
        if self.horizon_rows is not None:
            return self._rolling_transcript()
        s = self.stream
        status, T = 1, 0  # an onset threshold <= 0 is status 1 whatever the maps hold: no device work for it
        if self._prm.onset_threshold > 0:
            self._room(s.rows + s.rows_bound(0))
            T, status = s.candidates(self._note, self._bits, self._bend, self._held)
            self._held = s.rows  # rows at or after it were a tail's: sent again next time
        return self._decoded(0, T) if status == 0 else self._host_decoded()

    def finish(self):
        if self.horizon_rows is not None:
            rows = self.stream.finish()
            midi_data, note_events = self._rolling_transcript()  # a finished stream has no tail: the final slice
            self.stream.close()
            return rows, midi_data, note_events
        self._rows.append(self.stream.finish())
        self.stream.close()
        model_output = {k: np.ascontiguousarray(np.concatenate([r[k] for r in self._rows])) for k, _ in _inf._MAPS}
        return (model_output,) + _inf._output_to_notes(model_output, *self._decoding)

    def close(self) -> None:
        self.stream.close()

    def __enter__(self) -> "StreamingTranscriber":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()
