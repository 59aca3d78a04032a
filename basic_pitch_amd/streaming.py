"""Streaming sessions: audio that arrives over time -> posteriorgram rows as they become final.

The reference has no such interface (its `predict` takes a finished file); this is the library's `bp_stream_*` family
(include/basic_pitch_amd.h, csrc/stream_api.hip) behind `Model.open_stream`, `Model.push_streams` and
`StreamingTranscriber`.  The rows a stream emits, concatenated, are bit for bit what `Model.predict_pcm_raw` returns for
the concatenated input, for any chunking.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import inference as _inf

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

# the numpy type a chunk of each format is made of (BP_PCM_S24: packed bytes)
_DTYPES = {_native.BP_PCM_F32: np.float32, _native.BP_PCM_S16: np.int16, _native.BP_PCM_S24: np.uint8,
           _native.BP_PCM_S32: np.int32, _native.BP_PCM_U8: np.uint8, _native.BP_PCM_F64: np.float64}


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the streaming family's prototypes on a loaded library."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


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
        self._frame_bytes = self.channels * _native.BP_PCM_WAV[self.fmt][1] // 8
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
    arr = lambda vals: (C.c_void_p * n)(*vals)  # noqa: E731
    rows = (C.c_int64 * n)()
    rc = lib.bp_streams_push(
        model._handle, n, arr([s._s.value for s in streams]), arr([b.ctypes.data if k else None for b, k in parts]),
        (C.c_int64 * n)(*[k for _, k in parts]), _native.BP_MEM_HOST,
        *[arr([_inf._ptr(o[k]) for o in outs]) for k, _ in _inf._MAPS],
        (C.c_int64 * n)(*[o["note"].shape[0] for o in outs]), _native.BP_MEM_HOST, rows,
    )
    _native.check(lib, model._handle, rc, "bp_streams_push")
    return [s._taken(o, int(r)) for s, o, r in zip(streams, outs, rows)]


class StreamingTranscriber:
    """`predict()` for audio that arrives in chunks: `push(chunk)` feeds a stream and keeps the emitted rows on the host,
    `finish()` returns `(model_output, midi_data, note_events)` exactly as `predict()` does for the same audio.

    Note decoding stays a whole-track step at `finish()`: the melodia pass of `output_to_notes_polyphonic` walks the whole
    posteriorgram, so a note is only known once the track is.  Incremental note events are out of scope; what arrives
    incrementally are the posteriorgram rows (`push` returns them)."""

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
    ):
        self._decoding = (onset_threshold, frame_threshold, minimum_note_length, minimum_frequency, maximum_frequency,
                          multiple_pitch_bends, melodia_trick, midi_tempo)
        self.stream = Stream(_inf._model_from(model_or_model_path), sample_rate, channels, fmt)
        self._rows: List[Dict[str, np.ndarray]] = []

    def push(self, chunk: Any) -> Dict[str, np.ndarray]:
        out = self.stream.push(chunk)
        self._rows.append(out)
        return out

    def finish(self):
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
