"""Many short clips in one native call: raw PCM in, note events out (include/basic_pitch_amd_clips.h).

A clip of 1 to 15 windows is under 40 us of device work behind about ten launches and a wait when it goes through
`bp_infer_pcm_raw_candidates` alone.  `bp_infer_clips_candidates` takes a whole job of clips: one downmix and one resampling
launch for all of them, their windows packed into full batches, the dense half of note decoding for every clip as its own
track.  Clip by clip the bytes are those of the single-clip call (tests/test_gpu_clips.py), so the events are those of
`predict`.  `Model.transcribe_clips` is the public entry; this module binds the two prototypes and holds the host side.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import jobs as _jobs
from . import note_creation as _notes

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)


class bp_clip(C.Structure):
    _fields_ = [("pcm", C.c_void_p), ("n_frames", C.c_int64), ("format", C.c_int), ("channels", C.c_int)]


# name -> (restype, argtypes), as include/basic_pitch_amd_clips.h declares them (tests/test_clips_cpu.py compares)
PROTOTYPES = {
    "bp_clips_row_offsets": (_int, [_vp, _i64, _vp, _int, _pi64]),
    "bp_infer_clips_candidates": (_int, [_vp, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
}

# the BP_PCM_* code of each numpy sample type a clip may have: the little-endian types and their big-endian forms (what an
# AIFF, CAF or AU file holds).  Packed 24-bit PCM and G.711 have no numpy type, and int8 stays refused here as it always
# was (tests/test_clips_cpu.py): they go through predict_pcm_raw / open_stream(fmt=...) with BP_PCM_S24[_BE], BP_PCM_ULAW /
# BP_PCM_ALAW and BP_PCM_S8.
FORMATS = {np.dtype("<f4"): _native.BP_PCM_F32, np.dtype("<i2"): _native.BP_PCM_S16,
           np.dtype("<i4"): _native.BP_PCM_S32, np.dtype(np.uint8): _native.BP_PCM_U8,
           np.dtype("<f8"): _native.BP_PCM_F64, np.dtype(">i2"): _native.BP_PCM_S16_BE,
           np.dtype(">i4"): _native.BP_PCM_S32_BE, np.dtype(">f4"): _native.BP_PCM_F32_BE,
           np.dtype(">f8"): _native.BP_PCM_F64_BE}


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_clips.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def as_clip(clip: Any, index: int) -> np.ndarray:
    """Clip `index` as the C-contiguous [n_frames, channels] array the library reads; ValueError names the clip."""
    a = np.asarray(clip)
    if a.dtype not in FORMATS:
        raise ValueError(f"clip {index}: samples must be float32, int16, int32, uint8 or float64 (either byte order), got {a.dtype}")
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or not 1 <= a.shape[1] <= 64:
        raise ValueError(f"clip {index}: expected [n_frames] or [n_frames, channels] with 1 to 64 channels, got shape {np.shape(clip)}")
    return np.ascontiguousarray(a)


def clip_table(arrays: Sequence[np.ndarray]):
    """The `bp_clip` array of [n_frames, channels] arrays (which must outlive it)."""
    tab = (bp_clip * max(1, len(arrays)))()
    for i, a in enumerate(arrays):
        tab[i] = bp_clip(a.ctypes.data if a.size else None, a.shape[0], FORMATS[a.dtype], a.shape[1])
    return tab


def n_rows(n_frames: int, sample_rate: int, model_rate: int = 22050, hop: int = 36164, lead: int = 3840) -> int:
    """Rows of the maps of a clip of `n_frames` at `sample_rate`, without the library: ceil(n * rate / sample_rate) samples at
    the model's rate, then min(int(samples / hop * 142), windows * 142) with windows = ceil((samples + lead) / hop)
    (`bp_handle_track_n_frames(bp_handle_resampled_length(...))`; hop and lead-in double for the extended 44.1 kHz geometry)."""
    if n_frames <= 0:
        return 0
    n = (int(n_frames) * model_rate + sample_rate - 1) // sample_rate
    windows = (n + lead + hop - 1) // hop
    return min(int(n / hop * 142), windows * 142)


def row_offsets(n_frames: Sequence[int], sample_rate: int, **geometry: int) -> np.ndarray:
    """The pure-Python mirror of `bp_clips_row_offsets`: offsets[i] = rows of the clips before clip i, offsets[-1] = all rows."""
    return np.concatenate([[0], np.cumsum([n_rows(n, sample_rate, **geometry) for n in n_frames], dtype=np.int64)]).astype(np.int64)


def clips_row_offsets(model: Any, arrays: Sequence[np.ndarray], sample_rate: int) -> np.ndarray:
    """`bp_clips_row_offsets` for [n_frames, channels] arrays on `model`'s handle (no GPU work)."""
    lib = bind(model._lib)
    offs = np.zeros(len(arrays) + 1, np.int64)
    rc = lib.bp_clips_row_offsets(model._handle, len(arrays), clip_table(arrays), int(sample_rate), offs.ctypes.data_as(_pi64))
    _native.check(lib, model._handle, rc, "bp_clips_row_offsets")
    return offs


def _call(lib, handle, what: str, fn, fixed: tuple, offs: np.ndarray, prm: Any
          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray], np.ndarray]:
    """`fn(*fixed, prm, note_out, cand_bits, bend_map, status)` with the outputs the row offsets ask for: (offsets, note (T, 88)
    float32, onset-peak bitmap (T, 12) uint8, bend map (T, 88) int8 or None, status per clip), the rows of clip i at
    offsets[i]:offsets[i + 1]."""
    n, T = len(offs) - 1, int(offs[-1])
    note = np.empty((T, 88), np.float32)
    bits = np.empty((T, 12), np.uint8)
    bend = np.empty((T, 88), np.int8) if prm.include_pitch_bends else None
    status = np.zeros(max(1, n), np.int32)
    rc = fn(*fixed, C.addressof(prm), note.ctypes.data, bits.ctypes.data, bend.ctypes.data if bend is not None else None,
            status.ctypes.data)
    _native.check(lib, handle, rc, what)
    return offs, note, bits, bend, status[:n]


def infer_clips_candidates(model: Any, arrays: Sequence[np.ndarray], sample_rate: int, prm: Any):
    """One `bp_infer_clips_candidates` call for [n_frames, channels] arrays at one rate: as `_call` returns."""
    lib = bind(model._lib)
    return _call(lib, model._handle, "bp_infer_clips_candidates", lib.bp_infer_clips_candidates,
                 _jobs.clips_source(model, arrays, sample_rate), clips_row_offsets(model, arrays, sample_rate), prm)


def transcribe_groups(groups, candidates, events, fallback, results: List[Any], prm: Any, decode: str, multiple_pitch_bends: bool,
                      midi_tempo: float, threads: int) -> None:
    """The loop over the rate groups of a job, `groups` = [(rate, the indices of its clips)]: one native call per group —
    `events(ids, rate)` for decode="device", else `candidates(ids, rate)` — then per clip either `fallback(i)` (a status: on
    this thread, between the native calls, as it may use the handle), or the device's events straight to MIDI, or the
    sequential half of note decoding on a thread pool (the native decoder releases the GIL).  Fills results[i]."""
    from . import events as _events

    def decoded(note, bits, bend):
        ev = _notes.decode_candidates(note, bits, bend, prm)
        return _notes.note_events_to_midi(ev, multiple_pitch_bends, midi_tempo), ev

    with ThreadPoolExecutor(max_workers=max(1, int(threads))) as pool:
        pending = []
        for rate, ids in groups:
            if decode == "device":
                evs, bends, ev_offs, status = events(ids, rate)
            else:
                offs, note, bits, bend, status = candidates(ids, rate)
            for k, i in enumerate(ids):
                if status[k]:  # 1: a NaN, or an onset threshold <= 0; 2: the clip passed its region's capacity; 3, 4: FLAC
                    fallback(i)
                elif decode == "device":
                    ev = _events.clip_events(evs, bends, ev_offs, k, True)
                    results[i] = (_notes.note_events_to_midi(ev, multiple_pitch_bends, midi_tempo), ev)
                else:
                    r0, r1 = int(offs[k]), int(offs[k + 1])
                    pending.append((i, pool.submit(decoded, note[r0:r1], bits[r0:r1], bend[r0:r1] if bend is not None else None)))
        for i, fut in pending:
            results[i] = fut.result()


def transcribe_clips(model: Any, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], onset_threshold: float,
                     frame_threshold: float, minimum_note_length: float, minimum_frequency: Optional[float],
                     maximum_frequency: Optional[float], multiple_pitch_bends: bool, melodia_trick: bool, midi_tempo: float,
                     threads: int = 8, decode: str = "host") -> List[Tuple[Any, List["_notes.NoteEvent"]]]:
    """`Model.transcribe_clips`: clips grouped by rate, one native call per group, the sequential half of note decoding per clip
    on a thread pool (the native decoder releases the GIL), results in input order.  decode="device": that half runs on the
    device too (`bp_infer_clips_events`, basic_pitch_amd/events.py) and only events and bends come home."""
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    from . import events as _events
    from . import inference as _inf

    arrays = [as_clip(c, i) for i, c in enumerate(clips)]
    rates = _jobs.rates_of(arrays, sample_rates)
    prm = _notes._note_params(onset_threshold, frame_threshold, _inf._min_note_len_frames(minimum_note_length), True,
                              maximum_frequency, minimum_frequency, melodia_trick, _notes.ENERGY_TOLERANCE, True)
    results: List[Any] = [None] * len(arrays)

    def host_decoded(i: int):
        a = arrays[i]  # a status: the maps themselves decide, as predict does
        out = model.predict_pcm_raw(a, FORMATS[a.dtype], a.shape[0], a.shape[1], rates[i])
        results[i] = _inf._output_to_notes(out, onset_threshold, frame_threshold, minimum_note_length, minimum_frequency,
                                           maximum_frequency, multiple_pitch_bends, melodia_trick, midi_tempo)

    transcribe_groups(_jobs.rate_groups(rates), lambda ids, rate: infer_clips_candidates(model, [arrays[i] for i in ids], rate, prm),
                      lambda ids, rate: _events.infer_clips_events(model, [arrays[i] for i in ids], rate, prm),
                      host_decoded, results, prm, decode, multiple_pitch_bends, midi_tempo, threads)
    return results
