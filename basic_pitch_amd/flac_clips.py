"""Many FLAC files' bytes in one native call, decoded on the device (include/basic_pitch_amd_flac_clips.h).

Datasets of short excerpts are stored as FLAC.  `bp_infer_flac_candidates` decodes one file per call — four launches, an
upload and a wait for a few dozen frames — and `bp_infer_clips_candidates` takes PCM only.  `bp_infer_flac_clips_candidates` /
`bp_infer_flac_clips_events` take the bytes of a whole job: the four decode stages run once for all clips
(csrc/flac_clips.hip, the device code of the single-file decoder on a table of streams), and the samples go on, on the device,
to what the PCM clips calls run.  Clip by clip the bytes are those of the single-file call (tests/test_gpu_flac_clips.py).
`Model.transcribe_flac_clips` is the public entry; this module binds the prototypes and holds the host side.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import clips as _clips
from . import events as _events
from . import note_creation as _notes

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_pi64 = C.POINTER(C.c_int64)

HOST, FAILED = _native.BP_CLIP_FLAC_HOST, _native.BP_CLIP_FLAC_FAILED


class bp_flac_clip(C.Structure):
    _fields_ = [("file", C.c_void_p), ("nbytes", C.c_size_t)]


# name -> (restype, argtypes), as include/basic_pitch_amd_flac_clips.h declares them (tests/test_flac_clips_cpu.py compares)
PROTOTYPES = {
    "bp_flac_clips_row_offsets": (_int, [_vp, _i64, _vp, _int, _pi64, _vp]),
    "bp_flac_clips_decode_device": (_int, [_vp, _i64, _vp, _vp, _pi64, _vp]),
    "bp_infer_flac_clips_candidates": (_int, [_vp, _i64, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "bp_infer_flac_clips_events": (_int, [_vp, _i64, _vp, _int, _vp, _vp, _i64, _vp, _i64, _pi64, _vp]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the prototypes of include/basic_pitch_amd_flac_clips.h on a loaded library."""
    return _native.bind(lib, PROTOTYPES)


def clip_table(blobs: Sequence[Any]):
    """(the `bp_flac_clip` array of bytes-like objects, what keeps their memory alive)."""
    keep = [np.frombuffer(b, np.uint8) for b in blobs]
    tab = (bp_flac_clip * max(1, len(keep)))()
    for i, a in enumerate(keep):
        tab[i] = bp_flac_clip(a.ctypes.data if a.size else None, a.size)
    return tab, keep


def left_to_host(lay: Optional[Dict[str, int]], nbytes: int) -> bool:
    """The pure-Python mirror of the host-side status: True where the calls report BP_CLIP_FLAC_HOST.  `lay`: the clip's
    `Model.flac_layout`, None where that fails."""
    if lay is None or nbytes < 42:
        return True
    n, lo, hi = lay["n_frames"], lay["min_block"], lay["max_block"]
    if not (n > 0 and lo >= 16 and hi >= lo and 4 <= lay["bits_per_sample"] <= 24 and lay["channels"] <= 8 and nbytes < 1 << 31
            and n * lay["channels"] < 1 << 33 and lay["audio_start"] < nbytes):
        return True
    slots = (n + lo - 1) // lo + 1  # a row of max_block samples of scratch per frame slot
    return slots * hi > 8 * n + 2 * hi


def row_offsets(layouts: Sequence[Optional[Dict[str, int]]], nbytes: Sequence[int], sample_rate: int, **geometry: int
                ) -> Tuple[np.ndarray, np.ndarray]:
    """The pure-Python mirror of `bp_flac_clips_row_offsets`: (offsets, status); a clip left to the host counts no rows."""
    status = np.array([HOST if left_to_host(l, b) else 0 for l, b in zip(layouts, nbytes)], np.int32).reshape(-1)
    frames = [0 if s else l["n_frames"] for l, s in zip(layouts, status)]
    return _clips.row_offsets(frames, sample_rate, **geometry), status


def group_by_rate(layouts: Sequence[Optional[Dict[str, int]]]) -> Tuple[Dict[int, List[int]], List[int]]:
    """({rate: the indices of its clips, in order}, rates in order of first appearance; the indices without a layout)."""
    groups: Dict[int, List[int]] = {}
    none: List[int] = []
    for i, lay in enumerate(layouts):
        if lay is None:
            none.append(i)
        else:
            groups.setdefault(int(lay["sample_rate"]), []).append(i)
    return groups, none


def flac_clips_row_offsets(model: Any, blobs: Sequence[Any], sample_rate: int) -> Tuple[np.ndarray, np.ndarray]:
    """`bp_flac_clips_row_offsets` on `model`'s handle (no GPU work): (offsets, status)."""
    lib = bind(model._lib)
    tab, keep = clip_table(blobs)
    offs = np.zeros(len(keep) + 1, np.int64)
    status = np.zeros(max(1, len(keep)), np.int32)
    rc = lib.bp_flac_clips_row_offsets(model._handle, len(keep), tab, int(sample_rate), offs.ctypes.data_as(_pi64), status.ctypes.data)
    _native.check(lib, model._handle, rc, "bp_flac_clips_row_offsets")
    return offs, status[: len(keep)]


def decode_device(model: Any, blobs: Sequence[Any]) -> Tuple[List[Optional[np.ndarray]], np.ndarray]:
    """`bp_flac_clips_decode_device`: ([int32 samples [n_frames, channels] or None where the status is not 0], status)."""
    lib = bind(model._lib)
    tab, keep = clip_table(blobs)
    shapes = []
    for b, a in zip(blobs, keep):
        try:
            lay = model.flac_layout(bytes(b)) if a.size >= 42 else None
        except ValueError:
            lay = None
        shapes.append((max(0, lay["n_frames"]), lay["channels"]) if lay else (0, 1))
    offs = np.concatenate([[0], np.cumsum([n * c for n, c in shapes])]).astype(np.int64)
    pcm = np.zeros(max(1, int(offs[-1])), np.int32)
    status = np.zeros(max(1, len(keep)), np.int32)
    rc = lib.bp_flac_clips_decode_device(model._handle, len(keep), tab, pcm.ctypes.data, offs.ctypes.data_as(_pi64), status.ctypes.data)
    _native.check(lib, model._handle, rc, "bp_flac_clips_decode_device")
    return [pcm[offs[i] : offs[i + 1]].reshape(shapes[i]) if status[i] == 0 else None for i in range(len(keep))], status[: len(keep)]


def infer_flac_clips_candidates(model: Any, blobs: Sequence[Any], sample_rate: int, prm: Any):
    """One `bp_infer_flac_clips_candidates` call for FLAC clips of one rate: as `clips.infer_clips_candidates`."""
    lib = bind(model._lib)
    tab, keep = clip_table(blobs)
    fixed = (model._handle, len(keep), tab, int(sample_rate))
    return _clips._call(lib, model._handle, "bp_infer_flac_clips_candidates", lib.bp_infer_flac_clips_candidates, fixed,
                        flac_clips_row_offsets(model, blobs, sample_rate)[0], prm)


def infer_flac_clips_events(model: Any, blobs: Sequence[Any], sample_rate: int, prm: Any, room: Optional[Tuple[int, int]] = None):
    """One `bp_infer_flac_clips_events` call for FLAC clips of one rate: as `events.infer_clips_events`."""
    lib = bind(model._lib)
    tab, keep = clip_table(blobs)
    rows = int(flac_clips_row_offsets(model, blobs, sample_rate)[0][-1])
    fixed = (model._handle, len(keep), tab, int(sample_rate), C.addressof(prm))
    return _events._call(lib, model._handle, "bp_infer_flac_clips_events", lib.bp_infer_flac_clips_events, fixed, len(keep), rows, room)


def host_decode(lib: C.CDLL, blob: Any) -> Tuple[np.ndarray, int]:
    """The host decoder (csrc/flac_decode.cpp, the route `audio.read_flac` takes) on a clip's bytes: (float32 [n, channels],
    rate); ValueError with the decoder's message."""
    data = bytes(blob)
    ch, sr, bits, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    if not data or lib.bp_flac_info(data, len(data), C.byref(ch), C.byref(sr), C.byref(bits), C.byref(n)) != _native.BP_OK:
        raise ValueError(lib.bp_audio_last_error().decode(errors="replace") if data else "empty")
    pcm = np.empty((n.value, ch.value), dtype=np.float32)
    got = C.c_int64()
    rc = lib.bp_flac_decode(data, len(data), pcm.ctypes.data, n.value, C.byref(got))
    if rc != _native.BP_OK or got.value != n.value:
        raise ValueError(lib.bp_audio_last_error().decode(errors="replace"))
    return pcm, sr.value


def transcribe_flac_clips(model: Any, blobs: Sequence[Any], onset_threshold: float, frame_threshold: float,
                          minimum_note_length: float, minimum_frequency: Optional[float], maximum_frequency: Optional[float],
                          multiple_pitch_bends: bool, melodia_trick: bool, midi_tempo: float, threads: int = 8,
                          decode: str = "host", errors: str = "raise") -> List[Any]:
    """`Model.transcribe_flac_clips`: the clips grouped by STREAMINFO rate, one native call per group; the clips the device
    decoder leaves to the host or fails on — and those with status 1 or 2 — decoded by the host decoder and taken through
    `clips.transcribe_clips`, the PCM path.  Results in input order."""
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    if errors not in ("raise", "return"):
        raise ValueError(f"errors must be 'raise' or 'return', got {errors!r}")
    from . import inference as _inf

    lib = model._lib
    layouts: List[Optional[Dict[str, int]]] = []
    for b in blobs:
        try:
            layouts.append(model.flac_layout(bytes(b)))
        except ValueError:
            layouts.append(None)
    prm = _notes._note_params(onset_threshold, frame_threshold, _inf._min_note_len_frames(minimum_note_length), True,
                              maximum_frequency, minimum_frequency, melodia_trick, _notes.ENERGY_TOLERANCE, True)
    results: List[Any] = [None] * len(blobs)
    groups, on_host = group_by_rate(layouts)

    _clips.transcribe_groups(groups.items(), lambda ids, rate: infer_flac_clips_candidates(model, [blobs[i] for i in ids], rate, prm),
                             lambda ids, rate: infer_flac_clips_events(model, [blobs[i] for i in ids], rate, prm),
                             on_host.append, results, prm, decode, multiple_pitch_bends, midi_tempo, threads)
    # the host decoder's clips: the PCM path, all in one job (which itself falls back for its statuses 1 and 2)
    arrays, rates, ids = [], [], []
    for i in sorted(on_host):
        try:
            a, sr = host_decode(lib, blobs[i])
        except ValueError as e:
            err = ValueError(f"clip {i}: {e}")
            if errors == "raise":
                raise err from None
            results[i] = err
            continue
        arrays.append(a), rates.append(sr), ids.append(i)
    if arrays:
        done = _clips.transcribe_clips(model, arrays, rates, onset_threshold, frame_threshold, minimum_note_length, minimum_frequency,
                                       maximum_frequency, multiple_pitch_bends, melodia_trick, midi_tempo, threads, decode)
        for i, r in zip(ids, done):
            results[i] = r
    return results
