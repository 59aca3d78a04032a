"""Many IMA ADPCM files' bytes in one native call, expanded on the device (include/basic_pitch_amd_adpcm.h).

Call recordings and voice archives are short files of RIFF/WAVE format tag 0x11 (or CAF `ima4`).  `bp_infer_adpcm_clips_events`
takes the bytes of a whole job: one copy, ONE decode launch for all clips (csrc/adpcm_device.hip, a segment per clip), and the
samples go on, on the device, to what `bp_infer_clips_events` runs.  `Model.transcribe_adpcm_clips` is the public entry; this
module holds its host side.  The prototypes are bound in `_native.load_library`.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import clips as _clips
from . import events as _events
from . import note_creation as _notes

_pi64 = C.POINTER(C.c_int64)


def clip_table(blobs: Sequence[Any]):
    """(the `bp_adpcm_clip` array of bytes-like objects, what keeps their memory alive)."""
    keep = [np.frombuffer(b, np.uint8) for b in blobs]
    tab = (_native.bp_adpcm_clip * max(1, len(keep)))()
    for i, a in enumerate(keep):
        tab[i] = _native.bp_adpcm_clip(a.ctypes.data if a.size else None, a.size)
    return tab, keep


def host_decode(lib: C.CDLL, blob: Any) -> Tuple[np.ndarray, Dict[str, int]]:
    """The host decoder (csrc/adpcm_file.cpp) on a file's bytes: (int16 [n_frames, channels], the layout's fields); ValueError
    with the parser's message."""
    data = bytes(blob)
    lay = _native.bp_adpcm_layout()
    if lib.bp_adpcm_layout_of(data, len(data), C.byref(lay)) != _native.BP_OK:
        raise ValueError(lib.bp_files_last_error().decode(errors="replace"))
    pcm = np.empty((lay.n_frames, lay.channels), np.int16)
    got = C.c_int64()
    rc = lib.bp_adpcm_decode(data, len(data), pcm.ctypes.data, lay.n_frames, C.byref(got))
    if rc != _native.BP_OK or got.value != lay.n_frames:
        raise ValueError(lib.bp_files_last_error().decode(errors="replace"))
    return pcm, {k: int(getattr(lay, k)) for k, _ in lay._fields_}


def infer_adpcm_clips_events(model: Any, blobs: Sequence[Any], prm: Any, room: Optional[Tuple[int, int]] = None):
    """One `bp_infer_adpcm_clips_events` call for files of one codec, rate and channel count: as `events.infer_clips_events`."""
    lib = model._lib
    tab, keep = clip_table(blobs)
    lays = [model.adpcm_layout(bytes(b)) for b in blobs]
    rows = sum(int(model._pcm_frames(l["n_frames"], l["sample_rate"])) for l in lays)
    fixed = (model._handle, len(keep), tab, C.addressof(prm))
    return _events._call(lib, model._handle, "bp_infer_adpcm_clips_events", lib.bp_infer_adpcm_clips_events, fixed, len(keep), rows, room)


def transcribe_adpcm_clips(model: Any, blobs: Sequence[Any], onset_threshold: float, frame_threshold: float,
                           minimum_note_length: float, minimum_frequency: Optional[float], maximum_frequency: Optional[float],
                           multiple_pitch_bends: bool, melodia_trick: bool, midi_tempo: float, threads: int = 8,
                           decode: str = "device") -> List[Any]:
    """`Model.transcribe_adpcm_clips`: the files grouped by (codec, rate, channels), one native call per group; a clip with
    status 1 or 2, and every clip with decode="host", is decoded by the host decoder and taken through
    `clips.transcribe_clips`, the PCM path.  Results in input order; ValueError names the first file that is no such file."""
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    from . import inference as _inf

    lib = model._lib
    layouts = []
    for i, b in enumerate(blobs):
        try:
            layouts.append(model.adpcm_layout(bytes(b)))
        except ValueError as e:
            raise ValueError(f"clip {i}: {e}") from None
    prm = _notes._note_params(onset_threshold, frame_threshold, _inf._min_note_len_frames(minimum_note_length), True,
                              maximum_frequency, minimum_frequency, melodia_trick, _notes.ENERGY_TOLERANCE, True)
    results: List[Any] = [None] * len(blobs)
    on_host: List[int] = []
    if decode == "device":
        groups: Dict[Tuple[int, int, int], List[int]] = {}
        for i, l in enumerate(layouts):
            groups.setdefault((l["codec"], l["sample_rate"], l["channels"]), []).append(i)
        _clips.transcribe_groups(groups.items(), None, lambda ids, _key: infer_adpcm_clips_events(model, [blobs[i] for i in ids], prm),
                                 on_host.append, results, prm, decode, multiple_pitch_bends, midi_tempo, threads)
    else:
        on_host = list(range(len(blobs)))
    if on_host:
        ids = sorted(on_host)
        arrays = [host_decode(lib, blobs[i])[0] for i in ids]
        done = _clips.transcribe_clips(model, arrays, [layouts[i]["sample_rate"] for i in ids], onset_threshold, frame_threshold,
                                       minimum_note_length, minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick,
                                       midi_tempo, threads, decode)
        for i, r in zip(ids, done):
            results[i] = r
    return results
