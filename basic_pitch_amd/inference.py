"""Host-side mirror of the reference's inference interface for the hot path.

Same names, argument meaning and error behaviour as `basic_pitch/inference.py` (spotify/basic-pitch
v0.4.0): `Model` (71-182), `window_audio_file` (194-219), `get_audio_input` (222-244),
`unwrap_output` (247-279), `run_inference` (282-330), `predict` (431-506).  The arithmetic runs in
libbasicpitch_amd.so (hand-written HIP for gfx950) — there is no CPU execution path here.

Differences by design (the GPU needs batches; the reference loops batch-1):
  * `Model.predict(x)` takes any n >= 0 windows per call (the frozen graph's batch dim is dynamic);
  * `run_inference` sends the whole track to the device once (`bp_infer_track`: windowing and
    un-overlapping happen on the GPU) instead of calling predict once per window.
Both produce the values the per-window loop would.
"""
from __future__ import annotations

import csv
import ctypes as C
import enum
import json
import os
import pathlib
import threading
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import audio as _audio
from . import note_creation as infer
from . import weights as _weights
from .constants import (
    ANNOTATIONS_FPS,
    AUDIO_N_SAMPLES,
    AUDIO_SAMPLE_RATE,
    AUDIO_WINDOW_LENGTH,
    FFT_HOP,
    ANNOT_N_FRAMES,
    N_FREQ_BINS_CONTOURS,
    N_FREQ_BINS_NOTES,
)

DEFAULT_ONSET_THRESHOLD = 0.5
DEFAULT_FRAME_THRESHOLD = 0.3
DEFAULT_MINIMUM_NOTE_LENGTH_MS = 127.7
DEFAULT_MINIMUM_MIDI_TEMPO = 120
DEFAULT_SONIFICATION_SAMPLERATE = 44100
DEFAULT_OVERLAPPING_FRAMES = 30
DEFAULT_MIDI_VELOCITY_SCALE = 127

PKG_DIR = pathlib.Path(__file__).parent
ICASSP_2022_MODEL_PATH = PKG_DIR / "assets" / "nmp_weights.bin"


def _is_torch_cuda(x: Any) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda") and bool(x.is_cuda)


# the model's three posteriorgrams and their widths, in the order the native calls take their pointers
_MAPS = (("note", N_FREQ_BINS_NOTES), ("onset", N_FREQ_BINS_NOTES), ("contour", N_FREQ_BINS_CONTOURS))

# samples two neighbouring windows share / samples from one window's start to the next (inference.py:303-305)
_OVERLAP_LEN = DEFAULT_OVERLAPPING_FRAMES * FFT_HOP
_HOP_SIZE = AUDIO_N_SAMPLES - _OVERLAP_LEN

_WAV_PCM = {wav: fmt for fmt, wav in _native.BP_PCM_WAV.items()}  # WAV (format tag, bits) -> BP_PCM_*


def _empty_maps(lead: Tuple[int, ...], device: Any = None) -> Dict[str, Any]:
    """Fresh C-contiguous float32 {"note","onset","contour"} of shape `lead` + (width,): numpy arrays, or torch tensors
    on `device` when one is given."""
    if device is None:
        return {k: np.empty(lead + (w,), dtype=np.float32) for k, w in _MAPS}
    import torch

    return {k: torch.empty(lead + (w,), dtype=torch.float32, device=device) for k, w in _MAPS}


def _ptr(a: Any) -> int:
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _mem_kind(a: Any) -> int:
    return _native.BP_MEM_HOST if isinstance(a, np.ndarray) else _native.BP_MEM_DEVICE


class Model:
    """Drop-in for `basic_pitch.inference.Model`: load a serialized model, `predict(x) -> dict`.

    `model_path` is the serialized model, as in the reference: its `saved_models/icassp_2022/nmp.onnx` (the 18
    constants are extracted at load, basic_pitch_amd/weights.py; the `nmp/`, `nmp.tflite` and `nmp.mlpackage`
    artifacts resolve to the `nmp.onnx` next to them), or the pre-extracted blob shipped with this package
    (`ICASSP_2022_MODEL_PATH`, the default).  Like the reference (inference.py:148-154) an unloadable file raises
    ValueError; a missing HIP library / GPU raises NativeLibraryError.
    """

    class MODEL_TYPES(enum.Enum):
        MI355X_HIP = enum.auto()

    def __init__(
        self,
        model_path: Union[pathlib.Path, str] = ICASSP_2022_MODEL_PATH,
        device: int = 0,
        max_windows: int = 256,
        stage_timing: bool = False,
        time_dominant: bool = False,
        exact_f32_mfma: bool = False,
        bf16_weights: bool = False,
        ext_cqt_44k: bool = False,
        f16_corrections: bool = False,
        fp8_corrections: bool = False,
        blocking_wait: bool = False,
    ):
        self.model_type = Model.MODEL_TYPES.MI355X_HIP
        self._lib = _native.load_library()
        self._handle = C.c_void_p()
        blob = _weights.load_model_blob(model_path)  # ValueError if unloadable, like inference.py:148-154
        flags = 0
        for on, bit in (
            (stage_timing, _native.BP_FLAG_STAGE_TIMING),
            (time_dominant, _native.BP_FLAG_TIME_DOMINANT),  # HIP events around the dominant kernel only (2 records per chunk instead of 16)
            (exact_f32_mfma, _native.BP_FLAG_F32_MFMA),  # A/B reference: contour conv1 on the exact-f32 MFMA kernel
            (bf16_weights, _native.BP_FLAG_BF16_WEIGHTS),  # BASELINE.json configs[3]: conv weights rounded to bf16, 2 matrix instructions per product
            (ext_cqt_44k, _native.BP_FLAG_EXT_CQT_44K),  # BASELINE.json configs[4]: 44.1 kHz windows of 87,688 samples, 10-octave / 345-bin CQT
            (f16_corrections, _native.BP_FLAG_F16_CORRECTIONS),  # the default arithmetic since round 3 (all three split-precision products on f16): a no-op
            (fp8_corrections, _native.BP_FLAG_FP8_CORRECTIONS),  # retired in round 6: bp_create refuses the flag (ValueError)
            (blocking_wait, _native.BP_FLAG_BLOCKING_WAIT),  # whole-track calls sleep on an interrupt instead of spinning (file jobs: workers share cores)
        ):
            if on:
                flags |= bit
        rc = self._lib.bp_create(blob, len(blob), int(device), flags, int(max_windows), C.byref(self._handle))
        if rc != _native.BP_OK:
            self._handle = C.c_void_p()
            _native.check(self._lib, None, rc, f"File {model_path} cannot be loaded into the MI355X backend")
        self.device = int(device)
        self.max_windows = int(max_windows)
        # window length / sample rate of this handle's geometry (43844 @ 22050 unless ext_cqt_44k)
        self.audio_n_samples = int(self._lib.bp_handle_window_samples(self._handle))
        self.sample_rate = int(self._lib.bp_handle_sample_rate(self._handle))

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.bp_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "Model":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    # -- native call helpers ----------------------------------------------------------------------
    def _track_frames(self, n: int) -> int:
        """Rows of the un-overlapped posteriorgrams of a track of `n` samples at the model's rate."""
        return int(self._lib.bp_handle_track_n_frames(self._handle, n))

    def _pcm_frames(self, n_frames: int, sample_rate: int) -> int:
        """The same for `n_frames` of audio at `sample_rate`, resampled to the model's rate first."""
        return self._track_frames(int(self._lib.bp_handle_resampled_length(self._handle, int(n_frames), int(sample_rate))))

    def _use_torch_stream(self, device: Any) -> None:
        """Queue this handle's work on torch's current stream of `device`."""
        import torch

        self._lib.bp_set_stream(self._handle, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))

    def _infer(self, name: str, args: Tuple[Any, ...], out: Any, mem_kind: bool = True) -> None:
        """Call the library's `name(handle, *args, note, onset, contour[, BP_MEM_*])` and raise what its status maps to.
        `out`: the three maps, or (bp_infer_tracks) a list of them, passed as three arrays of pointers; whether they are
        numpy arrays or torch tensors decides the pointers and the memory kind."""
        if isinstance(out, list):
            ptrs = [(C.c_void_p * len(out))(*[_ptr(o[k]) for o in out]) for k, _ in _MAPS]
            first = out[0]["note"]
        else:
            ptrs = [_ptr(out[k]) for k, _ in _MAPS]
            first = out["note"]
        if mem_kind:
            ptrs.append(_mem_kind(first))
        _native.check(self._lib, self._handle, getattr(self._lib, name)(self._handle, *args, *ptrs), name)

    # -- inference --------------------------------------------------------------------------------
    def predict(self, x: Any) -> Dict[str, Any]:
        """x: float32 [n, 43844] or [n, 43844, 1] -> {"note","onset","contour"} (inference.py:156-182).

        numpy in -> fresh, writable, C-contiguous numpy arrays out (the reference's consumer mutates
        them, note_creation.py:338-341).  torch CUDA tensor in -> torch CUDA tensors out (zero copy).
        """
        return self._predict_device(x)

    def _predict_device(self, x: Any, out: Optional[Dict[str, Any]] = None, sync: bool = True) -> Dict[str, Any]:
        """`predict`; for a CUDA tensor `out` may name the tensors to fill, and `sync=False` returns without waiting for
        the device."""
        on_dev = _is_torch_cuda(x)
        if on_dev:
            import torch

            if x.dim() == 3 and x.shape[2] == 1:
                x = x[:, :, 0]
            if x.dim() != 2 or x.shape[1] != self.audio_n_samples or x.dtype != torch.float32:
                raise ValueError(f"expected float32 CUDA tensor of shape (n, {self.audio_n_samples}[, 1]), got {tuple(x.shape)}")
            if x.device.index != self.device:
                raise ValueError(f"input lives on cuda:{x.device.index}, model on cuda:{self.device}")
            x = x.contiguous()
        else:
            x = np.asarray(x)
            if x.ndim == 3 and x.shape[2] == 1:
                x = x[:, :, 0]
            if x.ndim != 2 or x.shape[1] != self.audio_n_samples:
                raise ValueError(f"expected input of shape (n, {self.audio_n_samples}[, 1]), got {x.shape}")
            x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        if out is None:
            out = _empty_maps((n, ANNOT_N_FRAMES), x.device if on_dev else None)
        if n and on_dev:
            self._use_torch_stream(x.device)
            self._infer("bp_infer_async", (_ptr(x), n), out, mem_kind=False)
            if sync:
                _native.check(self._lib, self._handle, self._lib.bp_synchronize(self._handle), "bp_synchronize")
        elif n:
            self._infer("bp_infer", (_ptr(x), n), out)
        return out

    def predict_track(self, samples: np.ndarray) -> Dict[str, np.ndarray]:
        """Whole mono 22.05 kHz track -> un-overlapped posteriorgrams (inference.py:282-315 on device)."""
        return self._predict_track_device(samples)

    def _predict_track_device(self, samples: "Any", out: Optional[Dict[str, "Any"]] = None) -> Dict[str, "Any"]:
        """`predict_track`; a device-resident track (1-D float32 CUDA tensor) -> device posteriorgrams (zero copy), into
        the tensors of `out` when given."""
        on_dev = _is_torch_cuda(samples)
        if on_dev:
            import torch

            if not (samples.dtype == torch.float32 and samples.dim() == 1):
                raise ValueError("expected a 1-D float32 CUDA tensor")
            samples = samples.contiguous()
        else:
            samples = np.ascontiguousarray(samples, dtype=np.float32)
            if samples.ndim != 1:
                raise ValueError("predict_track expects a 1-D mono signal")
        n = int(samples.shape[0])
        if out is None:
            out = _empty_maps((self._track_frames(n),), samples.device if on_dev else None)
        if on_dev:
            self._use_torch_stream(samples.device)
        self._infer("bp_infer_track", (_ptr(samples), n), out)
        return out

    def predict_tracks(self, tracks: "List[Any]") -> "List[Dict[str, Any]]":
        """Several mono 22.05 kHz tracks in one call, windows packed across track boundaries into full batches
        (bp_infer_tracks).  All numpy arrays (host in / host out) or all 1-D float32 CUDA tensors (device in / out)."""
        n = len(tracks)
        if n == 0:
            return []
        on_device = all(hasattr(t, "is_cuda") and t.is_cuda for t in tracks)
        if on_device:
            import torch

            tr = [t.contiguous() for t in tracks]
            if any(t.dtype != torch.float32 or t.dim() != 1 for t in tr):
                raise ValueError("expected 1-D float32 CUDA tensors")
            self._use_torch_stream(tr[0].device)
        else:
            tr = [np.ascontiguousarray(t, dtype=np.float32) for t in tracks]
            if any(t.ndim != 1 for t in tr):
                raise ValueError("predict_tracks expects 1-D mono signals")
        lens = [int(t.shape[0]) for t in tr]
        outs = [_empty_maps((self._track_frames(L),), tr[0].device if on_device else None) for L in lens]
        self._infer("bp_infer_tracks", (n, (C.c_void_p * n)(*[_ptr(t) for t in tr]), (C.c_int64 * n)(*lens)), outs)
        return outs

    @staticmethod
    def _as_pcm(pcm: np.ndarray) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 1:
            pcm = pcm[:, None]
        if pcm.ndim != 2 or pcm.shape[1] < 1:
            raise ValueError("expected PCM as float32 [n_frames] or [n_frames, channels]")
        return pcm

    def resample(self, pcm: np.ndarray, sample_rate: int) -> np.ndarray:
        """Decoded PCM [n_frames(, channels)] at `sample_rate` -> mono 22.05 kHz float32, computed on the device
        (channel mean + polyphase FIR; the `librosa.load(..., sr=22050, mono=True)` tail of inference.py:239)."""
        pcm = self._as_pcm(pcm)
        n_out = int(self._lib.bp_handle_resampled_length(self._handle, pcm.shape[0], int(sample_rate)))
        out = np.empty((n_out,), dtype=np.float32)
        rc = self._lib.bp_resample(
            self._handle, pcm.ctypes.data, pcm.shape[0], pcm.shape[1], int(sample_rate), out.ctypes.data, _native.BP_MEM_HOST
        )
        _native.check(self._lib, self._handle, rc, "bp_resample")
        return out

    def note_candidates(self, output: Dict[str, Any], prm) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], int]:
        """The dense half of note decoding on the device (`bp_note_candidates`, csrc/note_device.hip) for the posteriorgrams
        `output` (numpy arrays or CUDA tensors of T frames): (note map after constrain_frequency, onset-peak bitmap
        (T, 12) uint8, pitch-bend map (T, 88) int8 or None, status).  status 1: a NaN in the maps or an onset threshold
        <= 0 — decode the maps themselves (`note_creation.model_output_to_notes`).  `prm`: `note_creation._note_params`."""
        on_dev = _is_torch_cuda(output["note"])
        maps = {}
        for k, w in _MAPS:
            a = output[k]
            if on_dev:
                a = a.contiguous().float()
            else:
                a = np.require(a, np.float32, ["C"])
            if a.ndim != 2 or a.shape[1] != w:
                raise ValueError(f"{k}: expected (T, {w})")
            maps[k] = a
        T = int(maps["note"].shape[0])
        note = np.empty((T, N_FREQ_BINS_NOTES), np.float32)
        bits = np.empty((T, 12), np.uint8)
        bend = np.empty((T, N_FREQ_BINS_NOTES), np.int8) if prm.include_pitch_bends else None
        status = C.c_int(0)
        if on_dev:
            import torch

            torch.cuda.current_stream(maps["note"].device).synchronize()
        rc = self._lib.bp_note_candidates(
            self._handle, _ptr(maps["note"]), _ptr(maps["onset"]), _ptr(maps["contour"]), T, C.byref(prm),
            _mem_kind(maps["note"]), note.ctypes.data, bits.ctypes.data,
            bend.ctypes.data if bend is not None else None, C.byref(status),
        )
        _native.check(self._lib, self._handle, rc, "bp_note_candidates")
        return note, bits, bend, int(status.value)

    def predict_pcm(self, pcm: np.ndarray, sample_rate: int) -> Dict[str, np.ndarray]:
        """Decoded PCM at any rate / channel count -> un-overlapped posteriorgrams: downmix, resampling, windowing,
        CQT + CNN and un-overlapping all on the device (bp_infer_pcm)."""
        pcm = self._as_pcm(pcm)
        out = _empty_maps((self._pcm_frames(pcm.shape[0], sample_rate),))
        self._infer("bp_infer_pcm", (pcm.ctypes.data, pcm.shape[0], pcm.shape[1], int(sample_rate)), out)
        return out

    def predict_pcm_raw(self, samples, fmt: int, n_frames: int, channels: int, sample_rate: int) -> Dict[str, np.ndarray]:
        """predict_pcm on interleaved samples in the file's own format (`fmt` = a BP_PCM_* code; `samples` = any buffer
        of n_frames * channels of them): they cross PCIe as they are — 16-bit stereo is half the bytes of its float form
        — and become float on the device, bit-identical to converting on the host first (bp_infer_pcm_raw)."""
        buf = np.frombuffer(samples, dtype=np.uint8)
        width = _native.BP_PCM_WIDTH[int(fmt)]
        if buf.size < int(n_frames) * int(channels) * width:
            raise ValueError("predict_pcm_raw: the buffer is shorter than n_frames * channels samples")
        out = _empty_maps((self._pcm_frames(n_frames, sample_rate),))
        self._infer(
            "bp_infer_pcm_raw",
            (buf.ctypes.data if buf.size else None, int(fmt), int(n_frames), int(channels), int(sample_rate)), out,
        )
        return out

    def flac_layout(self, data: bytes) -> Dict[str, int]:
        """STREAMINFO of a FLAC file's bytes (host, no decoding): channels, sample_rate, bits_per_sample, block sizes,
        n_frames (0: not in the header)."""
        lay = _native.bp_flac_stream_layout()
        rc = self._lib.bp_flac_layout(data, len(data), C.byref(lay))
        if rc != _native.BP_OK:
            raise ValueError(f"bp_flac_layout: {self._lib.bp_audio_last_error().decode(errors='replace')}")
        return {k: int(getattr(lay, k)) for k, _ in lay._fields_}

    def flac_decode_device(self, data: bytes) -> Tuple[np.ndarray, int]:
        """A FLAC file's bytes decoded ON THE DEVICE (csrc/flac_device.hip): (int32 samples [n_frames, channels], sample
        rate) — the integers the host decoder's floats are made of.  ValueError if the stream cannot be decoded there
        (`NativeLibraryError` BP_ERR_UNSUPPORTED for what is left to the host decoder)."""
        lay = self.flac_layout(data)
        pcm = np.empty((max(0, lay["n_frames"]), lay["channels"]), dtype=np.int32)
        n = C.c_int64(0)
        rc = self._lib.bp_flac_decode_device(self._handle, data, len(data), pcm.ctypes.data if pcm.size else None, pcm.shape[0], C.byref(n))
        _native.check(self._lib, self._handle, rc, "bp_flac_decode_device")
        return pcm[: n.value], lay["sample_rate"]

    def adpcm_layout(self, data: bytes) -> Dict[str, int]:
        """The facts of an IMA ADPCM file's bytes from its headers (host, no decoding; include/basic_pitch_amd_adpcm.h):
        container, codec, channels, sample_rate, block_bytes, block_frames, n_frames, data_start, data_bytes.  ValueError for
        a file that is no such file or has a fault in its headers."""
        lay = _native.bp_adpcm_layout()
        rc = self._lib.bp_adpcm_layout_of(data, len(data), C.byref(lay))
        if rc != _native.BP_OK:
            raise ValueError(f"bp_adpcm_layout_of: {self._lib.bp_files_last_error().decode(errors='replace')}")
        return {k: int(getattr(lay, k)) for k, _ in lay._fields_}

    def adpcm_decode_device(self, data: bytes) -> Tuple[np.ndarray, int]:
        """An IMA ADPCM file's bytes decoded ON THE DEVICE (csrc/adpcm_device.hip): (int16 samples [n_frames, channels],
        sample rate), the samples of the host decoder `bp_adpcm_decode`."""
        lay = self.adpcm_layout(data)
        pcm = np.empty((lay["n_frames"], lay["channels"]), dtype=np.int16)
        n = C.c_int64(0)
        rc = self._lib.bp_adpcm_decode_device(self._handle, data, len(data), pcm.ctypes.data if pcm.size else None, pcm.shape[0], C.byref(n))
        _native.check(self._lib, self._handle, rc, "bp_adpcm_decode_device")
        return pcm[: n.value], lay["sample_rate"]

    def predict_adpcm(self, data: bytes) -> Dict[str, np.ndarray]:
        """The posteriorgrams of an IMA ADPCM file's bytes (RIFF/WAVE format tag 0x11, CAF ima4): the bytes cross PCIe as they
        are, a quarter of the PCM, one launch expands them on the device, then what predict_pcm_raw does (bp_infer_adpcm)."""
        lay = self.adpcm_layout(data)
        out = _empty_maps((self._pcm_frames(lay["n_frames"], lay["sample_rate"]),))
        self._infer("bp_infer_adpcm", (data, len(data)), out)
        return out

    def transcribe_adpcm_clips(
        self,
        blobs: Sequence[Any],
        onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
        frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
        minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
        minimum_frequency: Optional[float] = None,
        maximum_frequency: Optional[float] = None,
        multiple_pitch_bends: bool = False,
        melodia_trick: bool = True,
        midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
        threads: int = 8,
        decode: str = "device",
    ) -> "List[Any]":
        """Many short IMA ADPCM files (`bytes`-like) -> [(midi_data, note_events)] in input order, mirroring
        `transcribe_flac_clips`.  decode="device": the files of one codec, sample rate and channel count go to the device in
        ONE call and are expanded there by one launch (`bp_infer_adpcm_clips_events`); decode="host": the host decoder's
        samples take `transcribe_clips`.  The events of a clip are the same either way."""
        from . import adpcm_clips as _adpcm_clips

        return _adpcm_clips.transcribe_adpcm_clips(self, blobs, onset_threshold, frame_threshold, minimum_note_length,
                                                   minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick,
                                                   midi_tempo, threads, decode)

    def predict_flac(self, data: bytes) -> Dict[str, np.ndarray]:
        """The posteriorgrams of a FLAC file's bytes: decode on the device, then what predict_pcm_raw does (bp_infer_flac)."""
        lay = self.flac_layout(data)
        out = _empty_maps((self._pcm_frames(lay["n_frames"], lay["sample_rate"]),))
        self._infer("bp_infer_flac", (data, len(data)), out)
        return out

    # -- many clips in one call (basic_pitch_amd/clips.py) -----------------------------------------
    def transcribe_clips(
        self,
        clips: Sequence[Any],
        sample_rates: Union[int, Sequence[int]],
        onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
        frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
        minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
        minimum_frequency: Optional[float] = None,
        maximum_frequency: Optional[float] = None,
        multiple_pitch_bends: bool = False,
        melodia_trick: bool = True,
        midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
        threads: int = 8,
        decode: str = "host",
    ) -> "List[Tuple[Any, List[Any]]]":
        """Many short clips -> [(midi_data, note_events)] in input order, with the decoding parameters of `predict`.
        `clips`: numpy arrays [n] or [n, channels] of float32, int16, int32, uint8 or float64 samples (either byte order);
        `sample_rates`: one int for all or one per clip.  The clips of a rate go to the device in ONE call (`bp_infer_clips_candidates`: a constant
        number of launches per batch of windows instead of about ten per clip) and come back as what the sequential half of
        note decoding needs; the events of a clip are those of `predict_pcm_raw` + `model_output_to_notes` on it alone.
        decode="device": the sequential half runs on the device as well (`bp_infer_clips_events`, one workgroup per clip) and
        only events and bends come home; the same events."""
        from . import clips as _clips

        return _clips.transcribe_clips(self, clips, sample_rates, onset_threshold, frame_threshold, minimum_note_length,
                                       minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick, midi_tempo,
                                       threads, decode)

    def transcribe_flac_clips(
        self,
        blobs: Sequence[Any],
        onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
        frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
        minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
        minimum_frequency: Optional[float] = None,
        maximum_frequency: Optional[float] = None,
        multiple_pitch_bends: bool = False,
        melodia_trick: bool = True,
        midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
        threads: int = 8,
        decode: str = "host",
        errors: str = "raise",
    ) -> "List[Any]":
        """Many short FLAC files (`bytes`-like) -> [(midi_data, note_events)] in input order: `transcribe_clips` for clips
        that are still compressed.  The clips of a STREAMINFO rate go to the device in ONE call and are decoded there
        (`bp_infer_flac_clips_candidates`; decode="device": `bp_infer_flac_clips_events`); the events of a clip are those
        of `transcribe_clips` on the host decoder's samples.  A clip the device decoder leaves to the host or fails on is
        decoded by the host decoder and takes the PCM path.  A clip the host decoder cannot decode either raises ValueError
        with its index (errors="raise") or leaves that exception at its place in the list (errors="return")."""
        from . import flac_clips as _flac_clips

        return _flac_clips.transcribe_flac_clips(self, blobs, onset_threshold, frame_threshold, minimum_note_length,
                                                 minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick,
                                                 midi_tempo, threads, decode, errors)

    def note_events(self, outputs: Sequence[Dict[str, Any]], prm) -> "List[Tuple[Optional[List[Any]], int]]":
        """Note events of many posteriorgram segments in one call, decoded on the device (`bp_note_events_from_maps`,
        csrc/note_track.hip): `outputs` is a list of {"note", "onset", "contour"} dicts (numpy arrays or CUDA tensors), `prm`
        `note_creation._note_params`.  Returns [(events, status)] per dict: the events `model_output_to_notes` decodes from
        those maps, or None with status 1 (a NaN, or an onset threshold <= 0) or 2 (more events than the segment's region
        holds) — decode such maps on the host."""
        from . import events as _events

        return _events.note_events(self, outputs, prm)

    def sweep_note_events(self, outputs: Sequence[Dict[str, Any]], params: Sequence[Any],
                          pairs: "Optional[Sequence[Tuple[int, int]]]" = None):
        """The segments `outputs` (as for `note_events`) decoded under every parameter set of `params` (a list of
        `note_creation._note_params`) in ONE device call (`bp_note_events_sweep`): the maps go to the device once, the dense
        half runs once per distinct (frequency band, infer_onsets, onset threshold) among the sets, the tracker is one launch
        with a workgroup per decode.  Returns result[set][segment] = (events | None, status), each what `note_events` gives
        for that segment alone with that set; with `pairs`, a list of (segment, set), one such tuple per pair."""
        from . import sweep as _sweep

        return _sweep.sweep_note_events(self, outputs, params, pairs)

    def transcribe_clips_sweep(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Sequence[Any]
                               ) -> "List[List[List[Any]]]":
        """Many short clips (as for `transcribe_clips`) under every parameter set of `params` (a list of
        `note_creation._note_params`): result[set][clip] = note_events.  The clips of a rate go through the model ONCE
        (`bp_infer_clips_events_sweep`) whatever the number of sets; the events of a clip under a set are those of
        `transcribe_clips(..., decode="device")` with that set's parameters."""
        from . import sweep as _sweep

        return _sweep.transcribe_clips_sweep(self, clips, sample_rates, params)

    def sweep_note_scores(self, outputs: Sequence[Dict[str, Any]], params: Sequence[Any], refs: Sequence[Any],
                          pairs: "Optional[Sequence[Tuple[int, int]]]" = None, **tolerances: Any):
        """The segments `outputs` decoded under every set of `params` as by `sweep_note_events`, and every decode scored on
        the device against `refs` — per segment a sequence of (start_s, end_s, pitch_midi) or an (n, 3) array — in ONE call
        (`bp_note_events_sweep_score`): no event comes home, only the counts.  Returns a structured array with the fields
        n_ref, n_est, matched_onset, matched_offset, status, shaped (sets, segments), or (len(pairs),) with `pairs`;
        `score.precision_recall_f1` and `score.best_set` read it.  `tolerances`: the fields of `bp_score_params`
        (mir_eval's defaults).  A decode the device leaves (status != 0) is scored on the host; its status stays."""
        from . import score as _score

        return _score.sweep_note_scores(self, outputs, params, refs, pairs, **tolerances)

    def transcribe_clips_sweep_scores(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Sequence[Any],
                                      refs: Sequence[Any], pairs: "Optional[Sequence[Tuple[int, int]]]" = None, **tolerances: Any):
        """The same behind the model, for many short clips (as for `transcribe_clips_sweep`): the clips of a rate go through
        the model once (`bp_infer_clips_events_sweep_score`), and what comes home is the structured array of
        `sweep_note_scores`, a segment being a clip."""
        from . import score as _score

        return _score.transcribe_clips_sweep_scores(self, clips, sample_rates, params, refs, pairs, **tolerances)

    def sweep_frame_scores(self, outputs: Sequence[Dict[str, Any]], params: Sequence[Any], refs: Sequence[Any],
                           pairs: "Optional[Sequence[Tuple[int, int]]]" = None, notes: bool = True, **tolerances: Any):
        """`sweep_note_scores` with the frame level beside it, in ONE call (`bp_note_events_sweep_frame_score`): every decode is
        also scored frame by frame on the device (the restatement of mir_eval.multipitch in
        include/basic_pitch_amd_frame_score.h).  Returns (note counts, frame counts): the array of `sweep_note_scores` and one of
        the same shape with the fields n_frames, ref_frames, est_frames, true_pos, e_sub, status, which
        `frame_score.frame_metrics` and `frame_score.best_set_by_accuracy` read.  notes False: the note matching is skipped
        and the frame counts alone are returned.  A decode the device leaves (status != 0) is scored on the host; its status
        stays."""
        from . import frame_score as _frames

        return _frames.sweep_frame_scores(self, outputs, params, refs, pairs, notes, **tolerances)

    def transcribe_clips_sweep_frame_scores(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Sequence[Any],
                                            refs: Sequence[Any], pairs: "Optional[Sequence[Tuple[int, int]]]" = None,
                                            notes: bool = True, **tolerances: Any):
        """The same behind the model, for many short clips (as for `transcribe_clips_sweep_scores`): the clips of a rate go
        through the model once (`bp_infer_clips_events_sweep_frame_score`); returns as `sweep_frame_scores`, a segment being
        a clip."""
        from . import frame_score as _frames

        return _frames.transcribe_clips_sweep_frame_scores(self, clips, sample_rates, params, refs, pairs, notes, **tolerances)

    # -- multi-pitch estimates (basic_pitch_amd/multipitch.py) -------------------------------------
    def multipitch(self, outputs: Sequence[Any], params: Any = None) -> "List[Any]":
        """The multi-pitch estimate of every segment of `outputs` (the dicts `predict` / `run_inference` return, numpy arrays
        or CUDA tensors of one kind; their "contour" maps alone are read) in ONE call (`bp_multipitch_from_maps`): the f0 peaks
        of every contour row — at or above the threshold and above both neighbours, refined by a parabola —, picked and
        compacted on the device.  `params`: the fields of `bp_mp_params` (threshold 0.3, min_bin 1, max_bin 262 by default).
        Returns one `multipitch.MultiPitch` per segment: frames, times_s, pitch_midi, salience, freqs_hz, status."""
        from . import multipitch as _mp

        return _mp.multipitch(self, outputs, params)

    def transcribe_clips_multipitch(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None) -> "List[Any]":
        """The same behind the model, for many short clips (grouped by sample rate as `transcribe_clips` groups them): the
        clips of a rate go through the model once (`bp_infer_clips_multipitch`), and the points alone come home."""
        from . import multipitch as _mp

        return _mp.transcribe_clips_multipitch(self, clips, sample_rates, params)

    def sweep_multipitch_frame_scores(self, outputs: Sequence[Any], sets: Sequence[Any], refs: Sequence[Any],
                                      pairs: "Optional[Sequence[Tuple[int, int]]]" = None, **tolerances: Any):
        """Every segment of `outputs` under every set of `sets` (thresholds and bands: the fields of `bp_mp_params`), each
        decode scored frame by frame against `refs[segment]` ((start_s, end_s, pitch_midi) rows) on the device
        (`bp_multipitch_sweep_frame_score`): the structured array of `sweep_frame_scores`' frame level, shaped (sets,
        segments), or one record per pair of `pairs`.  A decode left for too many refs (status 3) is finished on the host; one
        with a NaN or an infinity in its rows (status 1) has no points and is reported as it is."""
        from . import multipitch as _mp

        return _mp.sweep_multipitch_frame_scores(self, outputs, sets, refs, pairs, **tolerances)

    def transcribe_clips_sweep_multipitch_frame_scores(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]],
                                                       sets: Sequence[Any], refs: Sequence[Any],
                                                       pairs: "Optional[Sequence[Tuple[int, int]]]" = None, **tolerances: Any):
        """The same behind the model (`bp_infer_clips_multipitch_sweep_frame_score`), a segment being a clip."""
        from . import multipitch as _mp

        return _mp.transcribe_clips_sweep_multipitch_frame_scores(self, clips, sample_rates, sets, refs, pairs, **tolerances)

    # -- the melody (basic_pitch_amd/melody.py) ----------------------------------------------------
    def melody(self, outputs: Sequence[Any], params: Any = None) -> "List[Any]":
        """The melody of every segment of `outputs` (the dicts `predict` / `run_inference` return, numpy arrays or CUDA
        tensors of one kind; their "contour" maps alone are read) in ONE call (`bp_melody_from_maps`): one f0 track with
        voiced / unvoiced decisions per segment, the best path of a Viterbi recurrence over its frames, decoded on the device
        with a workgroup per segment.  `params`: the fields of `bp_melody_params` (threshold 0.3, jump_penalty 0.05,
        voicing_penalty 0.5, max_jump 4, bins 0 ... 263 by default).  Returns one `melody.Melody` per segment: bins, times_s,
        pitch_midi, salience, freqs_hz, voiced, status."""
        from . import melody as _mel

        return _mel.melody(self, outputs, params)

    def transcribe_clips_melody(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None) -> "List[Any]":
        """The same behind the model, for many short clips (grouped by sample rate as `transcribe_clips` groups them): the
        clips of a rate go through the model once (`bp_infer_clips_melody`), and a 16-byte record per row comes home."""
        from . import melody as _mel

        return _mel.transcribe_clips_melody(self, clips, sample_rates, params)

    def sweep_melody_scores(self, outputs: Sequence[Any], sets: Sequence[Any], ref_tracks: Sequence[Any],
                            pairs: "Optional[Sequence[Tuple[int, int]]]" = None, **tolerances: Any):
        """Every segment of `outputs` under every set of `sets` (the fields of `bp_melody_params`), each decode scored on the
        device against `ref_tracks[segment]` (a MIDI pitch per row, 0.0 unvoiced: `melody.ref_track` makes one from an
        annotation) by the melody measures' counts (`bp_melody_sweep_score`): a structured array of `melody.MELODY_COUNTS`
        shaped (sets, segments), or one record per pair of `pairs`; `melody.measures` forms the ratios.  A decode with a NaN
        or a magnitude above 65536 in its rows (status 1) is all unvoiced and reported as it is."""
        from . import melody as _mel

        return _mel.sweep_melody_scores(self, outputs, sets, ref_tracks, pairs, **tolerances)

    def transcribe_clips_sweep_melody_scores(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], sets: Sequence[Any],
                                             ref_tracks: Sequence[Any], pairs: "Optional[Sequence[Tuple[int, int]]]" = None,
                                             **tolerances: Any):
        """The same behind the model (`bp_infer_clips_melody_sweep_score`), a segment being a clip."""
        from . import melody as _mel

        return _mel.transcribe_clips_sweep_melody_scores(self, clips, sample_rates, sets, ref_tracks, pairs, **tolerances)

    # -- forced alignment (basic_pitch_amd/align.py) -----------------------------------------------
    def align(self, outputs: Sequence[Any], ref_notes: Sequence[Any], **params: Any) -> "List[Any]":
        """Reference notes that are not on the audio's time base aligned to every segment of `outputs` (the dicts `predict` /
        `run_inference` return, numpy arrays or CUDA tensors of one kind; their "note" and "onset" maps are read) in ONE call
        (`bp_align_from_maps`): `ref_notes[i]` rows of (start_s, end_s, pitch_midi) become states in order
        (`align.states_from_notes`; `lead`, `tail`, `max_shift_s` go there), a monotone dynamic programme on the device finds
        every state's first frame (`threshold_q` 307, `onset_weight` 2 by default), and the notes come back on the audio's
        frames.  Returns one `align.Alignment` per segment: notes, first_frame, total, status."""
        from . import align as _al

        return _al.align(self, outputs, ref_notes, **params)

    def transcribe_clips_align(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], ref_notes: Sequence[Any],
                               **params: Any) -> "List[Any]":
        """The same behind the model, for many short clips (grouped by sample rate as `transcribe_clips` groups them): the
        clips of a rate go through the model once (`bp_infer_clips_align`), and 4 bytes per state come home."""
        from . import align as _al

        return _al.transcribe_clips_align(self, clips, sample_rates, ref_notes, **params)

    # -- tempo and beats (basic_pitch_amd/beat.py) -------------------------------------------------
    def beats(self, outputs: Sequence[Any], params: Any = None) -> "List[Any]":
        """Tempo and beats of every segment of `outputs` (the dicts `predict` / `run_inference` return, numpy arrays or CUDA
        tensors of one kind; their "onset" maps alone are read) in ONE call (`bp_beats_from_maps`): one period per segment by
        autocorrelation under a tempo prior, then the beat frames by a dynamic programme, in exact integers on the device.
        `params`: the fields of `bp_beat_params` (threshold_q 307, lags 21 ... 172, tightness 4 by default; `start_bpm` /
        `sd_octaves` make the prior).  Returns one `beat.Beats` per segment: frames, times_s, period_frames, bpm, status; the
        bpm goes into the `midi_tempo` arguments as it is."""
        from . import beat as _bt

        return _bt.beats(self, outputs, params)

    def transcribe_clips_beats(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None) -> "List[Any]":
        """The same behind the model, a segment being a clip ([n_frames, channels] arrays, each with its sample rate): the
        clips of a rate go through the model once (`bp_infer_clips_beats`), and 32 bytes per clip and 4 per beat come home."""
        from . import beat as _bt

        return _bt.transcribe_clips_beats(self, clips, sample_rates, params)

    # -- chords and key (basic_pitch_amd/chord.py) -------------------------------------------------
    def chords(self, outputs: Sequence[Any], params: Any = None, beats: Any = None) -> "List[Any]":
        """Chords and key of every segment of `outputs` (the dicts `predict` / `run_inference` return, numpy arrays or CUDA
        tensors of one kind; their "note" maps alone are read) in ONE call (`bp_chords_from_maps`): a chroma per row, a Viterbi
        path over a table of chord templates with a switching penalty, a key by profile correlation, in exact integers on the
        device.  `params`: the fields of `bp_chord_params` (threshold_q 307, switch_penalty 128 by default) and `vocabulary`
        ("majmin", "triads", "sevenths").  `beats`: the list `Model.beats` returns (or one array of frames per segment): the
        units are the stretches between beats instead of frames.  Returns one `chord.Chords` per segment: labels, runs,
        times_s, key, status."""
        from . import chord as _ch

        return _ch.chords(self, outputs, params, beats)

    def transcribe_clips_chords(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], params: Any = None,
                                bounds: Any = None) -> "List[Any]":
        """The same behind the model, a segment being a clip ([n_frames, channels] arrays, each with its sample rate): the
        clips of a rate go through the model once (`bp_infer_clips_chords`), and 32 bytes per clip and a byte per row come
        home.  `bounds`: per clip the boundary frames (or a `beat.Beats`), or None for frame units."""
        from . import chord as _ch

        return _ch.transcribe_clips_chords(self, clips, sample_rates, params, bounds)

    # -- two recordings against each other (basic_pitch_amd/sync.py) -------------------------------
    def sync(self, outputs_a: Sequence[Any], outputs_b: Sequence[Any], **params: Any) -> "List[Any]":
        """The i-th of `outputs_a` synchronised with the i-th of `outputs_b` (the dicts `predict` / `run_inference` return,
        numpy arrays or CUDA tensors of one kind; their "note" maps alone are read) in ONE call (`bp_sync_from_maps`): a chroma
        per row pooled over units of `hop` frames, one feature byte a class, and the best monotone path over the units of both
        by a dynamic time warp in exact integers on the device.  `params`: the fields of `bp_sync_params` (threshold_q 307,
        hop 4, band 0 by default).  Returns one `sync.Sync` per pair: status, total, path, and `map_times` / `transfer_notes`
        to move times and notes from one recording's time base to the other's."""
        from . import sync as _sy

        return _sy.sync(self, outputs_a, outputs_b, **params)

    def sync_pairs(self, outputs: Sequence[Any], pairs: Sequence[Any], **params: Any) -> "List[Any]":
        """The same for a table of (a, b) indices into `outputs`: one against many, or a segment against itself."""
        from . import sync as _sy

        return _sy.sync_pairs(self, outputs, pairs, **params)

    def transcribe_clips_sync(self, clips: Sequence[Any], sample_rates: Union[int, Sequence[int]], pairs: Sequence[Any],
                              **params: Any) -> "List[Any]":
        """The same behind the model, a segment being a clip ([n_frames, channels] arrays, each with its sample rate): the
        clips of a rate go through the model once (`bp_infer_clips_sync`), and 32 bytes per pair and 8 per path entry come
        home.  A pair whose clips differ in sample rate is a ValueError: use `sync` on `predict_pcm` outputs."""
        from . import sync as _sy

        return _sy.transcribe_clips_sync(self, clips, sample_rates, pairs, **params)

    # -- streaming (basic_pitch_amd/streaming.py) --------------------------------------------------
    def open_stream(self, sample_rate: int, channels: int = 1, fmt: int = _native.BP_PCM_F32):
        """A streaming session on this model for interleaved PCM of `fmt` (a BP_PCM_* code) at `sample_rate`:
        `Stream.push(chunk)` returns the posteriorgram rows that became final, `Stream.finish()` the rest; concatenated
        they are bit for bit `predict_pcm_raw` of the whole input (bp_stream_*)."""
        from .streaming import Stream

        return Stream(self, sample_rate, channels, fmt)

    def push_streams(self, streams, chunks) -> "List[Dict[str, np.ndarray]]":
        """One step for several of this model's streams: `chunks[i]` goes to `streams[i]`, the newly complete windows of
        all of them run in full batches (bp_streams_push).  Each stream's new rows, as `Stream.push` would return them."""
        from .streaming import push_streams

        return push_streams(self, streams, chunks)

    def peek_streams(self, streams) -> "List[Dict[str, np.ndarray]]":
        """`Stream.peek` for several of this model's streams in one step: the rows a finish would emit now for each of
        them, nothing committed, their tail windows in full batches (bp_streams_peek)."""
        from .streaming import peek_streams

        return peek_streams(self, streams)

    def transcripts(self, transcribers, workers=None, decode="host", midi=True):
        """`transcript()` of many live `StreamingTranscriber`s of this model behind one device step
        (`streaming.transcripts`, `bp_streams_candidates`): `(midi_data, note_events)` per transcriber, in order.
        `decode="device"` decodes the events on the device too (`bp_streams_events`); `midi=False` returns `(None, note_events)`."""
        from .streaming import transcripts

        return transcripts(self, transcribers, workers, decode, midi)

    # -- introspection ----------------------------------------------------------------------------
    def info(self) -> Dict[str, Any]:
        inf = _native.bp_info()
        _native.check(self._lib, self._handle, self._lib.bp_get_info(self._handle, C.byref(inf)), "bp_get_info")
        return {
            "device": inf.device_ordinal,
            "compute_units": inf.compute_units,
            "max_windows": inf.max_windows,
            "workspace_bytes": inf.workspace_bytes,
            "arch": inf.arch.decode(),
        }

    def stage_ms(self) -> Dict[str, float]:
        ms = (C.c_float * _native.BP_N_STAGES)()
        _native.check(self._lib, self._handle, self._lib.bp_get_stage_ms(self._handle, ms, _native.BP_N_STAGES), "bp_get_stage_ms")
        return {k: float(v) for k, v in zip(_native.STAGE_NAMES, ms)}


def window_audio_file(
    audio_original: np.ndarray, hop_size: int
) -> Iterable[Tuple[np.ndarray, Dict[str, float]]]:
    """Pad and window an audio signal into AUDIO_N_SAMPLES chunks (inference.py:194-219)."""
    for i in range(0, audio_original.shape[0], hop_size):
        window = audio_original[i : i + AUDIO_N_SAMPLES]
        if len(window) < AUDIO_N_SAMPLES:
            window = np.pad(window, pad_width=[[0, AUDIO_N_SAMPLES - len(window)]])
        t_start = float(i) / AUDIO_SAMPLE_RATE
        window_time = {"start": t_start, "end": t_start + (AUDIO_N_SAMPLES / AUDIO_SAMPLE_RATE)}
        yield np.expand_dims(window, axis=-1), window_time


def get_audio_input(
    audio_path: Union[pathlib.Path, str], overlap_len: int, hop_size: int
) -> Iterable[Tuple[np.ndarray, Dict[str, float], int]]:
    """Read a file as mono 22.05 kHz, prepend overlap_len/2 zeros, yield windows (inference.py:222-244)."""
    assert overlap_len % 2 == 0, f"overlap_length must be even, got {overlap_len}"
    audio_original, _ = _audio.load(str(audio_path), sr=AUDIO_SAMPLE_RATE, mono=True)
    original_length = audio_original.shape[0]
    audio_original = np.concatenate([np.zeros((int(overlap_len / 2),), dtype=np.float32), audio_original])
    for window, window_time in window_audio_file(audio_original, hop_size):
        yield np.expand_dims(window, axis=0), window_time, original_length


def unwrap_output(
    output: np.ndarray, audio_original_length: int, n_overlapping_frames: int, hop_size: int
) -> Optional[np.ndarray]:
    """Unwrap batched model predictions to a single matrix (inference.py:247-279)."""
    if len(output.shape) != 3:
        return None
    n_olap = int(0.5 * n_overlapping_frames)
    if n_olap > 0:
        output = output[:, n_olap:-n_olap, :]
    output_shape = output.shape
    unwrapped_output = output.reshape(output_shape[0] * output_shape[1], output_shape[2])
    n_expected_windows = audio_original_length / hop_size
    n_frames_per_window = (AUDIO_WINDOW_LENGTH * ANNOTATIONS_FPS) - n_overlapping_frames
    return unwrapped_output[: int(n_expected_windows * n_frames_per_window), :]


# `predict(path)` with a model PATH loads the model on every call in the reference (inference.py:291-292 -> Model(...)).
# Loading is 60 ms here (parsing, packing the operand fragments, 0.8 GB of device buffers) against ~1 ms for the
# reference's 10-second clip itself, so a loaded model is kept and reused — PER THREAD (the handle is stateful and not for
# two threads at once) and in thread-local storage, so that the models of a thread are released when the thread ends
# (a process-wide table keyed by thread id kept up to 8 x 0.8 GB alive for threads long gone).  At most
# _MODEL_CACHE_MAX models per thread, oldest evicted first; clear_model_cache() drops the calling thread's.
_MODEL_CACHE_MAX = 2


class _ThreadModels(threading.local):
    def __init__(self) -> None:
        self.models: "Dict[Tuple[Any, ...], Model]" = {}


_MODEL_CACHE = _ThreadModels()


def clear_model_cache() -> None:
    """Forget the models `predict(path)` / `run_inference(path)` keep loaded for the calling thread (their device
    buffers are freed when nobody else holds the Model)."""
    _MODEL_CACHE.models.clear()


def _model_from(model_or_model_path) -> Any:
    """A Model (or anything shaped like one) as it is; a path as the calling thread's cached Model loaded from that file."""
    if not isinstance(model_or_model_path, (str, os.PathLike)):
        return model_or_model_path
    try:
        real = os.path.realpath(os.fspath(model_or_model_path))
        st = os.stat(real)
        key = (real, st.st_mtime_ns, st.st_size)
    except OSError:
        return Model(model_or_model_path)  # raises what loading a missing file raises
    models = _MODEL_CACHE.models
    model = models.get(key)
    if model is not None and model._handle.value:
        return model
    model = Model(model_or_model_path)
    while len(models) >= _MODEL_CACHE_MAX:
        models.pop(next(iter(models)))  # oldest first; the handle is freed when nobody holds the Model
    models[key] = model
    return model


def run_inference(
    audio_path: Union[pathlib.Path, str],
    model_or_model_path: Union[Model, pathlib.Path, str] = ICASSP_2022_MODEL_PATH,
    debug_file: Optional[pathlib.Path] = None,
) -> Dict[str, np.ndarray]:
    """Run the model on the input audio path (inference.py:282-330).

    Returns {"note": (T,88), "onset": (T,88), "contour": (T,264)} float32, T = int(L/36164*142).
    """
    model = _model_from(model_or_model_path)

    def host_decoded():
        pcm, sr = _audio.read_audio(str(audio_path))
        return model.predict_pcm(pcm, sr), pcm.shape[0], sr

    # decode on the host (container parsing), everything after it on the device: channel-mean downmix, resampling
    # to 22.05 kHz, the 3840-sample lead-in + windowing, CQT + CNN, un-overlapping (inference.py:239-244, 302-315)
    with open(audio_path, "rb") as f:
        head = f.read(12)
    adpcm = False
    if (head[:4] in (b"RIFF", b"RF64", b"BW64", b"caff")) and hasattr(model, "predict_adpcm"):
        adpcm = _audio.is_adpcm_file(str(audio_path))  # from the format chunk alone
    if adpcm:
        # an IMA ADPCM file's BYTES go to the device and are expanded there (csrc/adpcm_device.hip): a quarter of the PCIe bytes
        # of the PCM and no host core-time per sample; where the library refuses, the numpy reader decodes the file here
        with open(audio_path, "rb") as f:
            blob = f.read()
        try:
            lay = model.adpcm_layout(blob)
            unwrapped_output, n_file_frames, file_sr = model.predict_adpcm(blob), lay["n_frames"], lay["sample_rate"]
        except (ValueError, _native.NativeLibraryError):  # (a fault in the headers: the reader names it with the path)
            unwrapped_output, n_file_frames, file_sr = host_decoded()
    elif head[:4] == b"RIFF" and head[8:12] == b"WAVE" and hasattr(model, "predict_pcm_raw"):
        # a WAV file's samples go to the device in the file's own format (no float copy on the host, half the PCIe bytes
        # for 16-bit audio); same posteriorgrams, bit for bit, as decoding them here
        raw, tag, bits, channels, file_sr = _audio.wav_raw(str(audio_path))
        n_file_frames = len(raw) // (bits // 8) // channels
        unwrapped_output = model.predict_pcm_raw(raw, _WAV_PCM[(tag, bits)], n_file_frames, channels, file_sr)
    elif ((head[:4] in (b"RF64", b"BW64") and head[8:12] == b"WAVE") or (head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC"))
          or head[:4] in (b"caff", b".snd")) and hasattr(model, "predict_pcm_raw"):
        # RF64 / BW64, AIFF / AIFF-C, CAF, AU: the same, in whichever of the fourteen sample formats the file holds (big-endian
        # words, signed bytes, G.711: converted on the device like the WAV formats)
        raw, fmt, channels, file_sr, n_file_frames = _audio.pcm_raw(str(audio_path))
        unwrapped_output = model.predict_pcm_raw(raw, fmt, n_file_frames, channels, file_sr)
    elif head[:4] == b"fLaC" and hasattr(model, "predict_flac"):
        # a FLAC file's BYTES go to the device and are decoded there (csrc/flac_device.hip): half the PCIe bytes of the PCM and
        # no host core-time per sample; what the device decoder leaves to the host (or cannot follow) is decoded here as
        # before — the host decoder also names the fault of a corrupt file
        with open(audio_path, "rb") as f:
            blob = f.read()
        try:
            lay = model.flac_layout(blob)
            if lay["n_frames"] <= 0:
                raise _native.NativeLibraryError("no sample count in STREAMINFO")
            unwrapped_output, n_file_frames, file_sr = model.predict_flac(blob), lay["n_frames"], lay["sample_rate"]
        except (ValueError, _native.NativeLibraryError):
            unwrapped_output, n_file_frames, file_sr = host_decoded()
    else:
        unwrapped_output, n_file_frames, file_sr = host_decoded()
    audio_original_length = int(-(-n_file_frames * AUDIO_SAMPLE_RATE // file_sr))  # librosa.resample: ceil(n * sr / file_sr)

    if debug_file:
        with open(debug_file, "w") as f:
            json.dump(
                {
                    "audio_original_length": audio_original_length,
                    "hop_size_samples": _HOP_SIZE,
                    "overlap_length_samples": _OVERLAP_LEN,
                    "unwrapped_output": {k: v.tolist() for k, v in unwrapped_output.items()},
                },
                f,
            )
    return unwrapped_output


def run_inference_windowed(
    audio_path: Union[pathlib.Path, str], model: Model, batch: int = 64
) -> Dict[str, np.ndarray]:
    """The reference's own structure (host windowing -> Model.predict -> host unwrap), batched.

    Used by the tests to show that the on-device track path equals the per-window path.
    """
    windows: List[np.ndarray] = []
    audio_original_length = 0
    for audio_windowed, _, audio_original_length in get_audio_input(audio_path, _OVERLAP_LEN, _HOP_SIZE):
        windows.append(audio_windowed[0])
    output: Dict[str, List[np.ndarray]] = {"note": [], "onset": [], "contour": []}
    for i in range(0, len(windows), batch):
        for k, v in model.predict(np.stack(windows[i : i + batch])).items():
            output[k].append(v)
    return {
        k: unwrap_output(np.concatenate(output[k]), audio_original_length, DEFAULT_OVERLAPPING_FRAMES, _HOP_SIZE)
        for k in output
    }


def _window_geometry(model: Any) -> Tuple[int, int, int]:
    """(window length, hop, lead-in) in samples at the model's own rate: the reference's 43844 / 36164 / 3840 at 22.05 kHz,
    hop and lead-in scaled by rate / 22050 for a model of another geometry (`Model(ext_cqt_44k=True)`: 87688 / 72328 / 7680
    at 44.1 kHz).  A model-shaped object without `sample_rate` and `audio_n_samples` has the reference's."""
    rate, win = getattr(model, "sample_rate", None), getattr(model, "audio_n_samples", None)
    if rate is None or win is None:
        return AUDIO_N_SAMPLES, _HOP_SIZE, _OVERLAP_LEN // 2
    return int(win), _HOP_SIZE * int(rate) // AUDIO_SAMPLE_RATE, (_OVERLAP_LEN // 2) * int(rate) // AUDIO_SAMPLE_RATE


def predict_window_range(
    audio_path: Union[pathlib.Path, str],
    model_or_model_path: Union[Model, pathlib.Path, str],
    piece: int,
    n_pieces: int,
) -> Dict[str, Any]:
    """Piece `piece` of `n_pieces` of ONE long file (the window-range fallback of the file-sharded job).

    A window's samples are determined by its index alone (start = w * 36164 - 3840: inference.py:207,242; w * hop - lead-in of
    the model's own geometry, `_window_geometry`) and a window's 142
    un-overlapped rows by the window alone (per-window normalisation, signal.py:177-183), so a rank can compute windows
    [w0, w1) = `sharding.split_windows(n_windows, n_pieces)[piece]` without any of its neighbours' data: the file is decoded
    and resampled (on the device, by the same kernel the whole-file call uses), this range's windows are cut on the host
    exactly as `window_audio_file` cuts them and go through `Model.predict` in full batches; `assemble_window_ranges`
    concatenates the pieces' rows — the same bits the unsplit call produces (the library's results do not depend on how
    windows are batched: tests/test_gpu_parity.py::test_batch_invariance_and_chunking)."""
    from .sharding import split_windows

    model = _model_from(model_or_model_path)
    verify_input_path(audio_path)
    pcm, file_sr = _audio.read_audio(str(audio_path))
    y = np.ascontiguousarray(model.resample(pcm, file_sr), dtype=np.float32)
    n_olap = DEFAULT_OVERLAPPING_FRAMES // 2
    win, hop, lead = _window_geometry(model)
    padded = np.concatenate([np.zeros((lead,), dtype=np.float32), y])
    n_windows = len(range(0, padded.shape[0], hop))
    w0, w1 = split_windows(n_windows, n_pieces)[piece]
    rows: Dict[str, List[np.ndarray]] = {k: [] for k, _ in _MAPS}
    batch = int(getattr(model, "max_windows", 256))
    for a in range(w0, w1, batch):
        b = min(w1, a + batch)
        x = np.zeros((b - a, win), dtype=np.float32)
        for w in range(a, b):
            seg = padded[w * hop : w * hop + win]
            x[w - a, : len(seg)] = seg
        for k, v in model.predict(x).items():
            if k in rows:
                v = np.asarray(v)[:, n_olap:-n_olap, :]
                rows[k].append(v.reshape(v.shape[0] * v.shape[1], v.shape[2]))
    return {"rows": {k: (np.concatenate(rows[k]) if rows[k] else np.zeros((0, w), np.float32)) for k, w in _MAPS},
            "range": (w0, w1), "n_windows": n_windows, "original_length": int(y.shape[0]), "hop": hop}


def _min_note_len_frames(minimum_note_length: float) -> int:
    """A note length in milliseconds as a number of model frames (inference.py:469)."""
    return int(np.round(minimum_note_length / 1000 * (AUDIO_SAMPLE_RATE / FFT_HOP)))


def _output_to_notes(
    model_output: Dict[str, np.ndarray], onset_threshold: float, frame_threshold: float, minimum_note_length: float,
    minimum_frequency: Optional[float], maximum_frequency: Optional[float], multiple_pitch_bends: bool, melodia_trick: bool,
    midi_tempo: float,
) -> Tuple["infer.pretty_midi.PrettyMIDI", List["infer.NoteEvent"]]:
    """`note_creation.model_output_to_notes` from the arguments `predict` takes (inference.py:470-480): (midi_data, note_events)."""
    return infer.model_output_to_notes(
        model_output, onset_thresh=onset_threshold, frame_thresh=frame_threshold,
        min_note_len=_min_note_len_frames(minimum_note_length), min_freq=minimum_frequency, max_freq=maximum_frequency,
        multiple_pitch_bends=multiple_pitch_bends, melodia_trick=melodia_trick, midi_tempo=midi_tempo,
    )


def _output_stem(audio_path: Union[pathlib.Path, str]) -> str:
    """The `<stem>` of a file's outputs `<stem>_basic_pitch.<ext>` (inference.py:395)."""
    return os.path.splitext(os.path.basename(str(audio_path)))[0]


def assemble_window_ranges(
    parts: Sequence[Dict[str, Any]],
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
    **_ignored: Any,
) -> Tuple[Dict[str, np.ndarray], "infer.pretty_midi.PrettyMIDI", List["infer.NoteEvent"]]:
    """The pieces of `predict_window_range` back into what `predict()` returns for the file: rows concatenated in window
    order, trimmed to int(L / hop * 142) (`unwrap_output`, inference.py:277-279), notes decoded over the WHOLE file (a note
    may span pieces)."""
    parts = sorted(parts, key=lambda p: p["range"][0])
    at = 0
    for p in parts:
        if p["range"][0] != at:
            raise ValueError(f"window ranges do not tile the file: expected a piece starting at window {at}, got {p['range']}")
        at = p["range"][1]
    if not parts or at != parts[0]["n_windows"]:
        raise ValueError("window ranges do not cover the file")
    n_rows = int(parts[0]["original_length"] / parts[0].get("hop", _HOP_SIZE) * (AUDIO_WINDOW_LENGTH * ANNOTATIONS_FPS - DEFAULT_OVERLAPPING_FRAMES))
    model_output = {k: np.ascontiguousarray(np.concatenate([p["rows"][k] for p in parts])[:n_rows]) for k, _ in _MAPS}
    return (model_output,) + _output_to_notes(
        model_output, onset_threshold, frame_threshold, minimum_note_length, minimum_frequency, maximum_frequency,
        multiple_pitch_bends, melodia_trick, midi_tempo,
    )


class OutputExtensions(enum.Enum):
    MIDI = "mid"
    MODEL_OUTPUT_NPZ = "npz"
    MIDI_SONIFICATION = "wav"
    NOTE_EVENTS = "csv"


def verify_input_path(audio_path: Union[pathlib.Path, str]) -> None:
    """inference.py:340-354."""
    if not os.path.isfile(audio_path):
        raise ValueError(f"{audio_path} is not a file path.")


def verify_output_dir(output_dir: Union[pathlib.Path, str]) -> None:
    """inference.py:357-371."""
    if not os.path.isdir(output_dir):
        raise ValueError(f"{output_dir} is not a directory.")


def build_output_path(
    audio_path: Union[pathlib.Path, str], output_directory: Union[pathlib.Path, str], output_type: OutputExtensions
) -> pathlib.Path:
    """inference.py:374-406: <dir>/<stem>_basic_pitch.<ext>; IOError if it already exists."""
    output_path = pathlib.Path(output_directory) / f"{_output_stem(audio_path)}_basic_pitch.{output_type.value}"
    if output_path.exists():
        raise IOError(f"{output_path} already exists and would be overwritten. Skipping output files for {audio_path}.")
    return output_path


def save_note_events(note_events: List["infer.NoteEvent"], save_path: Union[pathlib.Path, str]) -> None:
    """inference.py:409-428: CSV with start_time_s, end_time_s, pitch_midi, velocity, pitch_bend..."""
    with open(save_path, "w") as fhandle:
        writer = csv.writer(fhandle, delimiter=",")
        writer.writerow(["start_time_s", "end_time_s", "pitch_midi", "velocity", "pitch_bend"])
        for start_time, end_time, note_number, amplitude, pitch_bend in note_events:
            row = [start_time, end_time, note_number, int(np.round(DEFAULT_MIDI_VELOCITY_SCALE * amplitude))]
            if pitch_bend:
                row.extend(pitch_bend)
            writer.writerow(row)


def predict(
    audio_path: Union[pathlib.Path, str],
    model_or_model_path: Union[Model, pathlib.Path, str] = ICASSP_2022_MODEL_PATH,
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    debug_file: Optional[pathlib.Path] = None,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
) -> Tuple[Dict[str, np.ndarray], "infer.pretty_midi.PrettyMIDI", List["infer.NoteEvent"]]:
    """Run a single prediction (inference.py:431-506): (model_output, midi_data, note_events)."""
    model_output = run_inference(audio_path, model_or_model_path, debug_file)
    midi_data, note_events = _output_to_notes(
        model_output, onset_threshold, frame_threshold, minimum_note_length, minimum_frequency, maximum_frequency,
        multiple_pitch_bends, melodia_trick, midi_tempo,
    )
    if debug_file:
        with open(debug_file) as f:
            debug_data = json.load(f)
        with open(debug_file, "w") as f:
            json.dump(
                {
                    **debug_data,
                    "min_note_length": _min_note_len_frames(minimum_note_length),
                    "onset_thresh": onset_threshold,
                    "frame_thresh": frame_threshold,
                    "estimated_notes": [
                        (float(s0), float(s1), int(pitch), float(amp), [int(b) for b in pb] if pb else None)
                        for s0, s1, pitch, amp, pb in note_events
                    ],
                },
                f,
            )
    return model_output, midi_data, note_events


def predict_many(
    audio_paths: Sequence[Union[pathlib.Path, str]],
    model_or_model_path: Union[Model, pathlib.Path, str] = ICASSP_2022_MODEL_PATH,
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
    group: int = 64,
    decode_threads: Optional[int] = None,
    return_exceptions: bool = False,
    _finish: Optional[Any] = None,
) -> List[Tuple[Dict[str, np.ndarray], "infer.pretty_midi.PrettyMIDI", List["infer.NoteEvent"]]]:
    """predict() (inference.py:431-506) over many files, results in input order and identical to per-file predict().

    The reference runs one file after the other and one window per runtime call.  Here the files of a group are
    decoded on a host thread pool (file read + container parsing; the device does downmix and resampling:
    bp_resample), their windows packed across file boundaries into full batches (bp_infer_tracks), and the note
    decoding of a finished group (host C++, GIL released) runs on the same pool while the GPU works on the next
    group: one GPU produces posteriorgrams ~200 x faster than one host core decodes them.

    `return_exceptions=True` isolates failures per file like the reference's per-file try / except
    (inference.py:548-604): the entry of a file that cannot be read or decoded is the exception instead of a tuple.

    `_finish(index, result)` (internal; `predict_and_save_many`) runs on the pool right behind a file's note decoding and
    its return value replaces the file's entry — the writers of a batch job, so that ONE pipeline runs over all files
    (next group read while this one is on the GPU, decoding and writing of finished files behind it) and a file's
    posteriorgrams are dropped as soon as they are written.  The GPU is kept at most two groups ahead of the decoders.
    """
    import concurrent.futures as cf

    # a path loads the model like the reference does (once per thread: _model_from); a Model — or anything with its
    # resample / predict_tracks — is used
    model = _model_from(model_or_model_path)
    if group < 1:
        raise ValueError("group must be >= 1")
    paths = [pathlib.Path(p) for p in audio_paths]
    if not return_exceptions:
        for p in paths:
            verify_input_path(p)

    def decode_and_finish(i: int, model_output: Dict[str, np.ndarray]):
        res = (model_output,) + _output_to_notes(
            model_output, onset_threshold, frame_threshold, minimum_note_length, minimum_frequency, maximum_frequency,
            multiple_pitch_bends, melodia_trick, midi_tempo,
        )
        return res if _finish is None else _finish(i, res)

    def read(p: pathlib.Path):
        verify_input_path(p)
        return _audio.read_audio(str(p))

    workers = decode_threads if decode_threads else min(16, os.cpu_count() or 1)
    results: List[Any] = [None] * len(paths)
    with cf.ThreadPoolExecutor(max_workers=workers) as pool:
        groups = [list(range(g0, min(g0 + group, len(paths)))) for g0 in range(0, len(paths), group)]
        pending = [pool.submit(read, paths[i]) for i in groups[0]] if groups else []
        for gi, ids in enumerate(groups):
            reads, pending = pending, []
            if gi + 1 < len(groups):  # the next group's files are read while this one is on the GPU
                pending = [pool.submit(read, paths[i]) for i in groups[gi + 1]]
            signals, good = [], []
            for i, fut in zip(ids, reads):
                try:
                    pcm, sr = fut.result()
                    signals.append(model.resample(pcm, sr))  # downmix + resampling on the device
                    good.append(i)
                except Exception as e:
                    if not return_exceptions:
                        raise
                    results[i] = e
            if _finish is not None and gi >= 2:  # back-pressure: posteriorgrams of at most two groups await decoding
                for i in groups[gi - 2]:
                    if isinstance(results[i], cf.Future):
                        cf.wait([results[i]])
            for i, out in zip(good, model.predict_tracks(signals)):
                results[i] = pool.submit(decode_and_finish, i, out)
        for i, r in enumerate(results):
            if isinstance(r, cf.Future):
                try:
                    results[i] = r.result()
                except Exception as e:
                    if not return_exceptions:
                        raise
                    results[i] = e
    return results


def _save_outputs(audio_path, output_directory, result, save_midi: bool, sonify_midi: bool, save_model_outputs: bool,
                  save_notes: bool, sonification_samplerate: int) -> Dict[str, str]:
    """The four writers of inference.py:565-602 for one file's `(model_output, midi_data, note_events)`; returns the paths."""
    model_output, midi_data, note_events = result
    written: Dict[str, str] = {}
    if save_model_outputs:
        path = build_output_path(audio_path, output_directory, OutputExtensions.MODEL_OUTPUT_NPZ)
        np.savez(path, basic_pitch_model_output=model_output)
        written["model_output"] = str(path)
    if save_midi:
        path = build_output_path(audio_path, output_directory, OutputExtensions.MIDI)
        midi_data.write(str(path))
        written["midi"] = str(path)
    if sonify_midi:
        path = build_output_path(audio_path, output_directory, OutputExtensions.MIDI_SONIFICATION)
        infer.sonify_midi(midi_data, path, sr=sonification_samplerate)
        written["sonification"] = str(path)
    if save_notes:
        path = build_output_path(audio_path, output_directory, OutputExtensions.NOTE_EVENTS)
        save_note_events(note_events, path)
        written["note_events"] = str(path)
    return written


def predict_and_save_many(
    audio_path_list,
    output_directory: Union[pathlib.Path, str],
    save_midi: bool,
    sonify_midi: bool,
    save_model_outputs: bool,
    save_notes: bool,
    model_or_model_path: Union[Model, str, pathlib.Path] = ICASSP_2022_MODEL_PATH,
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    sonification_samplerate: int = DEFAULT_SONIFICATION_SAMPLERATE,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
    group: int = 64,
    decode_threads: Optional[int] = None,
    return_exceptions: bool = False,
) -> List[Any]:
    """`predict_and_save` (inference.py:509-618) as a batch job: ONE `predict_many` pipeline over all files (windows
    packed across files; the next group's files are read while this one is on the GPU; note decoding AND the writers of
    a finished file run on host threads behind it), a file's posteriorgrams are dropped once its outputs are written and
    the GPU runs at most two groups ahead, so memory stays at a few groups of posteriorgrams.  Same files, same bytes
    as the per-file loop.  Returns per file `{"n_note_events": k, "outputs": {kind: path}}` — or, with
    `return_exceptions=True`, the exception that file raised (otherwise the first failure propagates, like the
    reference's `raise e`).  Two inputs that map to the same output name (same stem) cannot both be written: as in the
    reference's sequential loop (inference.py:401-404) the first one wins and every later one gets the "already exists"
    IOError — decided up front, so concurrent writers never race on the exists-check."""
    model = _model_from(model_or_model_path)
    paths = [pathlib.Path(p) for p in audio_path_list]
    saving = save_midi or sonify_midi or save_model_outputs or save_notes
    # two inputs with the same stem would write the same files.  The map is made up front only so that concurrent writers
    # never race on the exists-check; what it MEANS follows the reference's sequential loop (inference.py:548-604): every
    # earlier file is predicted and written first, the later one then finds the outputs and gets the IOError — if the
    # earlier file really produced them — and nothing can collide when nothing is saved.
    dup = duplicate_output_stems(paths) if saving else {}
    if dup and not return_exceptions:
        paths = paths[: min(dup)]  # the loop would never get past the first duplicate: predict and write what precedes it
    todo = [i for i in range(len(paths)) if i not in dup]

    def finish_for(ids):
        def finish(j: int, res):
            written = _save_outputs(paths[ids[j]], output_directory, res, save_midi, sonify_midi, save_model_outputs,
                                    save_notes, sonification_samplerate)
            return {"n_note_events": len(res[2]), "outputs": written}
        return finish

    def run(ids):
        return predict_many([paths[i] for i in ids], model, onset_threshold, frame_threshold, minimum_note_length,
                            minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick, midi_tempo, group=group,
                            decode_threads=decode_threads, return_exceptions=return_exceptions, _finish=finish_for(ids))

    report: List[Any] = [None] * len(paths)
    for i, r in zip(todo, run(todo)):
        report[i] = r
    if dup and not return_exceptions:
        raise dup[min(dup)]  # every file in front of it has been written, like the reference's `raise e`
    # a duplicate whose earlier namesake FAILED (nothing was written under that stem) is an ordinary file after all
    first_of: Dict[str, int] = {}
    retry: List[int] = []
    retried: set = set()  # the stems of `retry`: one retry per stem, its later namesakes stay duplicates
    for i, p in enumerate(paths):
        stem = _output_stem(p)
        if i not in dup:
            first_of.setdefault(stem, i)
        elif isinstance(report[first_of.get(stem, i)], BaseException) and stem not in retried:
            retry.append(i)
            retried.add(stem)
        else:
            report[i] = dup[i]
    for i, r in zip(retry, run(retry) if retry else []):
        report[i] = r
    return report


def lane_models(model_path: Union[str, pathlib.Path] = ICASSP_2022_MODEL_PATH, devices: Optional[Sequence[int]] = None,
                lanes: int = 3) -> List[Model]:
    """The GPU lanes of a native file job: `lanes` models on every device of `devices` (default: device 0), device-major
    — lane i sits on devices[i // lanes].  Small workspaces (128 windows: one 3-minute track is 110), blocking waits so
    that a host thread parked on a lane leaves its core to the workers."""
    return [Model(model_path, device=int(d), max_windows=128, blocking_wait=True)
            for d in (devices if devices is not None else [0]) for _ in range(max(1, int(lanes)))]


def transcribe_files(
    audio_path_list,
    output_directory: Union[pathlib.Path, str],
    save_midi: bool = True,
    save_notes: bool = True,
    model_or_model_path: Union[Model, str, pathlib.Path] = ICASSP_2022_MODEL_PATH,
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
    models: Optional[Sequence[Model]] = None,
    lanes: int = 3,
    threads: int = 0,
    devices: Optional[Sequence[int]] = None,
    host_decode: bool = False,
    direct_io: bool = False,
    host_flac: bool = False,
    clip_batch: int = 0,
) -> List[Dict[str, Any]]:
    """The batch job of `predict_and_save` (inference.py:509-604) for WAV / AIFF / CAF / AU / FLAC input and MIDI /
    note-event output, run natively: ONE call into the library (`bp_transcribe_files`, csrc/file_pipeline.cpp), C++ worker threads from the
    file's bytes to its outputs, no Python in the loop.  Same bytes as `predict_and_save(..., save_midi, False, False,
    save_notes)`.  `models` (or `lanes` models per device of `devices` — default: device 0 — built from
    `model_or_model_path`) are the GPU lanes the workers queue for; lanes may live on different GPUs, a worker takes
    whichever is free, so ONE call shards its files over all GPUs of a node by itself (file-granular, no collective).
    Returns per file `{"status": 0 | bp_status, "n_note_events": k, "n_frames": T, "message": str, "ms": {stage: wall
    milliseconds of the worker}}`; per-file
    failures are reported, not raised (the reference's per-file try / except).  By default the dense half of note
    decoding runs on the device and 7 MB per 3-minute track come back instead of 27.6 (`host_decode=True`: the round-4
    path, all three posteriorgrams decoded on the host; same bytes).  `direct_io=True` reads the files with O_DIRECT straight
    into the page-locked buffers the GPU copies from (no page-cache copy; for corpora larger than the page cache).
    `clip_batch=N` (default 0: off) is for data sets of SHORT files — excerpts of at most 15 windows, about 25 s: a worker
    claims up to N consecutive inputs (at most 1024) and takes the short WAV / AIFF / CAF / AU / device-decodable FLAC files
    among them through one clips-events call per container and sample rate (`bp_infer_clips_events` / `bp_infer_flac_clips_events`) instead of one
    call per file; longer files, and whatever such a call does not finish, go the per-file route.  Same bytes, same reports.
    Measured on one MI355X with three lanes and 16 threads, jobs of 4,096 files with the outputs on a memory file system
    (profiles/files_clip_batches.md), files per second at N = 0 -> 64: one-window WAV 11,600 -> 61,200, four-window WAV 8,100 ->
    20,500, one-window FLAC 2,400 -> 50,200, four-window FLAC 2,400 -> 23,600.  N = 64 was best for three of the four corpora;
    choose N so that every worker thread gets several runs (512 files at N=256 keep two workers busy).  Where creating the
    output files bounds the job (5,000 creations per second on that machine's temporary directory) batching gains little:
    four-window WAV 0.94 x, FLAC 1.2 x."""
    own: List[Model] = []
    if models is None:
        if isinstance(model_or_model_path, Model):
            models = [model_or_model_path]
        else:
            own = lane_models(model_or_model_path, devices, lanes)
            models = own
    try:
        lib = models[0]._lib
        verify_output_dir(output_directory)
        paths = [os.fsencode(str(p)) for p in audio_path_list]
        n = len(paths)
        prm = _native.bp_transcribe_params()
        lib.bp_transcribe_params_default(C.byref(prm))
        # the decoder settings of model_output_to_notes (infer_onsets, the energy tolerance and pitch bends at its defaults)
        prm.notes = infer._note_params(
            onset_threshold, frame_threshold, _min_note_len_frames(minimum_note_length), True, maximum_frequency,
            minimum_frequency, melodia_trick, infer.ENERGY_TOLERANCE, True,
        )
        prm.midi_tempo = float(midi_tempo)
        prm.multiple_pitch_bends = int(bool(multiple_pitch_bends))
        prm.save_midi, prm.save_notes, prm.threads = int(bool(save_midi)), int(bool(save_notes)), int(threads)
        prm.host_decode = int(bool(host_decode))
        prm.direct_io = int(bool(direct_io))
        prm.host_flac = int(bool(host_flac))  # FLAC files: decoded on the device unless asked otherwise
        if int(clip_batch) < 0:
            raise ValueError("clip_batch must be >= 0")
        prm.clip_batch = int(clip_batch)
        handles = (C.c_void_p * len(models))(*[m._handle for m in models])
        cpaths = (C.c_char_p * max(1, n))(*paths)
        reports = (_native.bp_file_report * max(1, n))()
        rc = lib.bp_transcribe_files(handles, len(models), cpaths, n, os.fsencode(str(output_directory)), C.byref(prm), reports)
        if rc != _native.BP_OK:
            raise ValueError(f"bp_transcribe_files: {lib.bp_files_last_error().decode(errors='replace')}")
        return [{"status": int(reports[i].status), "n_note_events": int(reports[i].n_note_events),
                 "n_frames": int(reports[i].n_frames), "message": reports[i].message.decode(errors="replace"),
                 "ms": {k: float(getattr(reports[i], "ms_" + k)) for k in ("read", "lane_wait", "device", "notes", "write")}}
                for i in range(n)]
    finally:
        for m in own:
            m.close()


def duplicate_output_stems(paths: Sequence[Union[pathlib.Path, str]]) -> Dict[int, IOError]:
    """Indices of inputs whose output name `<stem>_basic_pitch.*` (build_output_path) an EARLIER input of the list
    already claims, with the IOError the reference's sequential loop would give them (inference.py:401-404)."""
    seen: Dict[str, int] = {}
    dup: Dict[int, IOError] = {}
    for i, p in enumerate(paths):
        stem = _output_stem(p)
        if stem in seen:
            dup[i] = IOError(f"the outputs of {p} would overwrite those of {paths[seen[stem]]} (same file stem "
                             f"'{stem}'). Skipping output files for {p}.")
        else:
            seen[stem] = i
    return dup


def predict_and_save(
    audio_path_list,
    output_directory: Union[pathlib.Path, str],
    save_midi: bool,
    sonify_midi: bool,
    save_model_outputs: bool,
    save_notes: bool,
    model_or_model_path: Union[Model, str, pathlib.Path] = ICASSP_2022_MODEL_PATH,
    onset_threshold: float = DEFAULT_ONSET_THRESHOLD,
    frame_threshold: float = DEFAULT_FRAME_THRESHOLD,
    minimum_note_length: float = DEFAULT_MINIMUM_NOTE_LENGTH_MS,
    minimum_frequency: Optional[float] = None,
    maximum_frequency: Optional[float] = None,
    multiple_pitch_bends: bool = False,
    melodia_trick: bool = True,
    debug_file: Optional[pathlib.Path] = None,
    sonification_samplerate: int = DEFAULT_SONIFICATION_SAMPLERATE,
    midi_tempo: float = DEFAULT_MINIMUM_MIDI_TEMPO,
) -> None:
    """inference.py:509-618: model output (.npz), MIDI (.mid), sonified MIDI (.wav), note events (.csv) per file."""
    model = _model_from(model_or_model_path)
    for audio_path in audio_path_list:
        result = predict(
            pathlib.Path(audio_path), model, onset_threshold, frame_threshold, minimum_note_length,
            minimum_frequency, maximum_frequency, multiple_pitch_bends, melodia_trick, debug_file, midi_tempo,
        )
        _save_outputs(audio_path, output_directory, result, save_midi, sonify_midi, save_model_outputs, save_notes,
                      sonification_samplerate)
