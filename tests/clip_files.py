"""Short audio files for the tests of the file job's batches (bp_transcribe_params.clip_batch): a RIFF/WAVE writer for
every sample format the native reader takes, signals with notes in them, and the probe's call."""
import ctypes as C
import os
import struct

import numpy as np

# the default mode's geometry (bp_track_n_windows): windows = ceil((samples at 22,050 Hz + 3,840) / 36,164)
HOP, LEAD = 36164, 3840
ONE_WINDOW = HOP - LEAD           # the most samples at 22,050 Hz of a one-window file
MAX_SHORT = 15 * HOP - LEAD       # ... of a 15-window file: the longest a batched call takes

FORMATS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}


def tones(n, channels, rate, seed):
    """Float64 [n, channels] in (-1, 1): three steady tones (another chord per seed) and a little noise."""
    rng = np.random.default_rng(seed)
    pitches = (48, 52, 55, 60, 64, 67, 72, 57, 62, 65)
    t = np.arange(n) / rate
    x = np.zeros((n, channels))
    for c in range(channels):
        for k in range(3):
            f = 440.0 * 2 ** ((pitches[(seed + 3 * c + 2 * k) % len(pitches)] - 69) / 12)
            x[:, c] += 0.2 * np.sin(2 * np.pi * f * t + k)
    return x + 1e-3 * rng.standard_normal((n, channels))


def pcm_bytes(x, fmt):
    """Float samples [n, channels] as the bytes a WAV file of format `fmt` stores."""
    x = np.asarray(x, np.float64)
    if fmt == "u8":
        return np.clip(np.round(x * 127) + 128, 0, 255).astype(np.uint8).tobytes()
    if fmt == "s16":
        return np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    if fmt == "s24":
        v = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4")
        return v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if fmt == "s32":
        return np.clip(np.round(x * 2147483647), -2147483648, 2147483647).astype("<i4").tobytes()
    return x.astype("<f4" if fmt == "f32" else "<f8").tobytes()


def wav_bytes(data, fmt, channels, rate):
    tag, bits = FORMATS[fmt]
    width = bits // 8
    head = struct.pack("<4sI4s4sIHHIIHH", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, tag, channels, rate,
                       rate * channels * width, channels * width, bits)
    return head + struct.pack("<4sI", b"data", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def write_wav(path, x, fmt, rate):
    """x: float [n, channels] (n may be 0)."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 2
    with open(path, "wb") as f:
        f.write(wav_bytes(pcm_bytes(x, fmt), fmt, x.shape[1], rate))
    return str(path)


def params(lib, clip_batch=1, **fields):
    from basic_pitch_amd import _native

    prm = _native.bp_transcribe_params()
    lib.bp_transcribe_params_default(C.byref(prm))
    prm.clip_batch = clip_batch
    for k, v in fields.items():
        setattr(prm, k, v)
    return prm


def probe(lib, paths, prm, handles=()):
    """bp_files_batch_probe: (rc, routes).  Without handles the default mode's geometry counts the windows."""
    n = len(paths)
    cpaths = (C.c_char_p * max(1, n))(*[os.fsencode(str(p)) for p in paths])
    route = (C.c_int32 * max(1, n))(*([99] * max(1, n)))
    hs = (C.c_void_p * len(handles))(*handles) if handles else None
    rc = lib.bp_files_batch_probe(hs, len(handles), cpaths, n, C.byref(prm), route)
    return rc, list(route)[:n]
