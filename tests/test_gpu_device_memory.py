"""Device memory of handles and streams (csrc/device_buffer.h): everything a handle or a stream allocates, lazily or not, is
gone when it is destroyed or closed, a create or an open that fails leaves nothing behind, and workspace_bytes is the
sum it was before the buffers had owners (profiles/device_buffer_refactor.md).

The count is the A/B library's own (bp_ab_live_device_bytes, declared nowhere: named here): the GPUs are shared, so the
free memory the device reports moves with other processes' work.  Nothing here faults: the failures are argument errors."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import flac_writer as FW
from conftest import ROOT

pytestmark = pytest.mark.gpu

HOP, WIN = 36164, 43844
BP_ERR_BAD_WEIGHTS, BP_ERR_UNSUPPORTED = -2, -6
# 44101 Hz -> 22050 Hz: the rates are coprime (up 22050, down 44101), and make_resample_plan's rule — evaluated on the
# CPU with the oracle's kaiser_beta — gives the filter n_taps = 8,478,253 > kMaxTableTaps = 2^22 (44100 Hz: 389 taps): the
# one-shot calls evaluate such taps in the kernel, bp_stream_open refuses the rate
UNTABULATED_RATE = 44101


@pytest.fixture(scope="module")
def nat():
    from basic_pitch_amd import _native

    return _native


@pytest.fixture(scope="module")
def blob():
    return open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()


@pytest.fixture(scope="module")
def ab(nat):
    from basic_pitch_amd import build, streaming

    lib = streaming.bind(nat.load_library(build.build_library(ab=True)))
    lib.bp_ab_live_device_bytes.restype, lib.bp_ab_live_device_bytes.argtypes = C.c_int64, []
    return lib


def _maps(rows):
    return [np.empty((rows, w), np.float32) for w in (88, 88, 264)]


def _ptrs(arrays):
    return [a.ctypes.data for a in arrays]


def _use_every_lazy_path(lib, nat, h, flac):
    """Every call of a handle that allocates on first use; returns nothing: the work is ordinary and must succeed."""
    def ok(rc, what):
        assert rc == 0, (what, rc, lib.bp_last_error(h))

    live = lib.bp_ab_live_device_bytes
    rng = np.random.default_rng(5)
    prm = nat.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    rows, status = C.c_int64(), C.c_int()

    x = rng.uniform(-1, 1, (2, WIN)).astype(np.float32)
    out = _maps(2 * 172)  # held in a name: the library writes to them
    ok(lib.bp_infer(h, x.ctypes.data, 2, *_ptrs(out), nat.BP_MEM_HOST), "bp_infer")

    n = HOP + 1
    track = rng.uniform(-1, 1, n).astype(np.float32)
    out = _maps(lib.bp_track_n_frames(n))
    ok(lib.bp_infer_track(h, track.ctypes.data, n, *_ptrs(out), nat.BP_MEM_HOST), "bp_infer_track")

    pcm = rng.integers(-32768, 32768, 2 * 22050).astype(np.int16)  # 0.5 s of 44.1 kHz stereo
    T = lib.bp_track_n_frames(lib.bp_resampled_length(22050, 44100))
    assert T > 0
    note, bits, bend = np.empty((T, 88), np.float32), np.empty((T, 12), np.uint8), np.empty((T, 88), np.int8)
    ok(lib.bp_infer_pcm_raw_candidates(h, pcm.ctypes.data, nat.BP_PCM_S16, 22050, 2, 44100, C.byref(prm), note.ctypes.data,
                                       bits.ctypes.data, bend.ctypes.data, C.byref(status)), "bp_infer_pcm_raw_candidates")
    out = _maps(T)
    ok(lib.bp_track_maps(h, T, *_ptrs(out), nat.BP_MEM_HOST), "bp_track_maps")

    out = _maps(lib.bp_track_n_frames(22050))
    ok(lib.bp_infer_flac(h, flac, len(flac), *_ptrs(out), nat.BP_MEM_HOST), "bp_infer_flac")

    # a rate the streams refuse: an argument error that allocates nothing
    before, s = live(), C.c_void_p()
    assert lib.bp_stream_open(h, nat.BP_PCM_S16, 1, UNTABULATED_RATE, C.byref(s)) == BP_ERR_UNSUPPORTED and not s.value
    assert live() == before

    # a 44.1 kHz stream that keeps its maps: one push of a window and a hop of the model-rate signal, peek, candidates
    cap = 1000
    out = _maps(cap)
    ok(lib.bp_stream_open(h, nat.BP_PCM_S16, 1, 44100, C.byref(s)), "bp_stream_open 44100")
    ok(lib.bp_stream_keep(s, C.byref(prm), cap), "bp_stream_keep")
    chunk = rng.integers(-32768, 32768, 2 * (WIN + HOP)).astype(np.int16)
    ok(lib.bp_stream_push(s, chunk.ctypes.data, len(chunk), nat.BP_MEM_HOST, *_ptrs(out), cap, nat.BP_MEM_HOST, C.byref(rows)), "push")
    assert rows.value == 2 * 142
    ok(lib.bp_stream_peek(s, *_ptrs(out), cap, nat.BP_MEM_HOST, C.byref(rows)), "bp_stream_peek")
    assert rows.value > 0
    note, bits, bend = np.empty((cap, 88), np.float32), np.empty((cap, 12), np.uint8), np.empty((cap, 88), np.int8)
    ok(lib.bp_stream_candidates(s, 1, note.ctypes.data, bits.ctypes.data, bend.ctypes.data, 0, cap, C.byref(rows),
                                C.byref(status)), "bp_stream_candidates")
    assert rows.value > 2 * 142
    # closing a stream gives back exactly its ring, its history and its kept maps
    before, state = live(), lib.bp_stream_state_bytes(s)
    lib.bp_stream_close(s)
    assert state > cap * 440 * 4 and before - live() == state

    # a 22.05 kHz stream (no resampling, no history): push, finish, close
    ok(lib.bp_stream_open(h, nat.BP_PCM_F32, 1, 22050, C.byref(s)), "bp_stream_open 22050")
    chunk = rng.uniform(-1, 1, WIN + HOP).astype(np.float32)
    ok(lib.bp_stream_push(s, chunk.ctypes.data, len(chunk), nat.BP_MEM_HOST, *_ptrs(out), cap, nat.BP_MEM_HOST, C.byref(rows)), "push")
    assert rows.value == 2 * 142
    ok(lib.bp_stream_finish(s, *_ptrs(out), cap, nat.BP_MEM_HOST, C.byref(rows)), "bp_stream_finish")
    assert rows.value > 0
    before, state = live(), lib.bp_stream_state_bytes(s)
    lib.bp_stream_close(s)
    assert before - live() == state == (WIN + 4 * HOP) * 4


def test_a_handle_and_its_streams_free_everything_they_allocated(ab, nat, blob):
    live = ab.bp_ab_live_device_bytes
    assert live() == 0
    rng = np.random.default_rng(9)
    tone = (8000 * np.sin(2 * np.pi * 220 * np.arange(22050) / 22050) + rng.integers(-50, 51, 22050)).astype(np.int16)
    flac = FW.encode(tone[:, None], 22050, 16, blocksize=4096)
    for cycle in range(2):
        h = C.c_void_p()
        assert ab.bp_create(blob, len(blob), 0, 0, 2, C.byref(h)) == 0, ab.bp_last_error(None)
        info = nat.bp_info()
        assert ab.bp_get_info(h, C.byref(info)) == 0 and info.max_windows == 2
        assert live() > info.workspace_bytes > 0  # mm and the filterbank scratch are held but not reported
        at_create = live()
        _use_every_lazy_path(ab, nat, h, flac)
        assert live() > at_create, cycle  # the staging buffers, the filters, the FLAC decoder's lists
        assert ab.bp_get_info(h, C.byref(info)) == 0 and live() > info.workspace_bytes
        ab.bp_destroy(h)
        assert live() == 0, cycle

    # creates that fail: a flag combination refused after the handle exists, weights refused before
    h = C.c_void_p()
    flags = nat.BP_FLAG_EXT_CQT_44K | nat.BP_FLAG_F32_MFMA
    assert ab.bp_create(blob, len(blob), 0, flags, 2, C.byref(h)) == BP_ERR_UNSUPPORTED and not h.value
    assert live() == 0
    renamed = bytearray(blob)  # the blobs of test_create_rejects_bad_weights
    renamed[16 : 16 + 24] = b"not_a_tensor".ljust(24, b"\0")
    assert struct.unpack_from("<I", blob, 12)[0] == 19
    for bad in (b"garbage", blob[:1000], bytes(renamed)):
        assert ab.bp_create(bad, len(bad), 0, 0, 2, C.byref(h)) == BP_ERR_BAD_WEIGHTS and not h.value
        assert live() == 0


# workspace_bytes of the parent of the change that gave the buffers owners, summed by that parent's own packing code
# (profiles/device_buffer_refactor.md): a deterministic sum over the tables and the workspace of bp_create — no margin
WORKSPACE_BYTES = [
    ("default", 0, 256, 2_143_170_220),
    ("exact f32", 2, 256, 2_044_473_004),
    ("bf16 weights", 4, 256, 2_143_170_220),
    ("extended 44.1 kHz", 8, 512, 4_661_649_356),
]


@pytest.mark.parametrize("name,flags,max_windows,expected", WORKSPACE_BYTES, ids=[w[0] for w in WORKSPACE_BYTES])
def test_workspace_bytes_is_what_it_was(nat, blob, name, flags, max_windows, expected):
    lib = nat.load_library()
    h = C.c_void_p()
    assert lib.bp_create(blob, len(blob), 0, flags, max_windows, C.byref(h)) == 0, lib.bp_last_error(None)
    info = nat.bp_info()
    rc = lib.bp_get_info(h, C.byref(info))
    lib.bp_destroy(h)
    assert rc == 0 and info.workspace_bytes == expected, (name, info.workspace_bytes)
