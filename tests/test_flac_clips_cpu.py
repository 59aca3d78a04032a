"""A job of FLAC clips in one call, the part that needs no GPU: the calls of include/basic_pitch_amd_flac_clips.h are exported
with the prototypes that header declares, they refuse a null handle, the row offsets and host-side statuses of a job, and the
grouping by STREAMINFO rate of the Python layer.

`bp_flac_clips_row_offsets` takes a handle, and a handle needs a device.  Where one can be made the call itself is compared with
the running sum of `bp_handle_track_n_frames(bp_handle_resampled_length(n_frames, rate))` over each clip's `bp_flac_layout`, a
clip left to the host counting no rows.  Without a device the pure-Python mirror `flac_clips.row_offsets` is checked against
`clips.row_offsets` and the handle-free forms of those two calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flac_writer as FW
from conftest import ROOT
from test_clips_cpu import _SCALAR, _ctype_of

NEW = ("bp_flac_clips_row_offsets", "bp_flac_clips_decode_device", "bp_infer_flac_clips_candidates", "bp_infer_flac_clips_events")
RATE = 44100


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, flac_clips

    build.build_library()
    return flac_clips.bind(_native.load_library())


@pytest.fixture(scope="module")
def model():
    """A model where a device is visible, else None."""
    from basic_pitch_amd import _native
    from basic_pitch_amd.inference import Model

    try:
        m = Model(device=0, max_windows=8)
    except _native.NativeLibraryError:
        yield None
        return
    yield m
    m.close()


def _tone(n, ch, bits, seed):
    rng = np.random.default_rng(seed)
    full = 1 << (bits - 1)
    x = 0.3 * full * np.sin(np.arange(n)[:, None] * (0.05 + 0.01 * np.arange(ch))) + rng.integers(-3, 4, (n, ch))
    return x.astype(np.int64)


@pytest.fixture(scope="module")
def job():
    """(blobs, what each is, left to the host?): lengths around 0, 1 and 142 rows at 44.1 kHz, and every host-side reason."""
    out = []
    for n, ch, bits, bs in ((100, 1, 16, 192), (509, 2, 16, 192), (510, 1, 8, 192), (511, 2, 24, 576), (72326, 1, 16, 4096),
                            (72328, 1, 16, 4096), (5000, 2, 16, 1152)):
        out.append((FW.encode(_tone(n, ch, bits, n), RATE, bits, blocksize=bs), f"{n} frames", False))
    pcm = _tone(9000, 2, 16, 1)
    out.insert(2, (FW.encode(pcm, RATE, 16, blocksize=1152, total_in_header=False), "no sample count in STREAMINFO", True))
    out.insert(4, (FW.encode(_tone(20000, 2, 16, 2), RATE, 16, sizes=[16, 4608]), "block sizes 16 and 4608: the scratch bound", True))
    out.insert(5, (FW.encode(_tone(20000, 2, 16, 3), RATE, 16, sizes=[1152, 576, 2304]), "block sizes 576 to 2304: inside the bound", False))
    out.append((out[0][0][:41], "41 bytes", True))
    out.append((b"", "no bytes", True))
    out.append((b"RIFF" + bytes(200), "not FLAC", True))
    return out


def _layout(lib, blob):
    from basic_pitch_amd import _native

    lay = _native.bp_flac_stream_layout()
    if not blob or lib.bp_flac_layout(bytes(blob), len(blob), C.byref(lay)) != _native.BP_OK:
        return None
    return {k: int(getattr(lay, k)) for k, _ in lay._fields_}


def test_every_symbol_of_the_flac_clips_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, build, flac_clips
    from basic_pitch_amd.inference import Model

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_flac_clips.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert '#include "basic_pitch_amd_events.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(flac_clips.PROTOTYPES) == set(_native.FLAC_CLIPS_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert flac_clips.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    assert names("bp_flac_clips_row_offsets") == ["h", "n_clips", "clips", "sample_rate", "offsets", "status"]
    assert names("bp_flac_clips_decode_device") == ["h", "n_clips", "clips", "pcm", "pcm_offsets", "status"]
    assert names("bp_infer_flac_clips_candidates") == ["h", "n_clips", "clips", "sample_rate", "params", "note_out", "cand_bits",
                                                       "bend_map", "status"]
    assert names("bp_infer_flac_clips_events") == ["h", "n_clips", "clips", "sample_rate", "params", "events", "max_events", "bends",
                                                   "max_bends", "event_offsets", "status"]
    # the struct and the two statuses as the header lays them out
    assert re.search(r"typedef struct \{ const void\* file; size_t nbytes; \} bp_flac_clip;", header)
    assert [f[0] for f in flac_clips.bp_flac_clip._fields_] == ["file", "nbytes"] and C.sizeof(flac_clips.bp_flac_clip) == 16
    values = {k: int(v) for k, v in re.findall(r"#define (BP_CLIP_FLAC_[A-Z]+) (\d+)", header)}
    assert values == {"BP_CLIP_FLAC_HOST": _native.BP_CLIP_FLAC_HOST, "BP_CLIP_FLAC_FAILED": _native.BP_CLIP_FLAC_FAILED}
    assert len({0, 1, 2} | set(values.values())) == 5
    # the other headers' lists are what they were; the source and the header are part of the build
    others = set(_native.EXPORTED_SYMBOLS) | set(_native.CLIPS_SYMBOLS) | set(_native.EVENTS_SYMBOLS)
    assert not set(NEW) & others and "bp_infer_flac_candidates" in _native.EXPORTED_SYMBOLS
    assert "flac_clips.hip" in build.SOURCES and "flac_device.hip" in build.SOURCES
    assert {"basic_pitch_amd_flac_clips.h", "flac_kernels.h"} <= {os.path.basename(h) for h in build.HEADERS}
    assert hasattr(Model, "transcribe_flac_clips")


def test_a_null_handle_is_refused_by_every_call(lib, job):
    from basic_pitch_amd import _native, flac_clips

    tab, keep = flac_clips.clip_table([b for b, _, _ in job])
    n = len(keep)
    offs, status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
    p64 = offs.ctypes.data_as(C.POINTER(C.c_int64))
    prm = _native.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    big = np.zeros(1 << 16, np.int32)
    assert lib.bp_flac_clips_row_offsets(None, n, tab, RATE, p64, status.ctypes.data) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_flac_clips_decode_device(None, n, tab, big.ctypes.data, p64, status.ctypes.data) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_flac_clips_candidates(None, n, tab, RATE, C.addressof(prm), big.ctypes.data, big.ctypes.data, big.ctypes.data,
                                              status.ctypes.data) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_flac_clips_events(None, n, tab, RATE, C.addressof(prm), big.ctypes.data, 16, big.ctypes.data, 16, p64,
                                          status.ctypes.data) == _native.BP_ERR_INVALID_ARG


def test_row_offsets_are_the_running_sum_of_the_device_clips_rows(lib, model, job):
    from basic_pitch_amd import _native, clips, flac_clips

    blobs = [b for b, _, _ in job]
    lays = [_layout(lib, b) for b in blobs]
    want_host = [h for _, _, h in job]
    # the fixture is what it says: every host-side reason is there, and the variable stream inside the bound is not one
    assert [flac_clips.left_to_host(l, len(b)) for l, b in zip(lays, blobs)] == want_host
    assert sum(want_host) == 5 and sum(l is None for l in lays) == 3
    assert any(l and l["n_frames"] == 0 for l in lays) and any(l and (l["min_block"], l["max_block"]) == (16, 4608) for l in lays)
    assert any(l and (l["min_block"], l["max_block"]) == (576, 2304) and not h for l, h in zip(lays, want_host))
    frames = [0 if h else l["n_frames"] for l, h in zip(lays, want_host)]
    if model is not None:
        rows = [lib.bp_handle_track_n_frames(model._handle, lib.bp_handle_resampled_length(model._handle, f, RATE)) for f in frames]
    else:
        rows = [lib.bp_track_n_frames(lib.bp_resampled_length(f, RATE)) for f in frames]
    want = np.concatenate([[0], np.cumsum(rows)])
    assert {0, 1, 141, 142} <= set(rows) and rows[0] == 0 and frames[0] == 100  # a device clip without rows too
    offs, status = flac_clips.row_offsets(lays, [len(b) for b in blobs], RATE)
    assert np.array_equal(offs, want) and np.array_equal(offs, clips.row_offsets(frames, RATE))
    assert status.tolist() == [_native.BP_CLIP_FLAC_HOST if h else 0 for h in want_host]
    assert np.array_equal(flac_clips.row_offsets([], [], RATE)[0], [0])
    if model is not None:
        got, got_status = flac_clips.flac_clips_row_offsets(model, blobs, RATE)
        assert got.dtype == np.int64 and np.array_equal(got, want) and got_status.tolist() == status.tolist()
        for k in range(len(blobs)):  # any grouping: a clip's rows and status are its own
            g, s = flac_clips.flac_clips_row_offsets(model, blobs[k:], RATE)
            assert np.array_equal(np.diff(g), np.diff(want)[k:]) and s.tolist() == status.tolist()[k:]
        assert np.array_equal(flac_clips.flac_clips_row_offsets(model, [], RATE)[0], [0])
        # one rate per call: the first clip whose STREAMINFO says another is named (a clip without rows has a rate too; one
        # without a STREAMINFO has none)
        with pytest.raises(ValueError, match=r"clip 0: .*44100 Hz.*48000"):
            flac_clips.flac_clips_row_offsets(model, blobs, 48000)
        with pytest.raises(ValueError, match=r"clip 2: .*44100 Hz.*48000"):
            flac_clips.flac_clips_row_offsets(model, [b"", b"RIFF" + bytes(200)] + blobs, 48000)


def test_clips_are_grouped_by_their_streaminfo_rate():
    from basic_pitch_amd import flac_clips

    lays = [{"sample_rate": r} if r else None for r in (44100, 22050, None, 44100, 48000, 22050, None, 44100)]
    groups, none = flac_clips.group_by_rate(lays)
    assert list(groups) == [44100, 22050, 48000]  # in order of first appearance
    assert groups == {44100: [0, 3, 7], 22050: [1, 5], 48000: [4]} and none == [2, 6]
    assert flac_clips.group_by_rate([]) == ({}, [])
    with pytest.raises(ValueError, match="decode must be"):
        flac_clips.transcribe_flac_clips(None, [], 0.5, 0.3, 127.7, None, None, False, True, 120, decode="gpu")
    with pytest.raises(ValueError, match="errors must be"):
        flac_clips.transcribe_flac_clips(None, [], 0.5, 0.3, 127.7, None, None, False, True, 120, errors="ignore")
