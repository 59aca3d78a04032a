"""Many clips in one call, the part that needs no GPU: the calls of include/basic_pitch_amd_clips.h are exported with the
prototypes that header declares, the row offsets of a job of clips, and the refusals that name the offending clip.

`bp_clips_row_offsets` takes a handle, and a handle needs a device.  Where one can be made (a GPU machine) the call itself is
compared with the running sum of `bp_handle_track_n_frames(bp_handle_resampled_length(...))` and its refusals are read from
`bp_last_error`.  Without a device the same lengths go through the handle-free forms `bp_track_n_frames(bp_resampled_length(...))`
and check the pure-Python mirror `clips.row_offsets`, which restates the documented formula; the refusals checked are those
of the Python layer, and the native call's answer to a null handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("bp_clips_row_offsets", "bp_infer_clips_candidates")
RATES = (22050, 44100, 48000)
# lengths at the model's rate: no samples; the first lengths with 1, 2 and 3 rows and their predecessors (int(n / 36164 * 142));
# the last length of one window and the first of two (ceil((n + 3840) / 36164)); one hop -1, 0, +1 (141, 142, 142 rows); two
# windows + 1 sample of audio
MODEL_LENGTHS = (0, 1, 254, 255, 509, 510, 764, 765, 32324, 32325, 36163, 36164, 36165, 2 * 36164 + 1)


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build, clips

    build.build_library()
    return clips.bind(_native.load_library())


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


def _source_lengths(rate):
    """Frames at `rate` around every model-rate length: the resampled length ceil(f * 22050 / rate) lands on it and beside it."""
    out = []
    for n in MODEL_LENGTHS:
        f = n * rate // 22050
        out += [max(0, f - 1), f, f + 1]
    return out


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "bp_handle": C.c_void_p}


def _ctype_of(param):
    """The rule of tests/test_stream_peek_cpu.py: handles and plain data pointers (structs, bytes, `int*` among them) are void
    pointers, `int64_t*` a pointer to int64."""
    words = re.sub(r"\bconst\b", " ", param).replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w != "*"][0]
    if stars == 0:
        return _SCALAR[base]
    assert stars == 1, param
    return C.POINTER(C.c_int64) if base == "int64_t" else C.c_void_p


def test_every_symbol_of_the_clips_header_is_exported_with_its_prototype(lib):
    from basic_pitch_amd import _native, clips
    from basic_pitch_amd.inference import Model

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_clips.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert '#include "basic_pitch_amd.h"' in header
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r"\b(void|int|int64_t)\s+(bp_[a-z_]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(protos) == set(NEW) == set(clips.PROTOTYPES) == set(_native.CLIPS_SYMBOLS)
    assert set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", header)) == set(NEW)  # every symbol the header declares
    for name in NEW:
        ret, params = protos[name]
        want = (_SCALAR[ret], [_ctype_of(p.strip()) for p in params.split(",")])
        assert clips.PROTOTYPES[name] == want, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype == want[0] and list(fn.argtypes) == want[1], name
    names = lambda name: [p.split()[-1].lstrip("*") for p in protos[name][1].split(",")]  # noqa: E731
    assert names("bp_clips_row_offsets") == ["h", "n_clips", "clips", "sample_rate", "offsets"]
    assert names("bp_infer_clips_candidates") == ["h", "n_clips", "clips", "sample_rate", "pcm_mem_kind", "params", "note_out",
                                                  "cand_bits", "bend_map", "status"]
    # the struct as the header lays it out
    assert re.search(r"typedef struct \{ const void\* pcm; int64_t n_frames; int format; int channels; \} bp_clip;", header)
    assert [f[0] for f in clips.bp_clip._fields_] == ["pcm", "n_frames", "format", "channels"] and C.sizeof(clips.bp_clip) == 24
    # the existing header and lists are what they were
    assert not set(NEW) & set(_native.EXPORTED_SYMBOLS) and "bp_infer_pcm_raw_candidates" in _native.EXPORTED_SYMBOLS
    assert hasattr(Model, "transcribe_clips")


@pytest.mark.parametrize("rate", RATES)
def test_row_offsets_are_the_running_sum_of_the_clips_rows(lib, model, rate):
    from basic_pitch_amd import clips

    lengths = _source_lengths(rate)
    if model is not None:
        rows = [lib.bp_handle_track_n_frames(model._handle, lib.bp_handle_resampled_length(model._handle, f, rate)) for f in lengths]
    else:
        rows = [lib.bp_track_n_frames(lib.bp_resampled_length(f, rate)) for f in lengths]
    want = np.concatenate([[0], np.cumsum(rows)])
    # the cases the list is there for: 0, 1, 2 and 3 rows, the rows of one window's length -1, 0, +1, two windows + 1 sample
    at_model_rate = [lib.bp_track_n_frames(n) for n in MODEL_LENGTHS]
    assert at_model_rate == [0, 0, 0, 1, 1, 2, 2, 3, 126, 126, 141, 142, 142, 284]
    assert [lib.bp_track_n_windows(n) for n in (32324, 32325, 2 * 36164 + 1)] == [1, 2, 3]
    assert {0, 1, 2, 3, 141, 142} <= set(rows)
    if model is not None:
        arrays = [np.zeros((f, 1 + i % 2), np.int16) for i, f in enumerate(lengths)]  # the channel count changes no row
        got = clips.clips_row_offsets(model, arrays, rate)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(clips.clips_row_offsets(model, [], rate), [0])
    # the documented formula, restated without the library
    assert np.array_equal(clips.row_offsets(lengths, rate), want)
    assert np.array_equal(clips.row_offsets([], rate), [0])


def test_bad_clips_are_refused_and_the_message_names_the_clip(lib, model):
    from basic_pitch_amd import _native, clips

    good = [np.zeros((100, 2), np.int16), np.zeros(50, np.float32), np.zeros((0, 1), np.uint8)]
    # the Python layer: a sample type or a shape the library has no format for
    for bad, word in ((np.zeros(10, np.int8), "int8"), (np.zeros((4, 2, 2), np.float32), "shape"),
                      (np.zeros((4, 65), np.float32), "channels"), (np.zeros((4, 0), np.float32), "channels")):
        with pytest.raises(ValueError, match=r"clip 2: .*" + word):
            clips.as_clip(bad, 2)
        for at in (0, 3):
            with pytest.raises(ValueError, match=f"clip {at}: "):
                [clips.as_clip(c, i) for i, c in enumerate(good[:at] + [bad] + good[at:])]
    with pytest.raises(ValueError, match="3 clips but 2 sample rates"):
        clips.transcribe_clips(None, good, [44100, 22050], 0.5, 0.3, 127.7, None, None, False, True, 120)
    # the native calls without a handle
    offs = np.zeros(4, np.int64)
    tab = clips.clip_table([clips.as_clip(c, i) for i, c in enumerate(good)])
    assert lib.bp_clips_row_offsets(None, 3, tab, 44100, offs.ctypes.data_as(C.POINTER(C.c_int64))) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_infer_clips_candidates(None, 3, tab, 44100, 0, None, None, None, None, None) == _native.BP_ERR_INVALID_ARG
    if model is None:
        return
    # the native argument domain (that of bp_infer_pcm_raw) clip by clip: the first offending clip is named
    h = model._handle
    err = lambda: lib.bp_last_error(h).decode()  # noqa: E731
    prm = _native.bp_note_params()
    lib.bp_note_params_default(C.byref(prm))
    out = (np.zeros((64, 88), np.float32), np.zeros((64, 12), np.uint8), np.zeros((64, 88), np.int8), np.zeros(8, np.int32))

    def both(table, n, rate, where):
        rc = lib.bp_clips_row_offsets(h, n, table, rate, offs.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == _native.BP_ERR_INVALID_ARG and where in err() and "bp_clips_row_offsets" in err(), err()
        rc = lib.bp_infer_clips_candidates(h, n, table, rate, _native.BP_MEM_HOST, C.addressof(prm), *[o.ctypes.data for o in out])
        assert rc == _native.BP_ERR_INVALID_ARG and where in err() and "bp_infer_clips_candidates" in err(), err()

    # (formats 0 ... 13 exist, BP_PCM_F32 ... BP_PCM_ALAW: 14 is the first code past them)
    for field, value in (("n_frames", -1), ("format", _native.BP_PCM_ALAW + 1), ("format", -1), ("channels", 0), ("channels", 65)):
        for at in (0, 1, 2):
            t = clips.clip_table([clips.as_clip(c, i) for i, c in enumerate(good)])
            setattr(t[at], field, value)
            if at < 2:
                t[2].channels = 99  # a later offender is not the one named
            both(t, 3, 44100, f"clip {at}:")
    for rate in (999, 768001):
        both(tab, 3, rate, "clip 0:")
    # samples are needed by the call that reads them, and only by it
    t = clips.clip_table([clips.as_clip(c, i) for i, c in enumerate(good)])
    t[1].pcm = None
    assert lib.bp_clips_row_offsets(h, 3, t, 44100, offs.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    rc = lib.bp_infer_clips_candidates(h, 3, t, 44100, _native.BP_MEM_HOST, C.addressof(prm), *[o.ctypes.data for o in out])
    assert rc == _native.BP_ERR_INVALID_ARG and "clip 1:" in err()
    rc = lib.bp_infer_clips_candidates(h, 3, tab, 44100, 7, C.addressof(prm), *[o.ctypes.data for o in out])
    assert rc == _native.BP_ERR_INVALID_ARG and "clip 0:" in err()
    assert lib.bp_clips_row_offsets(h, -1, tab, 44100, offs.ctypes.data_as(C.POINTER(C.c_int64))) == _native.BP_ERR_INVALID_ARG
    assert lib.bp_clips_row_offsets(h, 3, tab, 44100, None) == _native.BP_ERR_INVALID_ARG
