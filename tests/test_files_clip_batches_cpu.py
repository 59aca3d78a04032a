"""Batches of short files in the native file job (bp_transcribe_params.clip_batch), the part that needs no GPU: the setting
sits where `reserved[0]` sat and nothing else of the struct moved, and `bp_files_batch_probe` — the function the job's
workers decide with — routes files by their headers.

A handle needs a device, so the probe is called without one (n_handles = 0): the windows are then counted with the default
mode's geometry, which is that of the lanes `transcribe_files` builds (tests/test_gpu_files_clip_batches.py asks again with a
real handle)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clip_files as CF
import flac_writer as FW
from conftest import ROOT

INV = -1


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


def test_clip_batch_sits_where_reserved_sat_and_nothing_else_moved(lib):
    from basic_pitch_amd import _native

    P = _native.bp_transcribe_params
    # the layout of the struct before the setting had a name: the note parameters, a double, eight 32-bit fields
    before = {"notes": 0, "midi_tempo": 56, "multiple_pitch_bends": 64, "save_midi": 68, "save_notes": 72, "threads": 76,
              "host_decode": 80, "direct_io": 84, "host_flac": 88}
    assert C.sizeof(_native.bp_note_params) == 56 and C.sizeof(P) == 96
    assert {n: getattr(P, n).offset for n in before} == before
    assert P.clip_batch.offset == 92 and P.clip_batch.size == 4 and not hasattr(P, "reserved")
    # the header declares the same fields in the same order, and the limit beside the struct
    header = open(os.path.join(ROOT, "include", "basic_pitch_amd.h")).read()
    body = re.search(r"typedef struct bp_transcribe_params \{(.*?)\} bp_transcribe_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(bp_note_params|double|int32_t)\s+(\w+)\s*;", body)
    ctypes_of = {"bp_note_params": _native.bp_note_params, "double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(P._fields_)
    assert "[" not in body  # no array is left in the struct
    assert re.search(r"#define BP_FILES_CLIP_MAX_WINDOWS (\d+)", header).group(1) == str(_native.BP_FILES_CLIP_MAX_WINDOWS) == "15"
    # what the library itself writes: every byte of the struct, the setting 0
    prm = P()
    C.memset(C.byref(prm), 0xFF, C.sizeof(prm))
    lib.bp_transcribe_params_default(C.byref(prm))
    assert prm.clip_batch == 0 and (prm.midi_tempo, prm.save_midi, prm.save_notes) == (120.0, 1, 1)
    assert (prm.multiple_pitch_bends, prm.threads, prm.host_decode, prm.direct_io, prm.host_flac) == (0, 0, 0, 0, 0)
    raw = bytes(prm)
    assert raw[92:96] == bytes(4) and raw[76:92] == bytes(16)
    # ... and reads: the field at offset 92 is the one the library refuses when negative
    raw = bytearray(raw)
    raw[92:96] = (-1).to_bytes(4, "little", signed=True)
    bad = P.from_buffer_copy(bytes(raw))
    assert bad.clip_batch == -1
    assert CF.probe(lib, [], bad)[0] == INV and b"clip_batch" in lib.bp_files_last_error()
    for name in ("bp_files_batched", "bp_files_batch_probe"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.bp_files_batched() >= 0


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path, written with the tests' own writers."""
    d = tmp_path_factory.mktemp("clip_batches")
    f = {}
    one44 = CF.ONE_WINDOW * 2  # frames at 44,100 Hz that resample to exactly one full window's samples
    f["s16_stereo_44k"] = CF.write_wav(d / "a.wav", CF.tones(one44, 2, 44100, 1), "s16", 44100)
    f["one_frame_more"] = CF.write_wav(d / "a2.wav", CF.tones(one44 + 1, 2, 44100, 1), "s16", 44100)  # two windows: still short
    f["f32_mono_22k"] = CF.write_wav(d / "b.wav", CF.tones(9000, 1, 22050, 2), "f32", 22050)
    f["s24_48k"] = CF.write_wav(d / "c.wav", CF.tones(7000, 2, 48000, 3), "s24", 48000)
    f["u8"] = CF.write_wav(d / "d.wav", CF.tones(5000, 1, 22050, 4), "u8", 22050)
    f["s32"] = CF.write_wav(d / "d32.wav", CF.tones(500, 1, 16000, 4), "s32", 16000)
    f["f64"] = CF.write_wav(d / "d64.wav", CF.tones(500, 3, 96000, 4), "f64", 96000)
    f["zero_frames"] = CF.write_wav(d / "e.wav", np.zeros((0, 2)), "s16", 44100)
    f["15_windows"] = CF.write_wav(d / "f15.wav", np.zeros((CF.MAX_SHORT, 1)), "u8", 22050)
    f["16_windows"] = CF.write_wav(d / "f16.wav", np.zeros((CF.MAX_SHORT + 1, 1)), "u8", 22050)
    f["65_channels"] = CF.write_wav(d / "g.wav", np.zeros((10, 65)), "u8", 22050)
    f["64_channels"] = CF.write_wav(d / "g64.wav", np.zeros((10, 64)), "u8", 22050)
    f["rate_999"] = CF.write_wav(d / "h.wav", np.zeros((10, 1)), "s16", 999)
    f["rate_1000"] = CF.write_wav(d / "h1.wav", np.zeros((10, 1)), "s16", 1000)
    # a LIST chunk between fmt and data, and one behind the samples: the probe walks the chunks as the reader does
    plain = open(f["u8"], "rb").read()
    extra = plain[:36] + b"LIST" + (5).to_bytes(4, "little") + b"abcde\0" + plain[36:] + b"cue " + (4).to_bytes(4, "little") + bytes(4)
    (d / "i.wav").write_bytes(extra)
    f["extra_chunks"] = str(d / "i.wav")
    (d / "j.wav").write_bytes(plain[:36])  # no data chunk
    f["no_data_chunk"] = str(d / "j.wav")
    pcm = np.round(CF.tones(6000, 2, 44100, 5) * 20000).astype(np.int64)
    (d / "k.flac").write_bytes(FW.encode(pcm, 44100, 16, blocksize=1152))
    f["flac"] = str(d / "k.flac")
    (d / "l.flac").write_bytes(FW.encode(pcm, 44100, 16, blocksize=1152, total_in_header=False))
    f["flac_no_total"] = str(d / "l.flac")
    (d / "m.flac").write_bytes(FW.encode(pcm, 44100, 16, blocksize=1152, id3=True))
    f["flac_id3"] = str(d / "m.flac")
    (d / "n.flac").write_bytes(b"fLaC" + bytes(20))
    f["flac_cut_in_metadata"] = str(d / "n.flac")
    (d / "o.txt").write_text("not audio at all\n" * 10)
    f["text"] = str(d / "o.txt")
    (d / "p.wav").write_bytes(b"")
    f["empty"] = str(d / "p.wav")
    f["missing"] = str(d / "nowhere.wav")
    f["directory"] = str(d)
    return f


WANT = {"s16_stereo_44k": 1, "one_frame_more": 1, "f32_mono_22k": 1, "s24_48k": 1, "u8": 1, "s32": 1, "f64": 1, "zero_frames": 1,
        "15_windows": 1, "16_windows": 0, "65_channels": 0, "64_channels": 1, "rate_999": 0, "rate_1000": 1, "extra_chunks": 1,
        "no_data_chunk": "negative", "flac": 2, "flac_no_total": 0, "flac_id3": 2, "flac_cut_in_metadata": "negative",
        "text": "negative", "empty": "negative", "missing": "negative", "directory": "negative"}


def _check(routes, names, want):
    for name, r in zip(names, routes):
        w = want[name]
        assert (r < 0) if w == "negative" else (r == w), (name, r, w)


def test_the_probe_routes_files_by_their_headers(lib, files):
    names = list(files)
    assert set(names) == set(WANT)
    for batch in (1, 4, 5000):  # the value is not looked at beyond its sign
        rc, routes = CF.probe(lib, [files[n] for n in names], CF.params(lib, batch))
        assert rc == 0
        _check(routes, names, WANT)
    # FLAC files the host is asked to decode keep the per-file route; WAV files are not concerned
    rc, routes = CF.probe(lib, [files[n] for n in names], CF.params(lib, 4, host_flac=1))
    assert rc == 0
    _check(routes, names, {**WANT, "flac": 0, "flac_id3": 0, "flac_no_total": 0, "flac_cut_in_metadata": 0})
    # a job whose maps the host decodes batches nothing, and the probe opens no file for it
    for kw in ({"host_decode": 1}, {}):
        prm = CF.params(lib, 4, **kw)
        if not kw:
            prm.notes.onset_threshold = 0.0
        rc, routes = CF.probe(lib, [files[n] for n in names], prm)
        assert rc == 0 and routes == [0] * len(names)


def test_the_probe_reads_headers_only(lib, tmp_path):
    """A WAV file whose header promises three minutes and whose samples were never written (a sparse file of the full length),
    and one truncated behind its header: the route comes from the sizes, as the reader's `what is there` rule has it."""
    head = CF.wav_bytes(b"", "s16", 2, 44100)[:40] + (4 * 44100 * 180).to_bytes(4, "little")
    p = tmp_path / "long.wav"
    with open(p, "wb") as f:
        f.write(head)
        f.truncate(len(head) + 4 * 44100 * 180)
    q = tmp_path / "cut.wav"
    q.write_bytes(head + bytes(4 * 1000))  # the data chunk says 180 s, 1,000 frames are there
    rc, routes = CF.probe(lib, [p, q], CF.params(lib, 4))
    assert rc == 0 and routes == [0, 1]


def test_the_probes_arguments_are_checked(lib, files):
    from basic_pitch_amd import _native

    prm = CF.params(lib, 4)
    assert CF.probe(lib, [files["u8"]], CF.params(lib, -1))[0] == INV and b"negative clip_batch" in lib.bp_files_last_error()
    route = (C.c_int32 * 1)()
    one = (C.c_char_p * 1)(os.fsencode(files["u8"]))
    assert lib.bp_files_batch_probe(None, 0, one, 1, None, route) == INV
    assert lib.bp_files_batch_probe(None, 0, None, 1, C.byref(prm), route) == INV
    assert lib.bp_files_batch_probe(None, 0, one, 1, C.byref(prm), None) == INV
    assert lib.bp_files_batch_probe(None, 0, one, -1, C.byref(prm), route) == INV
    assert lib.bp_files_batch_probe(None, 1, one, 1, C.byref(prm), route) == INV  # a handle is announced, none is given
    assert lib.bp_files_batch_probe(None, 0, one, 0, C.byref(prm), route) == 0
    # the job refuses a negative setting too, before it looks at anything else of the job
    bad = CF.params(lib, -3)
    handle = (C.c_void_p * 1)(1)  # never dereferenced: the refusal comes first
    rep = (_native.bp_file_report * 1)()
    assert lib.bp_transcribe_files(handle, 1, one, 1, os.fsencode(os.path.dirname(files["u8"])), C.byref(bad), rep) == INV
    assert b"negative clip_batch" in lib.bp_files_last_error()
