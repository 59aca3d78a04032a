"""G.711 and IMA ADPCM files, the part that needs no GPU (include/basic_pitch_amd_adpcm.h): the host decoder of
csrc/adpcm_file.cpp against `audioop.adpcm2lin` sample for sample — per block, from the header's state, on nibble-swapped
bytes (tests/adpcm_files.py) — on encoded two-tone signals and on blocks of random codes that drive the predictor into both
rails; the layout's fields; the frame counts (a fact chunk that cuts the last block, a trailing partial block, a prefix that
ends inside a block); G.711 in RIFF/WAVE against the AU twin on all 256 codes of both laws; the refusals and their messages;
the numpy reader against the native decoder; and the parsers under the host sanitizers in a program of their own
(tools/sanitize/fuzz_adpcm.cpp)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adpcm_files as A
import container_files as K
from conftest import ROOT

BAD_AUDIO, INVALID = -7, -1
CSRC = os.path.join(ROOT, "basic_pitch_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


def layout(lib, blob):
    from basic_pitch_amd import _native

    lay = _native.bp_adpcm_layout()
    rc = lib.bp_adpcm_layout_of(blob, len(blob), C.byref(lay))
    return rc, lay


def decode(lib, blob):
    rc, lay = layout(lib, blob)
    assert rc == 0, lib.bp_files_last_error()
    pcm = np.full((lay.n_frames, lay.channels), 77, np.int16)
    got = C.c_int64(-1)
    rc = lib.bp_adpcm_decode(blob, len(blob), pcm.ctypes.data, lay.n_frames, C.byref(got))
    assert rc == 0 and got.value == lay.n_frames, lib.bp_files_last_error()
    return pcm, lay


def reference(blob, lay):
    """the file's whole blocks through audioop, cut to the layout's frame count"""
    blocks = lay.data_bytes // lay.block_bytes
    data = blob[lay.data_start : lay.data_start + blocks * lay.block_bytes]
    return A.reference_decode(data, lay.codec, lay.channels, lay.block_bytes, lay.n_frames)


def fields(lay):
    return (lay.container, lay.codec, lay.channels, lay.sample_rate, lay.block_bytes, lay.block_frames, lay.n_frames)


# ---- (a) encoded two-tone signals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("block", ["8C", 256, "512C"])
def test_wav_decode_equals_audioop(lib, channels, block):
    B = {"8C": 8 * channels, 256: 256, "512C": 512 * channels}[block]
    bf = A.wav_block_frames(B, channels)
    assert bf == (B - 4 * channels) * 2 // channels + 1 and (block != "8C" or bf == 9)
    n = 5 * bf + bf // 2 + 1  # the last block is cut by the fact chunk
    pcm = A.two_tones(n, channels, 8000, seed=channels)
    blob = A.ima_wav(pcm, 8000, B)
    got, lay = decode(lib, blob)
    assert fields(lay) == (K.WAV, A.IMA_WAV, channels, 8000, B, bf, n)
    assert lay.data_bytes == 6 * B and blob[lay.data_start : lay.data_start + 4 * channels] == A.wav_blocks(pcm, B)[: 4 * channels]
    assert np.array_equal(got, reference(blob, lay))
    # the writer's own sanity (the codec is lossy, the step adapts over the first frames): the decoded signal is the source's
    if n > 500:
        assert np.corrcoef(got[64:].astype(np.float64).ravel(), pcm[64:].astype(np.float64).ravel())[0, 1] > 0.95
    # without a fact chunk: whole blocks; a reader must not need the samples-per-block field either
    for kw in ({"fact": None}, {"fact": None, "samples_field": False}, {"extensible": True}, {"rf64": True}):
        blob2 = A.ima_wav(pcm, 8000, B, **kw)
        got2, lay2 = decode(lib, blob2)
        want_n = 6 * bf if kw.get("fact", 1) is None else n
        assert fields(lay2) == (K.WAV, A.IMA_WAV, channels, 8000, B, bf, want_n), kw
        assert np.array_equal(got2[:n], got) and np.array_equal(got2, reference(blob2, lay2))


@pytest.mark.parametrize("channels", [1, 2])
def test_caf_decode_equals_audioop(lib, channels):
    n = 64 * 7 + 13  # the pakt chunk's valid frames cut the last packet
    pcm = A.two_tones(n, channels, 22050, seed=3)
    blob = A.ima4_caf(pcm, 22050)
    got, lay = decode(lib, blob)
    assert fields(lay) == (K.CAF, A.IMA4, channels, 22050, 34 * channels, 64, n) and lay.data_bytes == 8 * 34 * channels
    assert np.array_equal(got, reference(blob, lay))
    assert np.corrcoef(got[64:].astype(np.float64).ravel(), pcm[64:].astype(np.float64).ravel())[0, 1] > 0.95
    for kw, want_n in (({"pakt": False}, 8 * 64), ({"data_size": -1}, n), ({"valid_frames": 10 ** 9}, 8 * 64)):
        blob2 = A.ima4_caf(pcm, 22050, **kw)
        got2, lay2 = decode(lib, blob2)
        assert lay2.n_frames == want_n and np.array_equal(got2[:n], got) and np.array_equal(got2, reference(blob2, lay2)), kw


# ---- (b) random codes under headers at the rails, indices 0, 40, 88 and 200 --------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_random_codes_clamp_at_both_rails(lib, channels):
    blocks, B = A.random_wav_blocks(channels)
    blob = A.ima_wav_of(blocks, channels, 44100, B)
    got, lay = decode(lib, blob)
    assert lay.n_frames == len(A.HEADER_STATES) * A.wav_block_frames(B, channels)
    want = reference(blob, lay)
    assert np.array_equal(got, want)
    assert (got == 32767).sum() > 500 and (got == -32768).sum() > 500  # both rails, many times
    packets = A.random_ima4_packets(channels)
    blob = A.ima4_caf_of(packets, channels, 44100)
    got, lay = decode(lib, blob)
    assert lay.n_frames == 40 * 64 and np.array_equal(got, reference(blob, lay))


# ---- frame counts -------------------------------------------------------------------------------------------------------------------
def test_partial_blocks_prefixes_and_small_buffers(lib):
    ch, B = 2, 256
    bf = A.wav_block_frames(B, ch)
    pcm = A.two_tones(4 * bf, ch, 16000)
    blocks = A.wav_blocks(pcm, B)
    whole = A.ima_wav_of(blocks, ch, 16000, B)
    full, lay0 = decode(lib, whole)
    assert lay0.n_frames == 4 * bf
    # a trailing partial block is dropped (with or without a fact chunk that counts it)
    for fact in (None, 4 * bf + 50):
        blob = A.ima_wav_of(blocks, ch, 16000, B, fact=fact, tail=blocks[:100])
        got, lay = decode(lib, blob)
        assert lay.n_frames == 4 * bf and lay.data_bytes == 4 * B + 100 and np.array_equal(got, full)
    # a prefix that ends inside the third block: two blocks
    cut = whole[: lay0.data_start + 2 * B + 77]
    got, lay = decode(lib, cut)
    assert lay.n_frames == 2 * bf and lay.data_start == lay0.data_start and np.array_equal(got, full[: 2 * bf])
    # a prefix that holds the headers alone
    rc, lay = layout(lib, whole[: lay0.data_start])
    assert rc == 0 and lay.n_frames == 0 and lay.data_bytes == 0
    # a fact count of zero; a file without blocks
    got, lay = decode(lib, A.ima_wav_of(blocks, ch, 16000, B, fact=0))
    assert lay.n_frames == 0 and got.shape == (0, ch)
    got, lay = decode(lib, A.ima_wav_of(b"", ch, 16000, B, fact=0))
    assert lay.n_frames == 0
    # CAF: a prefix inside a packet
    caf = A.ima4_caf(pcm[:300], 16000)
    full_c, lay_c = decode(lib, caf)
    cut = caf[: lay_c.data_start + 2 * 68 + 5]
    got, lay = decode(lib, cut)
    assert lay.n_frames == 128 and np.array_equal(got, full_c[:128])
    # the buffer's size is checked and the count reported; null pointers
    pcm16, n = np.zeros(8, np.int16), C.c_int64()
    assert lib.bp_adpcm_decode(whole, len(whole), pcm16.ctypes.data, 3, C.byref(n)) == INVALID and n.value == 4 * bf
    assert b"buffer too small" in lib.bp_files_last_error()
    assert lib.bp_adpcm_decode(None, 0, pcm16.ctypes.data, 3, None) == INVALID
    assert lib.bp_adpcm_layout_of(whole, len(whole), None) == INVALID


def test_wav_info_and_decode_take_ima(lib):
    pcm = A.two_tones(700, 2, 11025)
    blob = A.ima_wav(pcm, 11025, 256)
    want, lay = decode(lib, blob)
    c, r, b, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    assert lib.bp_wav_info(blob, len(blob), C.byref(c), C.byref(r), C.byref(b), C.byref(n)) == 0
    assert (c.value, r.value, b.value, n.value) == (2, 11025, 4, 700)
    x = np.empty((700, 2), np.float32)
    assert lib.bp_wav_decode(blob, len(blob), x.ctypes.data, 700, None) == 0
    assert np.array_equal(x, want.astype(np.float32) * np.float32(1 / 32768))
    # the PCM layout call has no sample format for blocks and says where to go
    from basic_pitch_amd import _native

    play = _native.bp_pcm_file_layout()
    assert lib.bp_pcm_file_layout_of(blob, len(blob), C.byref(play)) == BAD_AUDIO and b"bp_adpcm_layout_of" in lib.bp_files_last_error()


# ---- G.711 in RIFF/WAVE ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["ulaw", "alaw"])
@pytest.mark.parametrize("form", ["plain", "extensible", "rf64"])
def test_g711_wav_equals_the_au_twin_on_all_codes(lib, law, form, tmp_path):
    from basic_pitch_amd import _native, audio

    code = K.ULAW if law == "ulaw" else K.ALAW
    codes = np.concatenate([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1, dtype=np.uint8)])  # 256 frames of 2 channels
    wav = A.g711_wav(codes, law, 2, 8000, extensible=form == "extensible", rf64=form == "rf64")
    au = K.au_of(codes, code, 2, 8000)
    c, r, b, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    assert lib.bp_wav_info(wav, len(wav), C.byref(c), C.byref(r), C.byref(b), C.byref(n)) == 0, lib.bp_files_last_error()
    assert (c.value, r.value, b.value, n.value) == (2, 8000, 8, 256)
    x, y = np.empty((256, 2), np.float32), np.empty((256, 2), np.float32)
    assert lib.bp_wav_decode(wav, len(wav), x.ctypes.data, 256, None) == 0
    assert lib.bp_pcm_file_decode(au, len(au), y.ctypes.data, 256, None) == 0
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    table = K.ULAW_TABLE if law == "ulaw" else K.ALAW_TABLE
    assert np.array_equal(x.reshape(-1), table[codes].astype(np.float32) / np.float32(32768))
    lay = _native.bp_pcm_file_layout()
    assert lib.bp_pcm_file_layout_of(wav, len(wav), C.byref(lay)) == 0
    assert (lay.container, lay.format, lay.channels, lay.sample_rate, lay.bits_per_sample, lay.n_frames) == (K.WAV, code, 2, 8000, 8, 256)
    assert wav[lay.data_start : lay.data_start + 512] == codes.tobytes()
    # the numpy reader and the raw route say the same
    p = tmp_path / "g711.wav"
    p.write_bytes(wav)
    raw, r_code, r_ch, r_rate, r_n = audio.pcm_raw(p)
    assert (r_code, r_ch, r_rate, r_n) == (code, 2, 8000, 256) and raw.tobytes() == codes.tobytes()
    z, sr = audio.read_audio(p)
    assert sr == 8000 and np.array_equal(z.view(np.uint32), y.view(np.uint32))
    # 16-bit "G.711" is no such thing
    bad = bytearray(A.g711_wav(codes, law, 2, 8000))
    bad[34:36] = struct.pack("<H", 16)
    assert lib.bp_wav_info(bytes(bad), len(bad), None, None, None, None) == BAD_AUDIO
    assert b"unsupported WAV format tag %d" % (7 if law == "ulaw" else 6) in lib.bp_files_last_error()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refused():
    pcm = A.two_tones(400, 2, 8000)
    blocks = A.wav_blocks(pcm, 256)
    packets = A.ima4_packets(pcm)
    return {
        "block_align_not_whole_groups": (A.ima_wav_of(blocks, 2, 8000, 260, fact=400), r"block align 260 for 2 channels"),
        "block_align_headers_only": (A.ima_wav_of(blocks, 2, 8000, 8, fact=400), r"block align 8 for 2 channels"),
        "block_align_zero": (A.ima_wav_of(blocks, 2, 8000, 0, fact=400), r"block align 0 for 2 channels"),
        "three_bit_ima": (A.ima_wav_of(blocks, 2, 8000, 256, fact=400, bits=3), r"IMA ADPCM sample size 3"),
        "five_bit_ima": (A.ima_wav_of(blocks, 2, 8000, 256, fact=400, bits=5), r"IMA ADPCM sample size 5"),
        "wav_zero_channels": (A.ima_wav_of(blocks, 0, 8000, 256, fact=400), r"zero channels"),
        "caf_two_frames_a_packet": (A.ima4_caf_of(packets, 2, 8000, packet_frames=2), r"ima4 packet layout: 2 frames in 68 bytes"),
        "caf_wrong_packet_bytes": (A.ima4_caf_of(packets, 2, 8000, packet_bytes=34), r"ima4 packet layout: 64 frames in 34 bytes"),
        "caf_priming": (A.ima4_caf_of(packets, 2, 8000, valid_frames=300, priming=64), r"pakt chunk: 64 priming frames"),
        "caf_zero_channels": (A.ima4_caf_of(packets, 0, 8000), r"zero channels"),
    }


REFUSED = _refused()


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_name_the_fault(lib, name, tmp_path):
    from basic_pitch_amd import audio

    blob, message = REFUSED[name]
    rc, _ = layout(lib, blob)
    assert rc == BAD_AUDIO and re.search(message, lib.bp_files_last_error().decode()), lib.bp_files_last_error()
    pcm = np.zeros(4096, np.int16)
    assert lib.bp_adpcm_decode(blob, len(blob), pcm.ctypes.data, 1024, None) == BAD_AUDIO
    if blob[:4] == b"RIFF":  # the WAV calls say the same
        assert lib.bp_wav_info(blob, len(blob), None, None, None, None) == BAD_AUDIO
        assert re.search(message, lib.bp_files_last_error().decode())
    p = tmp_path / "bad.bin"
    p.write_bytes(blob)
    with pytest.raises(ValueError, match=message):  # the numpy reader too
        audio.read_audio(p)


def test_what_stays_refused_with_the_words_it_had(lib):
    ms_adpcm = struct.pack("<4sI4s4sIHHIIHHH4sI", b"RIFF", 38 + 64, b"WAVE", b"fmt ", 18, 2, 1, 8000, 4096, 256, 4, 0, b"data", 64) + bytes(64)
    for blob, call_message, adpcm_message in (
        (ms_adpcm, b"unsupported WAV format tag 2", b"not an IMA ADPCM file"),
        (K.REFUSED["ima4"][0], b"unsupported AIFF-C compression type 'ima4'", b"not an IMA ADPCM file"),
        (K.REFUSED["caf_aac"][0], b"unsupported CAF format 'aac '", b"not an IMA ADPCM file"),
        (K.REFUSED["au_encoding_23"][0], b"unsupported AU encoding 23", b"not an IMA ADPCM file"),
    ):
        from basic_pitch_amd import _native

        play = _native.bp_pcm_file_layout()
        assert lib.bp_pcm_file_layout_of(blob, len(blob), C.byref(play)) == BAD_AUDIO and call_message in lib.bp_files_last_error()
        rc, _ = layout(lib, blob)
        assert rc == BAD_AUDIO and adpcm_message in lib.bp_files_last_error()
    assert lib.bp_wav_info(ms_adpcm, len(ms_adpcm), None, None, None, None) == BAD_AUDIO
    assert lib.bp_files_last_error() == b"unsupported WAV format tag 2"
    # a plain PCM file is no IMA ADPCM file either
    rc, _ = layout(lib, K.wav_of(bytes(64), K.S16, 2, 44100))
    assert rc == BAD_AUDIO and b"not an IMA ADPCM file" in lib.bp_files_last_error()


# ---- the numpy reader ------------------------------------------------------------------------------------------------------------------
def test_the_numpy_reader_equals_the_native_decoder(lib, tmp_path):
    from basic_pitch_amd import audio

    files = {
        "mono.wav": A.ima_wav(A.two_tones(1000, 1, 8000), 8000, 256),
        "stereo.wav": A.ima_wav(A.two_tones(1000, 2, 44100), 44100, 2048),
        "ext.wav": A.ima_wav(A.two_tones(100, 2, 44100), 44100, 16, extensible=True),
        "rf64.wav": A.ima_wav(A.two_tones(100, 1, 44100), 44100, 8, rf64=True),
        "random.wav": A.ima_wav_of(A.random_wav_blocks(2, 512)[0], 2, 22050, A.random_wav_blocks(2, 512)[1]),
        "tail.wav": A.ima_wav_of(A.wav_blocks(A.two_tones(505, 1, 8000), 256), 1, 8000, 256, fact=None, tail=bytes(99)),
        "stereo.caf": A.ima4_caf(A.two_tones(1000, 2, 22050), 22050),
        "random.caf": A.ima4_caf_of(A.random_ima4_packets(1), 1, 8000, pakt=False),
        "empty.caf": A.ima4_caf(np.zeros((0, 2), np.int16), 22050),
    }
    for name, blob in files.items():
        p = tmp_path / name
        p.write_bytes(blob)
        want, lay = decode(lib, blob)
        assert audio.is_adpcm_file(p)
        blocks, codec, ch, sr, block_bytes, block_frames, n = audio.adpcm_raw(p)
        assert (codec, ch, sr, block_bytes, block_frames, n) == fields(lay)[1:], name
        assert blocks.tobytes() == blob[lay.data_start : lay.data_start + lay.data_bytes // lay.block_bytes * lay.block_bytes]
        assert np.array_equal(audio.ima_decode(blocks, codec, ch, block_bytes, n), want), name
        x, rate = audio.read_audio(p)
        assert rate == lay.sample_rate and x.dtype == np.float32 and np.array_equal(x, want.astype(np.float32) / np.float32(32768)), name
    for blob in (K.wav_of(bytes(64), K.S16, 2, 44100), K.caf_of(bytes(64), K.S16_BE, 2, 44100), K.au_of(bytes(64), K.ULAW, 1, 8000)):
        p = tmp_path / "pcm.bin"
        p.write_bytes(blob)
        assert not audio.is_adpcm_file(p) and audio.adpcm_raw(p) is None


# ---- the header, the bindings and the build list ------------------------------------------------------------------------------------
def test_the_header_the_bindings_and_the_build_list_agree(lib):
    from basic_pitch_amd import _native, build

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_adpcm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", code))
    assert declared == set(_native.ADPCM_SYMBOLS) and all(hasattr(lib, s) for s in declared)
    others = set(_native.EXPORTED_SYMBOLS) | set(_native.CONTAINERS_SYMBOLS) | set(_native.EVENTS_SYMBOLS) | set(_native.FLAC_CLIPS_SYMBOLS)
    assert not declared & others
    body = re.search(r"typedef struct bp_adpcm_layout \{(.*?)\} bp_adpcm_layout;", code, flags=re.S).group(1)
    names = [n for _, n in re.findall(r"\b(int32_t|int64_t)\s+(\w+)\s*;", body)]
    assert names == [n for n, _ in _native.bp_adpcm_layout._fields_] and C.sizeof(_native.bp_adpcm_layout) == 48
    assert re.search(r"BP_ADPCM_IMA_WAV = 1, BP_ADPCM_IMA4 = 2", code)
    assert (_native.BP_ADPCM_IMA_WAV, _native.BP_ADPCM_IMA4) == (A.IMA_WAV, A.IMA4)
    assert {"adpcm_file.cpp", "adpcm_device.hip"} <= set(build.SOURCES)
    assert {"basic_pitch_amd_adpcm.h", "adpcm_host.h"} <= {os.path.basename(h) for h in build.HEADERS}
    assert _native.BP_PCM_WAV[_native.BP_PCM_ULAW] == (7, 8) and _native.BP_PCM_WAV[_native.BP_PCM_ALAW] == (6, 8)


# ---- the parsers under the host sanitizers, in a program of their own --------------------------------------------------------------
HOST_SOURCES = ("adpcm_file.cpp", "wav_file.cpp", "pcm_file.cpp", "file_io.cpp")


def _build(out, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "fuzz_adpcm.cpp")] + [os.path.join(CSRC, s) for s in HOST_SOURCES]
    flags = ["-std=c++17", "-O1", "-pthread", "-w"] + extra
    cmds = [[cxx] + flags + ["-c", src, "-o", out + "." + os.path.basename(src) + ".o"] for src in srcs]
    return cmds, [cxx] + flags + [c[-1] for c in cmds] + ["-o", out]


def _check(cmd):
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_the_parsers_run_clean_under_the_host_sanitizers(tmp_path):
    seeds = tmp_path / "seeds"
    seeds.mkdir()
    pcm = A.two_tones(150, 2, 8000)
    files = {
        "ima.wav": A.ima_wav(pcm, 8000, 16),
        "ima_ext.wav": A.ima_wav(pcm[:, :1], 8000, 8, extensible=True),
        "ima_rf64.wav": A.ima_wav(pcm, 8000, 24, rf64=True),
        "ima4.caf": A.ima4_caf(pcm, 8000),
        "ulaw.wav": A.g711_wav(bytes(range(256)), "ulaw", 2, 8000),
        "alaw_rf64.wav": A.g711_wav(bytes(range(256)), "alaw", 1, 8000, rf64=True),
    }
    for name, blob in files.items():
        (seeds / name).write_bytes(blob)
    seed_files = sorted(str(p) for p in seeds.iterdir())
    plain, san = str(tmp_path / "fuzz_adpcm"), str(tmp_path / "fuzz_adpcm_san")
    builds = [_build(plain, []), _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])]
    with ThreadPoolExecutor(max_workers=min(10, os.cpu_count() or 1)) as pool:
        list(pool.map(_check, [c for compiles, _ in builds for c in compiles]))
        list(pool.map(_check, [link for _, link in builds]))
    syms = subprocess.run(["nm", san], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"

    def run(exe):
        res = subprocess.run([exe] + seed_files, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]  # -fno-sanitize-recover: a finding ends the sanitizer build's run
        return res.stdout

    out = run(plain)
    assert run(san) == out
    lines = out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("adpcm ok "), out
    ok, bad = (int(x) for x in re.match(r"adpcm ok (\d+) bad (\d+) checksum", lines[0]).groups())
    assert ok > 500 and bad > 500  # prefixes and extreme fields reach both ends
