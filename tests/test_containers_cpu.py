"""AIFF / AIFF-C, CAF, AU and RF64 files, the part that needs no GPU (include/basic_pitch_amd_containers.h): the header
parsers of csrc/pcm_file.cpp against files written by tests/container_files.py, the host decoder against the numpy reader
and the floats the source integers stand for (exact equality throughout), the refusals and their messages, the file job's
probe, and the parsers under the host sanitizers in a program of their own (tools/sanitize/fuzz_containers.cpp).

The writers are cross-checked against the standard library where it still has the modules (aifc, sunau, audioop)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import clip_files as CF
import container_files as K
from conftest import ROOT

BAD_AUDIO = -7
CSRC = os.path.join(ROOT, "basic_pitch_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


def _samples(code, n_frames, channels, seed=0):
    """uint8 bytes of n_frames x channels samples of `code`: every byte value occurs (floats: finite values, some denormal)."""
    rng = np.random.default_rng(1000 * code + seed)
    n = n_frames * channels
    if code in (K.F32, K.F32_BE, K.F64, K.F64_BE):
        x = rng.uniform(-1, 1, n)
        x[::7] *= 1e-41 if K.WIDTH[code] == 4 else 1e-310  # denormals
        x[3::11] = -0.0
        return x.astype({K.F32: "<f4", K.F32_BE: ">f4", K.F64: "<f8", K.F64_BE: ">f8"}[code]).view(np.uint8)
    raw = rng.integers(0, 256, n * K.WIDTH[code], dtype=np.uint8)
    raw[: min(256, raw.size)] = np.arange(min(256, raw.size), dtype=np.uint8)
    return raw


def layout(lib, blob):
    from basic_pitch_amd import _native

    lay = _native.bp_pcm_file_layout()
    rc = lib.bp_pcm_file_layout_of(blob, len(blob), C.byref(lay))
    return rc, lay


def fields(lay):
    return (lay.container, lay.format, lay.channels, lay.sample_rate, lay.bits_per_sample, lay.reserved, lay.n_frames, lay.data_start)


def decode(lib, blob, lay):
    pcm = np.full((lay.n_frames, lay.channels), 7.0, np.float32)
    got = C.c_int64(-1)
    rc = lib.bp_pcm_file_decode(blob, len(blob), pcm.ctypes.data, lay.n_frames, C.byref(got))
    assert rc == 0 and got.value == lay.n_frames, lib.bp_files_last_error()
    return pcm


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the variants: name -> (file bytes, the eight fields, the uint8 samples the file holds) -------------------------------------
def _variants():
    v = {}

    def add(name, blob, container, code, ch, rate, bits, raw, n_frames=None):
        raw = np.frombuffer(raw, np.uint8) if isinstance(raw, bytes) else np.asarray(raw, np.uint8)
        n = raw.size // (K.WIDTH[code] * ch) if n_frames is None else n_frames
        raw = raw[: n * ch * K.WIDTH[code]]
        start = blob.find(raw.tobytes()) if raw.size else None
        v[name] = (blob, (container, code, ch, rate, bits, 0, n), start, raw)

    # AIFF: every integer width, then the knobs
    for code, ch, rate in ((K.S8, 1, 8000), (K.S16_BE, 2, 44100), (K.S24_BE, 2, 48000), (K.S32_BE, 3, 96000)):
        raw = _samples(code, 301, ch)
        add(f"aiff_{code}", K.aiff_of(raw, code, ch, rate), K.AIFF, code, ch, rate, 8 * K.WIDTH[code], raw)
    raw = _samples(K.S16_BE, 77, 2)
    add("aiff_ssnd_first", K.aiff_of(raw, K.S16_BE, 2, 44100, ssnd_first=True), K.AIFF, K.S16_BE, 2, 44100, 16, raw)
    add("aiff_odd_chunk", K.aiff_of(raw, K.S16_BE, 2, 44100, before_ssnd=[(b"NAME", b"abc"), (b"ANNO", b"seven b")]),
        K.AIFF, K.S16_BE, 2, 44100, 16, raw)
    add("aiff_offset", K.aiff_of(raw, K.S16_BE, 2, 22050, ssnd_offset=10), K.AIFF, K.S16_BE, 2, 22050, 16, raw)
    add("aiff_12_bit", K.aiff(raw, 2, 44100, 12), K.AIFF, K.S16_BE, 2, 44100, 12, raw)  # 16-bit words, left-justified
    add("aiff_zero_frames", K.aiff_of(b"", K.S16_BE, 2, 44100), K.AIFF, K.S16_BE, 2, 44100, 16, b"")
    add("aiff_count_too_large", K.aiff_of(raw, K.S16_BE, 2, 44100, comm_frames=5000), K.AIFF, K.S16_BE, 2, 44100, 16, raw)
    add("aiff_count_smaller", K.aiff_of(raw, K.S16_BE, 2, 44100, comm_frames=50), K.AIFF, K.S16_BE, 2, 44100, 16, raw, 50)
    add("aiff_rate_11025", K.aiff_of(raw, K.S16_BE, 1, 11025), K.AIFF, K.S16_BE, 1, 11025, 16, raw)
    # AIFF-C: every compression type; Pascal strings of odd and even length
    for code, ch in ((K.S16, 2), (K.S24, 1), (K.S32, 2), (K.F32_BE, 2), (K.F64_BE, 1), (K.ULAW, 1), (K.ALAW, 2), (K.U8, 1)):
        raw = _samples(code, 300, ch)
        ctype, cbits = K.AIFC_TYPES[code]
        bits = 8 if code in (K.ULAW, K.ALAW) else cbits
        add(f"aifc_{ctype.decode().strip()}_{code}", K.aiff_of(raw, code, ch, 44100), K.AIFF, code, ch, 44100, bits, raw)
    raw = _samples(K.S16_BE, 64, 2)
    for ctype in (b"NONE", b"twos"):
        add(f"aifc_{ctype.decode()}", K.aiff(raw, 2, 44100, 16, ctype), K.AIFF, K.S16_BE, 2, 44100, 16, raw)
    add("aifc_in24", K.aiff(_samples(K.S24_BE, 64, 2), 2, 44100, 24, b"in24"), K.AIFF, K.S24_BE, 2, 44100, 24, _samples(K.S24_BE, 64, 2))
    add("aifc_in32", K.aiff(_samples(K.S32_BE, 64, 2), 2, 44100, 32, b"in32"), K.AIFF, K.S32_BE, 2, 44100, 32, _samples(K.S32_BE, 64, 2))
    add("aifc_FL32", K.aiff(_samples(K.F32_BE, 64, 1), 1, 44100, 32, b"FL32"), K.AIFF, K.F32_BE, 1, 44100, 32, _samples(K.F32_BE, 64, 1))
    add("aifc_ULAW", K.aiff(_samples(K.ULAW, 300, 1), 1, 8000, 16, b"ULAW"), K.AIFF, K.ULAW, 1, 8000, 8, _samples(K.ULAW, 300, 1))
    add("aifc_odd_pascal", K.aiff(raw, 2, 44100, 16, b"NONE", name=b"odd"), K.AIFF, K.S16_BE, 2, 44100, 16, raw)       # 1 + 3 bytes
    add("aifc_even_pascal", K.aiff(raw, 2, 44100, 16, b"NONE", name=b"even"), K.AIFF, K.S16_BE, 2, 44100, 16, raw)     # 1 + 4, padded
    add("aifc_empty_pascal", K.aiff(raw, 2, 44100, 16, b"NONE", name=b""), K.AIFF, K.S16_BE, 2, 44100, 16, raw)
    # CAF: every lpcm form and G.711; a data size of -1; a chunk in between
    for code in K.CAF_FORMATS:
        ch = 1 + code % 3
        raw = _samples(code, 200, ch)
        add(f"caf_{code}", K.caf_of(raw, code, ch, 44100), K.CAF, code, ch, 44100, K.CAF_FORMATS[code][2], raw)
    raw = _samples(K.S16_BE, 99, 2)
    add("caf_to_the_end", K.caf_of(raw, K.S16_BE, 2, 48000, data_size=-1), K.CAF, K.S16_BE, 2, 48000, 16, raw)
    add("caf_free_chunk", K.caf_of(raw, K.S16_BE, 2, 48000, before_data=[(b"free", bytes(13))]), K.CAF, K.S16_BE, 2, 48000, 16, raw)
    add("caf_zero_frames", K.caf_of(b"", K.F32, 2, 48000), K.CAF, K.F32, 2, 48000, 32, b"")
    # AU: every encoding; an annotation with the data size left open
    for code in K.AU_ENCODINGS:
        ch = 1 + code % 2
        raw = _samples(code, 200, ch)
        add(f"au_{code}", K.au_of(raw, code, ch, 8000), K.AU, code, ch, 8000, 8 * K.WIDTH[code], raw)
    raw = _samples(K.ULAW, 500, 1)
    add("au_annotation_open_size", K.au_of(raw, K.ULAW, 1, 8000, annotation=b"recorded somewhere\0\0", data_size=0xFFFFFFFF),
        K.AU, K.ULAW, 1, 8000, 8, raw)
    add("au_size_smaller", K.au_of(raw, K.ULAW, 1, 8000, data_size=100), K.AU, K.ULAW, 1, 8000, 8, raw, 100)
    add("au_zero_frames", K.au_of(b"", K.S16_BE, 2, 44100), K.AU, K.S16_BE, 2, 44100, 16, b"")
    # RF64 / BW64: the sizes live in ds64; plain WAV through the same call
    raw = _samples(K.S16, 333, 2)
    add("rf64", K.rf64_of(raw, K.S16, 2, 44100), K.WAV, K.S16, 2, 44100, 16, raw)
    add("bw64_f32", K.rf64_of(_samples(K.F32, 100, 1), K.F32, 1, 48000, magic=b"BW64"), K.WAV, K.F32, 1, 48000, 32, _samples(K.F32, 100, 1))
    add("wav", K.wav_of(raw, K.S16, 2, 44100), K.WAV, K.S16, 2, 44100, 16, raw)
    return v


VARIANTS = _variants()
REQUIRED = ("aiff_ssnd_first", "aiff_odd_chunk", "aiff_offset", "aiff_12_bit", "aifc_odd_pascal", "caf_to_the_end",
            "au_annotation_open_size", "rf64", "aiff_zero_frames", "aiff_count_too_large")


def test_the_variants_the_parsers_must_cope_with_are_all_here():
    assert set(REQUIRED) <= set(VARIANTS)
    # and the writers did what the names say
    blob = VARIANTS["aiff_ssnd_first"][0]
    assert 0 < blob.find(b"SSND") < blob.find(b"COMM")
    blob = VARIANTS["aiff_odd_chunk"][0]
    assert blob.find(b"NAME\0\0\0\3abc\0ANNO") > 0 and blob.find(b"ANNO") < blob.find(b"SSND")
    assert VARIANTS["aiff_offset"][0].find(b"SSND") > 0 and b"SSND" + (8 + 10 + 77 * 4).to_bytes(4, "big") + (10).to_bytes(4, "big") in VARIANTS["aiff_offset"][0]
    assert b"caff\0\1\0\0desc" in VARIANTS["caf_to_the_end"][0] and b"data" + b"\xff" * 8 in VARIANTS["caf_to_the_end"][0]
    blob = VARIANTS["rf64"][0]
    assert blob[:4] == b"RF64" and blob[4:8] == b"\xff" * 4 and blob[12:16] == b"ds64" and b"data\xff\xff\xff\xff" in blob
    assert int.from_bytes(blob[28:36], "little") == 333 * 4 and int.from_bytes(blob[36:44], "little") == 333


@pytest.mark.parametrize("name", list(VARIANTS))
def test_layout_decode_and_the_numpy_reader_agree(lib, name, tmp_path):
    from basic_pitch_amd import audio

    blob, want, start, raw = VARIANTS[name]
    rc, lay = layout(lib, blob)
    assert rc == 0, lib.bp_files_last_error()
    got = fields(lay)
    assert got[:7] == want, (got, want)
    if start is not None:
        assert lay.data_start == start
        assert blob[lay.data_start : lay.data_start + raw.size] == raw.tobytes()
    assert 0 <= lay.data_start <= len(blob)
    code, ch = want[1], want[2]
    # the host decoder = the floats the source integers stand for = the numpy reader, bit for bit
    expect = K.floats_of(raw, code).reshape(-1, ch)
    assert same_bits(decode(lib, blob, lay), expect)
    p = tmp_path / "f.bin"
    p.write_bytes(blob)
    view, r_code, r_ch, r_rate, r_n = audio.pcm_raw(p)
    assert (r_code, r_ch, r_rate, r_n) == (code, ch, want[3], want[6]) and view.tobytes() == raw.tobytes()
    x, sr = audio.read_audio(p)
    assert sr == want[3] and same_bits(x, expect)
    reader = {K.AIFF: audio.read_aiff, K.CAF: audio.read_caf, K.AU: audio.read_au, K.WAV: audio.read_wav}[want[0]]
    x, sr = reader(p)
    assert sr == want[3] and same_bits(x, expect)
    if want[0] == K.WAV:  # RF64 is a WAV file to the WAV calls too
        c, r, b, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        assert lib.bp_wav_info(blob, len(blob), C.byref(c), C.byref(r), C.byref(b), C.byref(n)) == 0
        assert (c.value, r.value, b.value, n.value) == (ch, want[3], want[4], want[6])
        pcm = np.empty((n.value, ch), np.float32)
        assert lib.bp_wav_decode(blob, len(blob), pcm.ctypes.data, n.value, None) == 0 and same_bits(pcm, expect)


def test_a_file_cut_short_holds_what_is_there(lib):
    for name in ("aiff_6", "caf_6", "au_6", "rf64"):
        blob, want, start, raw = VARIANTS[name]
        frame = K.WIDTH[want[1]] * want[2]
        cut = blob[: start + 10 * frame + 1]  # ten frames and a byte
        rc, lay = layout(lib, cut)
        assert rc == 0 and lay.n_frames == 10 and lay.data_start == start, name
        assert same_bits(decode(lib, cut, lay), K.floats_of(raw[: 10 * frame], want[1]).reshape(-1, want[2]))
    # the buffer's size is checked and the count reported
    blob, want, _, _ = VARIANTS["aiff_6"]
    pcm, n = np.zeros(4, np.float32), C.c_int64()
    assert lib.bp_pcm_file_decode(blob, len(blob), pcm.ctypes.data, 1, C.byref(n)) == -1 and n.value == want[6]
    assert lib.bp_pcm_file_decode(None, 0, pcm.ctypes.data, 1, None) == -1 and lib.bp_pcm_file_layout_of(blob, len(blob), None) == -1


REFUSED, REQUIRED_REFUSALS = K.REFUSED, K.REQUIRED_REFUSALS


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_name_the_fault(lib, name, tmp_path):
    from basic_pitch_amd import audio

    assert set(REQUIRED_REFUSALS) <= set(REFUSED)
    blob, message = REFUSED[name]
    rc, _ = layout(lib, blob)
    assert rc == BAD_AUDIO and re.search(message, lib.bp_files_last_error().decode()), lib.bp_files_last_error()
    pcm = np.zeros(4096, np.float32)
    assert lib.bp_pcm_file_decode(blob, len(blob), pcm.ctypes.data, 1024, None) == BAD_AUDIO
    p = tmp_path / "bad.bin"
    p.write_bytes(blob)
    with pytest.raises(ValueError, match=message):  # the numpy reader says the same
        audio.pcm_raw(p)
    with pytest.raises(ValueError, match=message):
        audio.read_audio(p)


def test_what_is_none_of_the_containers(lib):
    for blob in (b"", b"FORM", b"FORM\0\0\0\4ILBM", b"dns.\0\0\0\x18" + bytes(16), b"riff" + bytes(40), b"not audio at all\n" * 10):
        rc, _ = layout(lib, blob)
        assert rc == BAD_AUDIO and b"not a WAV, AIFF, CAF or AU file" in lib.bp_files_last_error()


# ---- the writers against the standard library, where it still has the modules ----------------------------------------------
def test_g711_formulas_agree_with_audioop_on_all_256_codes():
    from basic_pitch_amd import audio

    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(audio.g711_expand(codes, "ulaw"), K.ULAW_TABLE) and np.array_equal(audio.g711_expand(codes, "alaw"), K.ALAW_TABLE)
    assert (K.ULAW_TABLE.min(), K.ULAW_TABLE.max()) == (-32124, 32124) and (K.ALAW_TABLE.min(), K.ALAW_TABLE.max()) == (-32256, 32256)
    # the encoder by search inverts the expansion (two codes of mu-law expand to 0: the search returns one of them)
    assert np.array_equal(K.ALAW_TABLE[K.g711_compress(K.ALAW_TABLE, K.ALAW_TABLE)], K.ALAW_TABLE)
    assert np.array_equal(K.ULAW_TABLE[K.g711_compress(K.ULAW_TABLE, K.ULAW_TABLE)], K.ULAW_TABLE)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        audioop = pytest.importorskip("audioop")
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), "<i2"), K.ULAW_TABLE)
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes.tobytes(), 2), "<i2"), K.ALAW_TABLE)


def test_the_standard_library_reads_the_aiff_files_back(tmp_path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        aifc = pytest.importorskip("aifc")
    for name in ("aiff_6", "aiff_7", "aiff_ssnd_first", "aiff_odd_chunk", "aifc_NONE", "aifc_odd_pascal", "aifc_ULAW", "aifc_alaw_13"):
        blob, want, _, raw = VARIANTS[name]
        p = tmp_path / (name + ".aif")
        p.write_bytes(blob)
        with aifc.open(str(p), "rb") as f:
            assert (f.getnchannels(), f.getframerate(), f.getnframes()) == (want[2], want[3], want[6]), name
            frames = f.readframes(f.getnframes())
        if want[1] in (K.ULAW, K.ALAW):  # aifc expands G.711 to native 16-bit words
            assert frames == K.plain_bytes(raw, want[1]).tobytes(), name
        else:
            assert frames == raw.tobytes(), name


def test_the_standard_library_reads_the_au_files_back(tmp_path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        sunau = pytest.importorskip("sunau")
    for name in ("au_6", "au_7", "au_8", "au_12", "au_annotation_open_size"):
        blob, want, _, raw = VARIANTS[name]
        p = tmp_path / (name + ".au")
        p.write_bytes(blob)
        with sunau.open(str(p), "rb") as f:
            assert (f.getnchannels(), f.getframerate()) == (want[2], want[3]), name
            frames = f.readframes(want[6])
        if want[1] == K.ULAW:  # sunau expands mu-law
            assert frames == K.plain_bytes(raw, want[1]).tobytes(), name
        else:
            assert frames == raw.tobytes(), name


# ---- the file job's probe: the same function the workers decide with, without handles ----------------------------------------
def test_the_probe_routes_the_new_containers(lib, tmp_path):
    one = CF.ONE_WINDOW  # samples at 22,050 Hz of a one-window file
    files, want = [], []

    def add(name, blob, route):
        p = tmp_path / name
        p.write_bytes(blob)
        files.append(p)
        want.append(route)

    short = K.encode(CF.tones(one, 1, 22050, 1), K.S16_BE)
    add("one.aif", K.aiff_of(short, K.S16_BE, 1, 22050), 1)
    add("one.caf", K.caf_of(short, K.S16_BE, 1, 22050), 1)
    add("one.au", K.au_of(short, K.S16_BE, 1, 22050), 1)
    add("one_rf64.wav", K.rf64_of(K.plain_bytes(short, K.S16_BE), K.S16, 1, 22050), 1)
    add("one_ulaw.aifc", K.aiff_of(K.encode(CF.tones(one, 1, 22050, 2), K.ULAW), K.ULAW, 1, 22050), 1)
    long_ = bytes(CF.MAX_SHORT + 1)  # 16 windows of signed bytes
    add("16.aif", K.aiff_of(long_, K.S8, 1, 22050), 0)
    add("16.caf", K.caf_of(long_, K.S8, 1, 22050), 0)
    add("16.au", K.au_of(long_, K.S8, 1, 22050), 0)
    add("16_rf64.wav", K.rf64_of(long_, K.U8, 1, 22050), 0)
    add("15.au", K.au_of(long_[:-1], K.S8, 1, 22050), 1)
    add("65_channels.au", K.au_of(bytes(650), K.S8, 65, 22050), 0)  # the per-file route reports it
    for name in ("ima4", "caf_two_frames_a_packet", "au_encoding_23", "truncated_comm", "aiff_zero_channels"):
        add("bad_" + name + ".bin", REFUSED[name][0], "negative")
    rc, routes = CF.probe(lib, files, CF.params(lib, 8))
    assert rc == 0
    for p, r, w in zip(files, routes, want):
        assert (r < 0) if w == "negative" else (r == w), (p.name, r, w)
    # the message of a recognised container names what was found; that of a file that is none of them is what it always was
    rc, routes = CF.probe(lib, [files[-5]], CF.params(lib, 8))
    assert routes[0] == BAD_AUDIO and b"compression type 'ima4'" in lib.bp_files_last_error()
    text = tmp_path / "notes.txt"
    text.write_text("not audio at all\n" * 10)
    rc, routes = CF.probe(lib, [text], CF.params(lib, 8))
    assert rc == 0 and routes[0] == BAD_AUDIO
    assert lib.bp_files_last_error() == b"not a WAV or FLAC file (the native pipeline reads RIFF/WAVE and FLAC)"
    # a job whose maps the host decodes batches none of them
    rc, routes = CF.probe(lib, files, CF.params(lib, 8, host_decode=1))
    assert rc == 0 and routes == [0] * len(files)


def test_the_header_the_bindings_and_the_build_list_agree(lib):
    from basic_pitch_amd import _native, build, clips, streaming

    header = open(os.path.join(ROOT, "include", "basic_pitch_amd_containers.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(bp_[a-z_0-9]+)\s*\(", code))
    assert declared == set(_native.CONTAINERS_SYMBOLS) == {"bp_pcm_file_layout_of", "bp_pcm_file_decode"}
    assert not declared & set(_native.EXPORTED_SYMBOLS) and all(hasattr(lib, s) for s in declared)
    body = re.search(r"typedef struct bp_pcm_file_layout \{(.*?)\} bp_pcm_file_layout;", code, flags=re.S).group(1)
    names = [n for _, n in re.findall(r"\b(int32_t|int64_t)\s+(\w+)\s*;", body)]
    assert names == [n for n, _ in _native.bp_pcm_file_layout._fields_] and C.sizeof(_native.bp_pcm_file_layout) == 40
    assert re.search(r"BP_CONTAINER_WAV = 1, BP_CONTAINER_AIFF = 2, BP_CONTAINER_CAF = 3, BP_CONTAINER_AU = 4", code)
    assert (_native.BP_CONTAINER_WAV, _native.BP_CONTAINER_AIFF, _native.BP_CONTAINER_CAF, _native.BP_CONTAINER_AU) == (K.WAV, K.AIFF, K.CAF, K.AU)
    # the fourteen codes: the enum, the Python constants, the widths, the tests' own table
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basic_pitch_amd.h")).read(), flags=re.S)
    enum = dict(re.findall(r"\b(BP_PCM_\w+) = (\d+)", re.search(r"typedef enum bp_pcm_format \{(.*?)\}", main, flags=re.S).group(1)))
    assert len(enum) == 14 and all(getattr(_native, k) == int(v) for k, v in enum.items())
    assert [enum[k] for k in ("BP_PCM_F32", "BP_PCM_S16", "BP_PCM_S24", "BP_PCM_S32", "BP_PCM_U8", "BP_PCM_F64")] == list("012345")
    assert {getattr(_native, "BP_PCM_" + n): getattr(K, n) for n in ("S16_BE", "S24_BE", "S32_BE", "F32_BE", "F64_BE", "S8", "ULAW", "ALAW")} == {c: c for c in range(6, 14)}
    assert _native.BP_PCM_WIDTH == K.WIDTH and set(streaming._DTYPES) == set(K.WIDTH)
    assert all(np.dtype(streaming._DTYPES[c]).itemsize in (1, K.WIDTH[c]) for c in K.WIDTH)
    for t, c in ((">i2", K.S16_BE), (">i4", K.S32_BE), (">f4", K.F32_BE), (">f8", K.F64_BE), ("<i2", K.S16), ("<f4", K.F32)):
        assert clips.FORMATS[np.dtype(t)] == c and clips.as_clip(np.zeros((4, 2), t), 0).dtype == np.dtype(t)
    assert "pcm_file.cpp" in build.SOURCES and "basic_pitch_amd_containers.h" in {os.path.basename(h) for h in build.HEADERS}


# ---- the parsers under the host sanitizers, in a program of their own --------------------------------------------------------
DEVICE_FREE = ("flac_decode.cpp", "note_decode.cpp", "wav_file.cpp", "note_writers.cpp", "file_io.cpp", "pcm_file.cpp")


def _build(out, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "fuzz_containers.cpp")] + [os.path.join(CSRC, s) for s in DEVICE_FREE]
    flags = ["-std=c++17", "-O1", "-pthread", "-w"] + extra
    cmds = [[cxx] + flags + ["-c", src, "-o", out + "." + os.path.basename(src) + ".o"] for src in srcs]
    return cmds, [cxx] + flags + [c[-1] for c in cmds] + ["-o", out]


def _check(cmd):
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_the_parsers_run_clean_under_the_host_sanitizers(tmp_path):
    seeds = tmp_path / "seeds"
    seeds.mkdir()
    for name in ("aiff_7", "aiff_odd_chunk", "aiff_offset", "aifc_ulaw_12", "aifc_sowt_1", "aifc_fl32_9", "aifc_odd_pascal", "caf_6", "caf_0",
                 "caf_to_the_end", "caf_12", "au_6", "au_annotation_open_size", "au_10", "rf64", "bw64_f32", "wav"):
        (seeds / name).write_bytes(VARIANTS[name][0])
    seed_files = sorted(str(p) for p in seeds.iterdir())
    plain, san = str(tmp_path / "fuzz_containers"), str(tmp_path / "fuzz_containers_san")
    builds = [_build(plain, []), _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])]
    with ThreadPoolExecutor(max_workers=min(14, os.cpu_count() or 1)) as pool:
        list(pool.map(_check, [c for compiles, _ in builds for c in compiles]))
        list(pool.map(_check, [link for _, link in builds]))
    syms = subprocess.run(["nm", san], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"

    def run(exe):
        res = subprocess.run([exe, "4000"] + seed_files, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]  # -fno-sanitize-recover: a finding ends the sanitizer build's run
        return res.stdout

    out = run(plain)
    assert run(san) == out
    lines = out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("containers ok "), out
    ok, bad = (int(x) for x in re.match(r"containers ok (\d+) bad (\d+) checksum", lines[0]).groups())
    assert ok > 500 and bad > 500  # the mutations reach both ends
