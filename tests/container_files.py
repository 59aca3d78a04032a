"""Writers of AIFF / AIFF-C, CAF, AU and RF64 files for the container tests: plain `struct` packing from the format
descriptions (Apple's AIFF 1.3 and AIFF-C, Core Audio Format 1.0, the Sun / NeXT audio header, EBU Tech 3306), with the
knobs the parsers must cope with — chunk order, odd-sized chunks, an SSND offset, Pascal strings, `to the end of the file`
sizes.  Also the sample encoders (source integers -> the bytes of each BP_PCM_* code, and the floats they stand for) and
G.711 written as the literal formulas of ITU-T G.711."""
import struct

import numpy as np

# BP_PCM_* (include/basic_pitch_amd.h)
F32, S16, S24, S32, U8, F64, S16_BE, S24_BE, S32_BE, F32_BE, F64_BE, S8, ULAW, ALAW = range(14)
WIDTH = {F32: 4, S16: 2, S24: 3, S32: 4, U8: 1, F64: 8, S16_BE: 2, S24_BE: 3, S32_BE: 4, F32_BE: 4, F64_BE: 8, S8: 1, ULAW: 1, ALAW: 1}
# each new code and the plain code it equals bit for bit on the converted bytes
PLAIN = {S16_BE: S16, S24_BE: S24, S32_BE: S32, F32_BE: F32, F64_BE: F64, S8: U8, ULAW: S16, ALAW: S16}
WAV, AIFF, CAF, AU = 1, 2, 3, 4  # BP_CONTAINER_*


# ---- G.711, one code at a time, as the standard's expansion reads (no numpy: the vectorised forms are checked against these)
def ulaw_value(b):
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return 0x84 - t if u & 0x80 else t - 0x84


def alaw_value(b):
    a = b ^ 0x55
    t, s = (a & 15) << 4, (a >> 4) & 7
    t = t + 8 if s == 0 else t + 0x108 if s == 1 else (t + 0x108) << (s - 1)
    return t if a & 0x80 else -t


ULAW_TABLE = np.array([ulaw_value(b) for b in range(256)], np.int32)
ALAW_TABLE = np.array([alaw_value(b) for b in range(256)], np.int32)


def g711_compress(v, table):
    """The code whose expansion lies nearest to each int value (an encoder by search: all a test needs)."""
    order = np.argsort(table, kind="stable")
    levels = table[order]
    v = np.asarray(v, np.int64)
    k = np.clip(np.searchsorted(levels, v), 1, 255)
    k = np.where(np.abs(levels[k - 1] - v) <= np.abs(levels[k] - v), k - 1, k)
    return order[k].astype(np.uint8)


# ---- samples
def plain_bytes(raw, code):
    """The bytes of the PLAIN twin of `raw` (uint8 array of samples of a new code): swapped words, offset bytes, expanded G.711."""
    raw = np.asarray(raw, np.uint8)
    if code in (S16_BE, S24_BE, S32_BE, F32_BE, F64_BE):
        return np.ascontiguousarray(raw.reshape(-1, WIDTH[code])[:, ::-1]).reshape(-1)
    if code == S8:
        return raw ^ 0x80
    if code in (ULAW, ALAW):
        return (ULAW_TABLE if code == ULAW else ALAW_TABLE)[raw].astype("<i2").view(np.uint8)
    return raw


def floats_of(raw, code):
    """float32 of every sample of `raw`, from the source integers: value / 2^(bits - 1), (v - 128) / 128, expanded / 32768,
    float64 rounded to float32."""
    p, code = plain_bytes(raw, code), PLAIN.get(code, code)
    if code == S16:
        return (p.view("<i2").astype(np.float64) / 32768.0).astype(np.float32)
    if code == S24:
        b = p.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return (np.where(v >= 1 << 23, v - (1 << 24), v) / 8388608.0).astype(np.float32)
    if code == S32:
        return (p.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    if code == U8:
        return ((p.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    if code == F64:
        return p.view("<f8").astype(np.float32)
    return p.view("<f4").copy()


def encode(x, code):
    """Float samples [n, channels] in (-1, 1) as the uint8 bytes a file of sample format `code` stores."""
    x = np.asarray(x, np.float64)
    ints = {S16: ("<i2", 15), S16_BE: (">i2", 15), S32: ("<i4", 31), S32_BE: (">i4", 31)}
    if code in ints:
        t, bits = ints[code]
        return np.clip(np.round(x * (2**bits - 1)), -(2**bits), 2**bits - 1).astype(t).reshape(-1).view(np.uint8)
    if code in (S24, S24_BE):
        b = np.clip(np.round(x * 8388607), -8388608, 8388607).astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b if code == S24 else b[:, ::-1]).reshape(-1)
    if code in (U8, S8):
        return (np.clip(np.round(x * 127), -128, 127).astype(np.int64) + (128 if code == U8 else 0)).astype(np.uint8).reshape(-1)
    if code in (ULAW, ALAW):
        return g711_compress(np.round(x * 32767).reshape(-1), ULAW_TABLE if code == ULAW else ALAW_TABLE)
    t = {F32: "<f4", F32_BE: ">f4", F64: "<f8", F64_BE: ">f8"}[code]
    return x.astype(t).reshape(-1).view(np.uint8)


# ---- AIFF / AIFF-C
def ext80(rate):
    """An integer rate as an 80-bit extended float."""
    if rate == 0:
        return bytes(10)
    e = int(rate).bit_length() - 1
    return struct.pack(">HQ", 16383 + e, int(rate) << (63 - e))


def chunk(cid, body):
    return cid + struct.pack(">I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


# the compression type of each sample format in an AIFF-C file, and its COMM sample size
AIFC_TYPES = {S8: (b"NONE", 8), S16_BE: (b"NONE", 16), S24_BE: (b"NONE", 24), S32_BE: (b"NONE", 32), S16: (b"sowt", 16),
              S24: (b"sowt", 24), S32: (b"sowt", 32), F32_BE: (b"fl32", 32), F64_BE: (b"fl64", 64), ULAW: (b"ulaw", 16),
              ALAW: (b"alaw", 16), U8: (b"raw ", 8)}


def aiff(data, channels, rate, bits, ctype=None, name=b"not compressed", comm_frames=None, ssnd_offset=0, ssnd_first=False,
         before_ssnd=(), comm_bytes=None, width=None):
    """An AIFF (ctype None) or AIFF-C file.  name: the Pascal string behind the type (an even total with its count byte, padded).
    comm_frames: COMM's count if not what `data` holds.  ssnd_offset: bytes of filler in front of the samples.  ssnd_first: SSND
    in front of COMM.  before_ssnd: (id, body) chunks between COMM and SSND.  comm_bytes: cut COMM to this many bytes."""
    data = bytes(data)
    width = width or (1 if ctype in (b"ulaw", b"ULAW", b"alaw", b"ALAW") else (bits + 7) // 8)
    frames = len(data) // (width * max(1, channels)) if comm_frames is None else comm_frames
    comm = struct.pack(">HIH", channels, frames, bits) + ext80(rate)
    if ctype is not None:
        pstr = bytes([len(name)]) + name
        comm += ctype + pstr + (b"\0" if len(pstr) & 1 else b"")
    if comm_bytes is not None:
        comm = comm[:comm_bytes]
    c_comm = chunk(b"COMM", comm)
    c_ssnd = chunk(b"SSND", struct.pack(">II", ssnd_offset, 0) + bytes(ssnd_offset) + data)
    extra = b"".join(chunk(i, b) for i, b in before_ssnd)
    fver = chunk(b"FVER", struct.pack(">I", 0xA2805140)) if ctype is not None else b""
    body = fver + (c_ssnd + extra + c_comm if ssnd_first else c_comm + extra + c_ssnd)
    return b"FORM" + struct.pack(">I", 4 + len(body)) + (b"AIFF" if ctype is None else b"AIFC") + body


def aiff_of(raw, code, channels, rate, **kw):
    """The natural file of samples of `code`: plain AIFF for big-endian integers and signed bytes, AIFF-C for the rest."""
    ctype, bits = AIFC_TYPES[code]
    return aiff(raw, channels, rate, kw.pop("bits", bits), None if ctype == b"NONE" and not kw.pop("aifc", False) else ctype,
                width=WIDTH[code], **kw)


# ---- CAF
CAF_FORMATS = {S8: (b"lpcm", 0, 8), S16_BE: (b"lpcm", 0, 16), S24_BE: (b"lpcm", 0, 24), S32_BE: (b"lpcm", 0, 32),
               S16: (b"lpcm", 2, 16), S24: (b"lpcm", 2, 24), S32: (b"lpcm", 2, 32), F32_BE: (b"lpcm", 1, 32),
               F64_BE: (b"lpcm", 1, 64), F32: (b"lpcm", 3, 32), F64: (b"lpcm", 3, 64), ULAW: (b"ulaw", 0, 8), ALAW: (b"alaw", 0, 8)}


def caf_chunk(cid, body, size=None):
    return cid + struct.pack(">q", len(body) if size is None else size) + body


def caf(data, channels, rate, fmt_id, flags, bits, packet_bytes=None, packet_frames=1, data_size=None, before_data=(), version=1):
    """data_size: the size field of the data chunk if not the true one (-1: to the end of the file)."""
    width = (bits + 7) // 8
    desc = struct.pack(">d4sIIIII", float(rate), fmt_id, flags, channels * width if packet_bytes is None else packet_bytes,
                       packet_frames, channels, bits)
    extra = b"".join(caf_chunk(i, b) for i, b in before_data)
    return (b"caff" + struct.pack(">HH", version, 0) + caf_chunk(b"desc", desc) + extra
            + caf_chunk(b"data", struct.pack(">I", 0) + bytes(data), data_size))


def caf_of(raw, code, channels, rate, **kw):
    fmt_id, flags, bits = CAF_FORMATS[code]
    return caf(raw, channels, rate, fmt_id, flags, bits, **kw)


# ---- AU
AU_ENCODINGS = {ULAW: 1, S8: 2, S16_BE: 3, S24_BE: 4, S32_BE: 5, F32_BE: 6, F64_BE: 7, ALAW: 27}


def au(data, channels, rate, encoding, annotation=b"", data_size=None, header_bytes=None):
    """data_size: the header's if not the true one (0xffffffff: to the end of the file)."""
    data = bytes(data)
    start = 24 + len(annotation)
    return (b".snd" + struct.pack(">IIIII", start if header_bytes is None else header_bytes, len(data) if data_size is None else data_size,
                                  encoding, rate, channels) + annotation + data)


def au_of(raw, code, channels, rate, **kw):
    return au(raw, channels, rate, AU_ENCODINGS[code], **kw)


# ---- RIFF/WAVE and RF64
WAV_TAGS = {U8: (1, 8), S16: (1, 16), S24: (1, 24), S32: (1, 32), F32: (3, 32), F64: (3, 64)}


def _fmt_chunk(code, channels, rate):
    tag, bits = WAV_TAGS[code]
    return struct.pack("<4sIHHIIHH", b"fmt ", 16, tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)


def wav_of(raw, code, channels, rate):
    data = bytes(raw)
    body = _fmt_chunk(code, channels, rate) + struct.pack("<4sI", b"data", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return struct.pack("<4sI4s", b"RIFF", 4 + len(body), b"WAVE") + body


def rf64_of(raw, code, channels, rate, magic=b"RF64"):
    """Every 32-bit size is 0xffffffff; the true ones lie in ds64, the first chunk (EBU Tech 3306)."""
    data = bytes(raw)
    frames = len(data) // (WIDTH[code] * channels)
    tail = _fmt_chunk(code, channels, rate) + struct.pack("<4sI", b"data", 0xFFFFFFFF) + data + (b"\0" if len(data) & 1 else b"")
    ds64 = struct.pack("<4sIQQQI", b"ds64", 28, 4 + 36 + len(tail), len(data), frames, 0)
    return struct.pack("<4sI4s", magic, 0xFFFFFFFF, b"WAVE") + ds64 + tail


def twin_wav(raw, code, channels, rate):
    """The WAV file that holds the same samples as `raw` of `code`: the plain format of the converted bytes."""
    return wav_of(plain_bytes(raw, code), PLAIN.get(code, code), channels, rate)


# ---- files the parsers refuse: name -> (file bytes, what the message must name)
REFUSED = {
    "truncated_comm": (aiff(bytes(40), 2, 44100, 16, comm_bytes=10), r"truncated COMM chunk"),
    "truncated_comm_aifc": (aiff(bytes(40), 2, 44100, 16, b"NONE", comm_bytes=18), r"truncated COMM chunk"),
    "ima4": (aiff(bytes(68), 2, 44100, 16, b"ima4", name=b"IMA 4:1", width=2), r"compression type 'ima4'"),
    "caf_two_frames_a_packet": (caf(bytes(80), 2, 44100, b"lpcm", 0, 16, packet_bytes=8, packet_frames=2), r"packet layout: 2 frames in 8 bytes"),
    "caf_wrong_packet_bytes": (caf(bytes(80), 2, 44100, b"lpcm", 0, 16, packet_bytes=8), r"packet layout: 1 frames in 8 bytes"),
    "caf_aac": (caf(bytes(80), 2, 44100, b"aac ", 0, 0, packet_bytes=0, packet_frames=1024), r"CAF format 'aac '"),
    "caf_version_2": (caf(bytes(80), 2, 44100, b"lpcm", 0, 16, version=2), r"CAF version"),
    "au_encoding_23": (au(bytes(80), 1, 8000, 23), r"AU encoding 23"),
    "au_header_size": (au(bytes(80), 1, 8000, 3, header_bytes=8), r"AU header size 8"),
    "aiff_zero_channels": (aiff(bytes(40), 0, 44100, 16), r"zero channels"),
    "caf_zero_channels": (caf(bytes(40), 0, 44100, b"lpcm", 0, 16), r"zero channels"),
    "au_zero_channels": (au(bytes(40), 0, 8000, 3), r"zero channels"),
    "aiff_no_ssnd": (aiff(bytes(40), 2, 44100, 16).replace(b"SSND", b"JUNK"), r"missing SSND chunk"),
    "aiff_40_bits": (aiff(bytes(40), 1, 44100, 40), r"sample size 40"),
    "aiff_rate_zero": (aiff(bytes(40), 1, 0, 16), r"sample rate"),
}
REQUIRED_REFUSALS = ("truncated_comm", "ima4", "caf_two_frames_a_packet", "au_encoding_23", "aiff_zero_channels")
