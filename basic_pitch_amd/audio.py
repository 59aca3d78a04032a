"""Audio ingest for the hot path: decode -> mono -> 22.05 kHz float32.

Stands in for `librosa.load(path, sr=22050, mono=True)` at basic_pitch/inference.py:239 (librosa is
a third-party dependency of the reference and is not available here).  Downmix is the channel mean
like librosa's `to_mono`.  Resampling follows the design of librosa's default `res_type="soxr_hq"`
(libsoxr at SOXR_HQ: linear phase, pass-band to 0.9136 of the lower Nyquist, stop-band from that
Nyquist, 126 dB, Kaiser-windowed sinc — 389 taps at the input rate for 2 : 1): with it the reference's
golden posteriorgrams for its 44.1 kHz clip are reproduced inside its own atol = 1e-4.
The same design runs on the device (csrc/audio_ingest.hip); this host copy serves the per-window
path and checks the device one.
"""
from __future__ import annotations

import math
import pathlib
import struct
from fractions import Fraction
from typing import Tuple, Union

import numpy as np

from . import _native as _n

AUDIO_SAMPLE_RATE = 22050


WAV_TAG_IMA = 0x11  # IMA / DVI ADPCM: blocks, not samples (`adpcm_raw`, `ima_decode`)


def _wav_chunks(path: Union[str, pathlib.Path]):
    """The chunk walk of a RIFF/WAVE file (RF64 / BW64 too): (view of the data chunk, format tag, bits, channels, sample_rate,
    block align, the fact chunk's sample count or None)."""
    with open(path, "rb") as f:
        data = memoryview(f.read())  # chunks below are views, not copies (a 3-minute stereo file is 31 MB)
    rf64 = len(data) >= 4 and bytes(data[:4]) in (b"RF64", b"BW64")
    if len(data) < 12 or not (rf64 or data[:4] == b"RIFF") or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos = 12
    fmt = None
    pcm = None
    ds64_data = None
    fact = None
    while pos + 8 <= len(data):
        cid = bytes(data[pos : pos + 4])
        size = struct.unpack_from("<I", data, pos + 4)[0]
        if rf64 and cid == b"data" and size == 0xFFFFFFFF and ds64_data is not None:
            size = ds64_data
        body = data[pos + 8 : pos + 8 + size]
        if rf64 and cid == b"ds64" and len(body) >= 24:
            ds64_data = struct.unpack_from("<Q", body, 8)[0]
        if cid == b"fmt ":
            tag, ch, sr, _br, align, bits = struct.unpack_from("<HHIIHH", body, 0)
            if tag == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: real tag in the GUID
                tag = struct.unpack_from("<H", body, 24)[0]
            fmt = (tag, ch, sr, bits, align)
        elif cid == b"data":
            pcm = body
        elif cid == b"fact" and len(body) >= 4:
            fact = struct.unpack_from("<I", body, 0)[0]
            fact = None if fact == 0xFFFFFFFF else fact
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, ch, sr, bits, align = fmt
    return pcm, tag, bits, ch, sr, align, fact


def wav_raw(path: Union[str, pathlib.Path]):
    """The samples of a RIFF/WAVE file as the file stores them: (uint8 view of the data chunk, format tag, bits, channels,
    sample_rate).  Tag 1 = integer PCM (8 / 16 / 24 / 32 bits), 3 = IEEE float (32 / 64), 7 / 6 = G.711 mu-law / A-law (8).
    RF64 / BW64 files, whose data size lies in the ds64 chunk, are WAV files here.  IMA ADPCM (tag 0x11) is not samples but
    blocks: `adpcm_raw`."""
    return _wav_pcm(path, _wav_chunks(path))


def _wav_pcm(path, chunks):
    pcm, tag, bits, ch, sr, _align, _fact = chunks
    if tag == WAV_TAG_IMA:
        raise ValueError(f"{path}: IMA ADPCM samples are blocks, not PCM (audio.adpcm_raw reads the file)")
    if not ((tag == 1 and bits in (8, 16, 24, 32)) or (tag == 3 and bits in (32, 64)) or (tag in (6, 7) and bits == 8)):
        raise ValueError(f"{path}: unsupported PCM bit depth {bits}" if tag == 1 else f"{path}: unsupported WAV format tag {tag}")
    if ch < 1:
        raise ValueError(f"{path}: zero channels")
    return pcm, tag, bits, ch, sr


_IMA_STEP = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130,
    143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282,
    1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630,
    9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], dtype=np.int32)
_IMA_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8], dtype=np.int32)


def is_adpcm_file(path: Union[str, pathlib.Path]) -> bool:
    """Whether the format chunk of a RIFF/WAVE (RF64 / BW64) or CAF file says IMA ADPCM: tag 0x11, or `ima4`.  Reads the
    chunk heads up to that chunk, nothing else."""
    with open(path, "rb") as f:
        head = f.read(12)
        if head[:4] == b"caff":
            f.seek(8)
            while True:
                h = f.read(12)
                if len(h) < 12:
                    return False
                size = struct.unpack(">q", h[4:])[0]
                if h[:4] == b"desc":
                    return f.read(12)[8:12] == b"ima4"
                if size < 0:
                    return False
                f.seek(size, 1)
        if head[:4] not in (b"RIFF", b"RF64", b"BW64") or head[8:12] != b"WAVE":
            return False
        while True:
            h = f.read(8)
            if len(h) < 8:
                return False
            size = struct.unpack("<I", h[4:])[0]
            if h[:4] == b"fmt ":
                body = f.read(min(size, 26))
                if len(body) < 16:
                    return False
                tag = struct.unpack_from("<H", body, 0)[0]
                if tag == 0xFFFE and len(body) >= 26:
                    tag = struct.unpack_from("<H", body, 24)[0]
                return tag == WAV_TAG_IMA
            if h[:4] == b"data":  # (a data chunk of 0xffffffff bytes in front of the format: not walked)
                return False
            f.seek(size + (size & 1), 1)


def adpcm_raw(path: Union[str, pathlib.Path]):
    """The blocks of an IMA ADPCM file as the file stores them, or None for a file that is something else: (uint8 view of the
    whole blocks, codec BP_ADPCM_IMA_WAV | BP_ADPCM_IMA4, channels, sample_rate, block_bytes, block_frames, n_frames).  RIFF/WAVE
    format tag 0x11 (plain, EXTENSIBLE, RF64 / BW64) and CAF `ima4`; the layouts are those of
    include/basic_pitch_amd_adpcm.h, independent of the C++ parser (csrc/adpcm_file.cpp), which the tests hold to it."""
    with open(path, "rb") as f:
        head = f.read(12)
    if head[:4] in (b"RIFF", b"RF64", b"BW64") and head[8:12] == b"WAVE":
        try:
            pcm, tag, bits, ch, sr, align, fact = _wav_chunks(path)
        except ValueError:
            return None
        if tag != WAV_TAG_IMA:
            return None
        if bits != 4:
            raise ValueError(f"{path}: unsupported IMA ADPCM sample size {bits} (4 bits a sample are read)")
        if ch < 1:
            raise ValueError(f"{path}: zero channels")
        payload = align - 4 * ch
        if payload <= 0 or payload % (4 * ch):
            raise ValueError(f"{path}: unsupported IMA ADPCM block align {align} for {ch} channels (4 header bytes and whole "
                             "groups of 4 bytes a channel are read)")
        block_frames = payload * 2 // ch + 1
        blocks = len(pcm) // align
        n = blocks * block_frames if fact is None else min(fact, blocks * block_frames)
        return np.frombuffer(pcm, dtype=np.uint8)[: blocks * align], _n.BP_ADPCM_IMA_WAV, ch, sr, align, block_frames, n
    if head[:4] != b"caff":
        return None
    with open(path, "rb") as f:
        data = memoryview(f.read())
    if len(data) < 8 or struct.unpack_from(">H", data, 4)[0] != 1:
        return None
    desc = pcm = pakt = None
    pos = 8
    while pos + 12 <= len(data):
        cid = bytes(data[pos : pos + 4])
        size = struct.unpack_from(">q", data, pos + 4)[0]
        rest = len(data) - (pos + 12)
        body = data[pos + 12 : pos + 12 + (rest if size < 0 else min(size, rest))]
        if cid == b"desc" and len(body) >= 32:
            desc = struct.unpack_from(">d4sIIIII", body, 0)
        elif cid == b"pakt" and len(body) >= 24:
            pakt = struct.unpack_from(">qqii", body, 0)
        elif cid == b"data":
            pcm = body[4:]
        if size < 0:
            break
        pos += 12 + size
    if desc is None or desc[1] != b"ima4":
        return None
    if pcm is None:
        raise ValueError(f"{path}: missing desc or data chunk")
    rate, _fid, _flags, packet_bytes, packet_frames, ch, _bits = desc
    if ch < 1:
        raise ValueError(f"{path}: zero channels")
    if packet_frames != 64 or packet_bytes != 34 * ch:
        raise ValueError(f"{path}: unsupported CAF ima4 packet layout: {packet_frames} frames in {packet_bytes} bytes a packet "
                         f"(read: 64 frames in {34 * ch} bytes)")
    packets = len(pcm) // (34 * ch)
    n = packets * 64
    if pakt is not None:
        if pakt[2] != 0:
            raise ValueError(f"{path}: unsupported CAF pakt chunk: {pakt[2]} priming frames (read: 0)")
        if 0 <= pakt[1] < n:
            n = pakt[1]
    return np.frombuffer(pcm, dtype=np.uint8)[: packets * 34 * ch], _n.BP_ADPCM_IMA4, ch, _rate(path, rate), 34 * ch, 64, n


def ima_decode(blocks: np.ndarray, codec: int, channels: int, block_bytes: int, n_frames: int) -> np.ndarray:
    """The whole blocks `adpcm_raw` returns -> int16 [n_frames, channels].  The chains (one channel of one block) run side by
    side in numpy, a chain's codes one after the other: d = s>>3 (+ s, + s>>1, + s>>2 by the code's bits 2, 1, 0), subtracted
    for bit 3, the predictor clamped to int16, the index moved by {-1, -1, -1, -1, 2, 4, 6, 8} and clamped to 0 ... 88."""
    ch = int(channels)
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, block_bytes)
    nb = b.shape[0]
    if nb == 0 or n_frames <= 0:
        return np.zeros((0, ch), np.int16)
    if codec == _n.BP_ADPCM_IMA_WAV:
        hdr = b[:, : 4 * ch].reshape(nb, ch, 4)
        pred = (hdr[:, :, 0].astype(np.int32) | (hdr[:, :, 1].astype(np.int32) << 8)).astype(np.uint16).view(np.int16).astype(np.int32)
        index = np.minimum(hdr[:, :, 2].astype(np.int32), 88)
        codes = b[:, 4 * ch :].reshape(nb, -1, ch, 4).transpose(0, 2, 1, 3).reshape(nb, ch, -1)  # [block][channel][byte]
        first = [pred.copy()]
    else:
        sub = b.reshape(nb, ch, 34)
        h = (sub[:, :, 0].astype(np.int32) << 8) | sub[:, :, 1].astype(np.int32)
        pred = (h & 0xFF80).astype(np.uint16).view(np.int16).astype(np.int32)
        index = np.minimum(h & 0x7F, 88)
        codes = sub[:, :, 2:]
        first = []
    nib = np.stack([codes & 15, codes >> 4], axis=-1).reshape(nb, ch, -1).astype(np.int32)  # low nibble first
    out = first
    for k in range(nib.shape[2]):
        c = nib[:, :, k]
        s = _IMA_STEP[index]
        d = (s >> 3) + np.where(c & 4, s, 0) + np.where(c & 2, s >> 1, 0) + np.where(c & 1, s >> 2, 0)
        pred = np.clip(np.where(c & 8, pred - d, pred + d), -32768, 32767)
        index = np.clip(index + _IMA_INDEX[c & 7], 0, 88)
        out.append(pred)
    x = np.stack(out, axis=1)  # [block][frame][channel]
    return np.ascontiguousarray(x.reshape(-1, ch)[:n_frames].astype(np.int16))


def read_adpcm(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """IMA ADPCM in RIFF/WAVE or CAF -> (float32 samples [n, channels], sample_rate): the decoded int16 / 32768."""
    got = adpcm_raw(path)
    if got is None:
        raise ValueError(f"{path}: not an IMA ADPCM file (RIFF/WAVE format tag 0x11 or CAF ima4)")
    blocks, codec, ch, sr, block_bytes, _block_frames, n = got
    return ima_decode(blocks, codec, ch, block_bytes, n).astype(np.float32) * np.float32(1.0 / 32768.0), sr


def read_wav(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """Return (float32 samples [n, channels] in [-1, 1), sample_rate) for PCM8/16/24/32, float, G.711 or IMA ADPCM WAV."""
    chunks = _wav_chunks(path)
    if chunks[1] == WAV_TAG_IMA:
        return read_adpcm(path)
    pcm, tag, bits, ch, sr = _wav_pcm(path, chunks)
    if tag == 1:  # integer PCM; scale factors are powers of two: multiplying by the reciprocal is exact
        if bits == 8:
            x = np.frombuffer(pcm, dtype=np.uint8).astype(np.float32)
            x -= 128.0
            x *= np.float32(1.0 / 128.0)
        elif bits == 16:
            x = np.frombuffer(pcm[: len(pcm) // 2 * 2], dtype="<i2").astype(np.float32)
            x *= np.float32(1.0 / 32768.0)
        elif bits == 24:
            b = np.frombuffer(pcm[: len(pcm) // 3 * 3], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = np.where(v >= 1 << 23, v - (1 << 24), v)
            x = v.astype(np.float32) / float(1 << 23)
        elif bits == 32:
            x = (np.frombuffer(pcm[: len(pcm) // 4 * 4], dtype="<i4").astype(np.float64) / float(1 << 31)).astype(np.float32)
        else:
            raise ValueError(f"{path}: unsupported PCM bit depth {bits}")
    elif tag == 3:  # IEEE float
        w = 4 if bits == 32 else 8
        x = np.frombuffer(pcm[: len(pcm) // w * w], dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
    elif tag in (6, 7):  # G.711
        x = g711_expand(np.frombuffer(pcm, dtype=np.uint8), "ulaw" if tag == 7 else "alaw").astype(np.float32) * np.float32(1.0 / 32768.0)
    else:
        raise ValueError(f"{path}: unsupported WAV format tag {tag}")
    n = len(x) // ch
    return x[: n * ch].reshape(n, ch), sr


_WAV_CODES = {wav: code for code, wav in _n.BP_PCM_WAV.items()}  # WAV (format tag, bits) -> BP_PCM_*


def _ext80(b: bytes) -> float:
    """An 80-bit extended float (AIFF's sample rate): sign and 15-bit exponent, 64-bit mantissa with its integer bit."""
    se, mant = struct.unpack(">HQ", b)
    v = math.ldexp(float(mant), (se & 0x7FFF) - 16383 - 63)
    return -v if se & 0x8000 else v


def _rate(path, v: float) -> int:
    if not (0.5 <= v < 2147483647.0):
        raise ValueError(f"{path}: bad sample rate in the header")
    return int(math.floor(v + 0.5))


def _int_code(nbytes: int, little: bool) -> int:
    return {1: _n.BP_PCM_S8, 2: _n.BP_PCM_S16 if little else _n.BP_PCM_S16_BE, 3: _n.BP_PCM_S24 if little else _n.BP_PCM_S24_BE,
            4: _n.BP_PCM_S32 if little else _n.BP_PCM_S32_BE}[nbytes]


def _aiff_raw(path, data: memoryview):
    """AIFF / AIFF-C (Apple's AIFF 1.3 and AIFF-C drafts): chunks in any order, padded to even size; COMM says what the
    samples are, SSND holds them behind an offset."""
    aifc = bytes(data[8:12]) == b"AIFC"
    comm = ssnd = None
    pos = 12
    while pos + 8 <= len(data):
        cid = bytes(data[pos : pos + 4])
        size = struct.unpack_from(">I", data, pos + 4)[0]
        body = data[pos + 8 : pos + 8 + size]
        if cid == b"COMM":
            need = 22 if aifc else 18
            if len(body) < need:
                raise ValueError(f"{path}: truncated COMM chunk: {len(body)} of {need} bytes")
            ch, frames, bits = struct.unpack_from(">HIH", body, 0)
            comm = (ch, frames, bits, _ext80(bytes(body[8:18])), bytes(body[18:22]) if aifc else b"NONE")
        elif cid == b"SSND":
            if len(body) < 8:
                raise ValueError(f"{path}: truncated SSND chunk")
            ssnd = body[8 + min(struct.unpack_from(">I", body, 0)[0], len(body) - 8) :]
        pos += 8 + size + (size & 1)
    if comm is None:
        raise ValueError(f"{path}: missing COMM chunk")
    ch, frames, bits, rate, ctype = comm
    if ssnd is None:
        if frames:
            raise ValueError(f"{path}: missing SSND chunk")
        ssnd = data[:0]
    if ch < 1:
        raise ValueError(f"{path}: zero channels")
    if ctype in (b"NONE", b"twos", b"in24", b"in32", b"sowt"):
        if not 1 <= bits <= 32:
            raise ValueError(f"{path}: unsupported AIFF sample size {bits}")
        code = _int_code((bits + 7) // 8, ctype == b"sowt")
    elif ctype in (b"fl32", b"FL32") and bits == 32:
        code = _n.BP_PCM_F32_BE
    elif ctype in (b"fl64", b"FL64") and bits == 64:
        code = _n.BP_PCM_F64_BE
    elif ctype in (b"ulaw", b"ULAW"):
        code = _n.BP_PCM_ULAW
    elif ctype in (b"alaw", b"ALAW"):
        code = _n.BP_PCM_ALAW
    elif ctype == b"raw " and 1 <= bits <= 8:
        code = _n.BP_PCM_U8
    elif ctype in (b"fl32", b"FL32", b"fl64", b"FL64", b"raw "):
        raise ValueError(f"{path}: unsupported sample size {bits} for AIFF-C compression type {ctype.decode('latin-1')!r}")
    else:
        raise ValueError(f"{path}: unsupported AIFF-C compression type {ctype.decode('latin-1')!r}")
    return ssnd, code, ch, _rate(path, rate), frames


def _caf_raw(path, data: memoryview):
    """CAF (Apple Core Audio Format 1.0): `desc` says what the samples are, `data` holds them behind a 4-byte edit count."""
    if len(data) < 8 or struct.unpack_from(">H", data, 4)[0] != 1:
        raise ValueError(f"{path}: unsupported CAF version")
    desc = pcm = None
    pos = 8
    while pos + 12 <= len(data):
        cid = bytes(data[pos : pos + 4])
        size = struct.unpack_from(">q", data, pos + 4)[0]
        rest = len(data) - (pos + 12)
        if size < 0 and cid != b"data":
            raise ValueError(f"{path}: negative size of CAF chunk {cid.decode('latin-1')!r}")
        body = data[pos + 12 : pos + 12 + (rest if size < 0 else min(size, rest))]
        if cid == b"desc":
            if len(body) < 32:
                raise ValueError(f"{path}: truncated desc chunk")
            desc = struct.unpack_from(">d4sIIIII", body, 0)
        elif cid == b"data":
            pcm = body[4:]
        if size < 0:
            break
        pos += 12 + size
    if desc is None or pcm is None:
        raise ValueError(f"{path}: missing desc or data chunk")
    rate, fid, flags, packet_bytes, packet_frames, ch, bits = desc
    if ch < 1:
        raise ValueError(f"{path}: zero channels")
    is_float, little = bool(flags & 1), bool(flags & 2)
    if fid == b"lpcm" and is_float and bits in (32, 64):
        code = {(32, True): _n.BP_PCM_F32, (32, False): _n.BP_PCM_F32_BE, (64, True): _n.BP_PCM_F64, (64, False): _n.BP_PCM_F64_BE}[(bits, little)]
    elif fid == b"lpcm" and not is_float and bits in (8, 16, 24, 32):
        code = _int_code(bits // 8, little)
    elif fid == b"lpcm":
        raise ValueError(f"{path}: unsupported CAF lpcm of {bits}-bit {'floats' if is_float else 'integers'}")
    elif fid in (b"ulaw", b"alaw"):
        code = _n.BP_PCM_ULAW if fid == b"ulaw" else _n.BP_PCM_ALAW
    else:
        raise ValueError(f"{path}: unsupported CAF format {fid.decode('latin-1')!r}")
    if packet_frames != 1 or packet_bytes != ch * _n.BP_PCM_WIDTH[code]:
        raise ValueError(f"{path}: unsupported CAF packet layout: {packet_frames} frames in {packet_bytes} bytes a packet")
    return pcm, code, ch, _rate(path, rate), None


_AU_CODES = {1: _n.BP_PCM_ULAW, 2: _n.BP_PCM_S8, 3: _n.BP_PCM_S16_BE, 4: _n.BP_PCM_S24_BE, 5: _n.BP_PCM_S32_BE,
             6: _n.BP_PCM_F32_BE, 7: _n.BP_PCM_F64_BE, 27: _n.BP_PCM_ALAW}


def _au_raw(path, data: memoryview):
    """AU (.snd, the Sun / NeXT header): six big-endian words, an annotation, the samples."""
    if len(data) < 24:
        raise ValueError(f"{path}: truncated AU header")
    header_bytes, data_size, encoding, rate, ch = struct.unpack_from(">IIIII", data, 4)
    if header_bytes < 24:
        raise ValueError(f"{path}: bad AU header size {header_bytes}")
    if encoding not in _AU_CODES:
        raise ValueError(f"{path}: unsupported AU encoding {encoding}")
    if ch < 1:
        raise ValueError(f"{path}: zero channels")
    pcm = data[header_bytes:]
    if data_size != 0xFFFFFFFF:
        pcm = pcm[:data_size]
    return pcm, _AU_CODES[encoding], ch, _rate(path, float(rate)), None


def pcm_raw(path: Union[str, pathlib.Path]):
    """The samples of a WAV (RF64 / BW64 too), AIFF / AIFF-C, CAF or AU file as the file stores them: (uint8 view of the
    samples, BP_PCM_* code, channels, sample_rate, n_frames) — what `Model.predict_pcm_raw` takes.  `wav_raw` for every
    container the device converts itself; independent of the C++ parsers (csrc/pcm_file.cpp), which the tests hold to it.
    Not read: the little-endian AU variant, Sony Wave64 and the compressed AIFF-C types; IMA ADPCM files hold blocks, not
    samples: `adpcm_raw`."""
    with open(path, "rb") as f:
        head = f.read(12)
    if head[:4] in (b"RIFF", b"RF64", b"BW64") and head[8:12] == b"WAVE":
        pcm, tag, bits, ch, sr = wav_raw(path)
        code, frames = _WAV_CODES[(tag, bits)], None
    else:
        with open(path, "rb") as f:
            data = memoryview(f.read())
        if head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC"):
            pcm, code, ch, sr, frames = _aiff_raw(path, data)
        elif head[:4] == b"caff":
            pcm, code, ch, sr, frames = _caf_raw(path, data)
        elif head[:4] == b".snd":
            pcm, code, ch, sr, frames = _au_raw(path, data)
        else:
            raise ValueError(f"{path}: not a WAV, AIFF, CAF or AU file")
    held = len(pcm) // (_n.BP_PCM_WIDTH[code] * ch)
    n = held if frames is None else min(frames, held)  # a file that ends early: what is there
    return np.frombuffer(pcm, dtype=np.uint8)[: n * ch * _n.BP_PCM_WIDTH[code]], code, ch, sr, n


def g711_expand(b: np.ndarray, law: str) -> np.ndarray:
    """ITU-T G.711 bytes -> int32 values left-justified in 16 bits, in arithmetic (law: "ulaw" | "alaw")."""
    b = b.astype(np.int32)
    if law == "ulaw":
        u = ~b & 0xFF
        t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
        return np.where(u & 0x80, 0x84 - t, t - 0x84)
    a = b ^ 0x55
    t, s = (a & 15) << 4, (a >> 4) & 7
    t = np.where(s == 0, t + 8, np.where(s == 1, t + 0x108, (t + 0x108) << np.maximum(s - 1, 0)))
    return np.where(a & 0x80, t, -t)


def pcm_to_float(raw: np.ndarray, code: int, channels: int) -> np.ndarray:
    """The uint8 samples `pcm_raw` returns -> float32 [n, channels], the scaling of libsndfile's float read: integers /
    2^(bits-1), unsigned bytes (v - 128) / 128, G.711 expanded / 32768, float64 rounded (powers of two: exact)."""
    raw = np.ascontiguousarray(raw)
    if code in (_n.BP_PCM_S16, _n.BP_PCM_S16_BE):
        x = raw.view("<i2" if code == _n.BP_PCM_S16 else ">i2").astype(np.float32) * np.float32(1.0 / 32768.0)
    elif code in (_n.BP_PCM_S24, _n.BP_PCM_S24_BE):
        b = raw.reshape(-1, 3).astype(np.int32)
        lo, hi = (0, 2) if code == _n.BP_PCM_S24 else (2, 0)
        v = b[:, lo] | (b[:, 1] << 8) | (b[:, hi] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float32) / np.float32(1 << 23)
    elif code in (_n.BP_PCM_S32, _n.BP_PCM_S32_BE):
        x = (raw.view("<i4" if code == _n.BP_PCM_S32 else ">i4").astype(np.float64) / float(1 << 31)).astype(np.float32)
    elif code == _n.BP_PCM_U8:
        x = (raw.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    elif code == _n.BP_PCM_S8:
        x = raw.view(np.int8).astype(np.float32) * np.float32(1.0 / 128.0)
    elif code in (_n.BP_PCM_ULAW, _n.BP_PCM_ALAW):
        x = g711_expand(raw, "ulaw" if code == _n.BP_PCM_ULAW else "alaw").astype(np.float32) * np.float32(1.0 / 32768.0)
    elif code in (_n.BP_PCM_F32, _n.BP_PCM_F32_BE):
        x = raw.view("<f4" if code == _n.BP_PCM_F32 else ">f4").astype(np.float32)
    elif code in (_n.BP_PCM_F64, _n.BP_PCM_F64_BE):
        x = raw.view("<f8" if code == _n.BP_PCM_F64 else ">f8").astype(np.float32)
    else:
        raise ValueError(f"unknown BP_PCM_* code {code}")
    return x.reshape(-1, channels)


def _read_container(path, magics) -> Tuple[np.ndarray, int]:
    with open(path, "rb") as f:
        head = f.read(12)
    if head[:4] not in magics:
        raise ValueError(f"{path}: not such a file")
    raw, code, ch, sr, _n_frames = pcm_raw(path)
    return pcm_to_float(raw, code, ch), sr


def read_aiff(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """AIFF / AIFF-C -> (float32 samples [n, channels], sample_rate); in numpy, the checker of the native parser."""
    return _read_container(path, (b"FORM",))


def read_caf(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """CAF (lpcm, ulaw, alaw) -> (float32 samples [n, channels], sample_rate)."""
    return _read_container(path, (b"caff",))


def read_au(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """AU (.snd) -> (float32 samples [n, channels], sample_rate)."""
    return _read_container(path, (b".snd",))


def to_mono(x: np.ndarray) -> np.ndarray:
    """Channel mean (librosa.to_mono semantics)."""
    return x if x.ndim == 1 else x.mean(axis=1, dtype=np.float32) if x.shape[1] > 1 else x[:, 0]


_SOXR_HQ_BITS = 20  # soxr_quality_spec(SOXR_HQ): 20-bit precision
_BETA_FIT = (  # libsoxr lsx_kaiser_beta: cubic fits of the Kaiser beta over the attenuation, per octave of transition width
    (-6.784957e-10, 1.02856e-05, 0.1087556, -0.8978365),
    (-6.897885e-10, 1.027433e-05, 0.10876, -0.8974658),
    (-1.000683e-09, 1.030092e-05, 0.1087677, -0.8977898),
    (-3.654474e-10, 1.040631e-05, 0.1087085, -0.8917766),
    (8.106988e-09, 6.983091e-06, 0.1091387, -0.9022048),
    (9.519571e-09, 7.272678e-06, 0.1090068, -0.8890768),
    (-5.626821e-09, 1.342186e-05, 0.1083999, -0.8565452),
    (-9.965946e-08, 5.073548e-05, 0.1040967, -0.6822778),
    (1.604808e-07, -5.856462e-05, 0.1185998, -1.24824),
    (-1.511964e-07, 6.363034e-05, 0.1064627, -0.8076665),
)


def soxr_hq_taps(up: int, down: int) -> np.ndarray:
    """The anti-alias / anti-image filter of an up : down rate change at the rate `orig_sr * up`, DC gain `up`.

    libsoxr's SOXR_HQ recipe (soxr.c soxr_quality_spec, filter.c lsx_design_lpf / lsx_kaiser_beta / lsx_make_lpf):
    pass-band end 1 - .05 / TO_3dB(20 bit) = 0.9136 and stop-band begin 1.0 of the lower Nyquist, 21 bit = 126.4 dB,
    6 dB point half way, beta from libsoxr's fit, taps from its length formula rounded up to 1 (mod 4)."""
    from scipy.special import i0

    db = 20.0 * np.log10(2.0)
    rej = _SOXR_HQ_BITS * db
    fp = 1.0 - 0.05 / ((1.6e-6 * rej - 7.5e-4) * rej + 0.646)
    att = (_SOXR_HQ_BITS + 1) * db
    fn = float(max(up, down))  # Nyquist of the filter's rate in units of the lower Nyquist
    tr_bw = 0.5 * (1.0 - fp) / fn
    fc = 1.0 / fn - tr_bw
    realm = np.log2(tr_bw * 0.5 / fc / 0.0005)
    r0 = int(np.clip(int(realm), 0, 9))
    r1 = int(np.clip(int(realm) + 1, 0, 9))
    b0, b1 = (((c[0] * att + c[1]) * att + c[2]) * att + c[3] for c in (_BETA_FIT[r0], _BETA_FIT[r1]))
    beta = b0 + (b1 - b0) * (realm - int(realm))
    n = int(np.ceil((((0.0007528358 - 1.577737e-05 * beta) * beta + 0.6248022) * beta + 0.06186902) / tr_bw + 1))
    n = (n + 2) // 4 * 4 + 1
    z = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    sinc = np.where(z != 0, np.sin(fc * np.pi * z) / np.where(z != 0, np.pi * z, 1.0), fc)
    y = z / (0.5 * (n - 1) + 0.5)
    return sinc * i0(beta * np.sqrt(1.0 - y * y)) / i0(beta) * up


def resample(x: np.ndarray, orig_sr: int, target_sr: int = AUDIO_SAMPLE_RATE) -> np.ndarray:
    """`librosa.resample(x, orig_sr, target_sr)` with its default soxr_hq response: one zero-phase polyphase stage,
    the signal zero outside the file, output length ceil(n * target / orig)."""
    if orig_sr == target_sr:
        return np.ascontiguousarray(x, dtype=np.float32)
    import scipy.signal

    fr = Fraction(int(target_sr), int(orig_sr))
    up, down = fr.numerator, fr.denominator
    h = soxr_hq_taps(up, down)
    c = (len(h) - 1) // 2
    n_out = int(np.ceil(len(x) * target_sr / orig_sr))
    # upfirdn output i = sum_j x[j] h[i * down - j * up]; output sample k sits at filter index k * down + c
    lead = -c % down
    y = scipy.signal.upfirdn(np.concatenate([np.zeros(lead), h]), x.astype(np.float64), up, down)
    k0 = (c + lead) // down
    y = y[k0 : k0 + n_out]
    if len(y) < n_out:
        y = np.pad(y, (0, n_out - len(y)))
    return np.ascontiguousarray(y, dtype=np.float32)


def read_flac(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """FLAC -> (float32 samples [n, channels] in [-1, 1), sample_rate): the native decoder (csrc/flac_decode.cpp),
    CRC- and MD5-checked; value / 2^(bits - 1) like libsndfile's float read that librosa.load uses."""
    import ctypes as C

    from . import _native

    lib = _native.load_library()
    with open(path, "rb") as f:
        data = f.read()
    ch, sr, bits, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    rc = lib.bp_flac_info(data, len(data), C.byref(ch), C.byref(sr), C.byref(bits), C.byref(n))
    if rc != _native.BP_OK:
        raise ValueError(f"{path}: {lib.bp_audio_last_error().decode(errors='replace')}")
    pcm = np.empty((n.value, ch.value), dtype=np.float32)
    got = C.c_int64()
    rc = lib.bp_flac_decode(data, len(data), pcm.ctypes.data, n.value, C.byref(got))
    if rc != _native.BP_OK or got.value != n.value:
        raise ValueError(f"{path}: {lib.bp_audio_last_error().decode(errors='replace')}")
    return pcm, sr.value


def _read_with_optional_backend(path: str) -> Tuple[np.ndarray, int]:
    """mp3 / ogg / m4a and anything else librosa.load would hand to soundfile or audioread: use whichever of those
    decoders this installation has (soundfile, audioread, an `ffmpeg` executable); none ships with this package."""
    try:
        import soundfile  # type: ignore

        x, sr = soundfile.read(path, dtype="float32", always_2d=True)
        return np.ascontiguousarray(x), int(sr)
    except ImportError:
        pass
    try:
        import audioread  # type: ignore

        with audioread.audio_open(path) as f:
            sr, ch = f.samplerate, f.channels
            buf = b"".join(f)
        x = np.frombuffer(buf, dtype="<i2").astype(np.float32) / 32768.0
        return x[: len(x) // ch * ch].reshape(-1, ch), int(sr)
    except ImportError:
        pass
    import shutil
    import subprocess

    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg:
        probe = subprocess.run([ffmpeg, "-i", path], capture_output=True, text=True).stderr
        import re

        m = re.search(r"Audio:.*?(\d+) Hz, (mono|stereo|(\d+) channels|[\d.]+)", probe)
        if m:
            sr = int(m.group(1))
            ch = {"mono": 1, "stereo": 2}.get(m.group(2)) or (int(m.group(3)) if m.group(3) else 2)
            raw = subprocess.run([ffmpeg, "-v", "error", "-i", path, "-f", "f32le", "-acodec", "pcm_f32le", "-ac", str(ch),
                                  "-ar", str(sr), "-"], capture_output=True, check=True).stdout
            x = np.frombuffer(raw, dtype="<f4")
            return np.ascontiguousarray(x[: len(x) // ch * ch].reshape(-1, ch)), sr
    raise ValueError(
        f"{path}: not a WAV or FLAC file, and no decoder for other formats (mp3 / ogg / m4a) is installed: "
        "basic_pitch_amd reads RIFF/WAVE and FLAC natively and uses soundfile, audioread or an ffmpeg executable when present"
    )


def read_audio(path: Union[str, pathlib.Path]) -> Tuple[np.ndarray, int]:
    """Decode any supported file to (float32 [n, channels], sample_rate): the decode half of librosa.load
    (inference.py:239).  Dispatch is by content, not extension: RIFF/WAVE (RF64 / BW64 too), AIFF / AIFF-C, CAF, AU and
    FLAC are read natively."""
    with open(path, "rb") as f:
        head = f.read(12)
    if head[:4] in (b"RIFF", b"RF64", b"BW64") and head[8:12] == b"WAVE":
        return read_wav(path)
    if head[:4] == b"caff" and adpcm_raw(path) is not None:
        return read_adpcm(path)
    if (head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC")) or head[:4] in (b"caff", b".snd"):
        raw, code, ch, sr, _n_frames = pcm_raw(path)
        return pcm_to_float(raw, code, ch), sr
    if head[:4] == b"fLaC" or (head[:3] == b"ID3" and str(path).lower().endswith(".flac")):
        return read_flac(path)
    return _read_with_optional_backend(str(path))


def load(path: Union[str, pathlib.Path], sr: int = AUDIO_SAMPLE_RATE, mono: bool = True) -> Tuple[np.ndarray, int]:
    """`librosa.load(path, sr=sr, mono=True)`: decode, channel mean, soxr_hq-design resampling."""
    x, file_sr = read_audio(path)
    y = to_mono(x) if mono else x
    return resample(np.ascontiguousarray(y), file_sr, sr), sr


def get_duration(filename: Union[str, pathlib.Path]) -> float:
    x, sr = read_audio(filename)
    return x.shape[0] / float(sr)
