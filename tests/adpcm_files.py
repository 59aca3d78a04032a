"""IMA ADPCM test files without the library (include/basic_pitch_amd_adpcm.h): an encoder built on the standard library's
`audioop.lin2adpcm`, the RIFF/WAVE (format tag 0x11) and CAF (`ima4`) writers around it, G.711 WAV files, and the reference
decode of a file's blocks by `audioop.adpcm2lin` — per block (WAV) or packet (CAF), from the header's state, on nibble-swapped
bytes (audioop packs the first code of a byte into the HIGH nibble; both file layouts put it into the LOW one).

Nothing here imports basic_pitch_amd: the writers state the layouts as the header file does."""
import struct
import warnings

import numpy as np

with warnings.catch_warnings():
    warnings.simplefilter("ignore", DeprecationWarning)
    import audioop

import container_files as K

IMA_WAV, IMA4 = 1, 2
TAG_IMA = 0x11
_SWAP = bytes(((b & 15) << 4) | (b >> 4) for b in range(256))


def swap_nibbles(b: bytes) -> bytes:
    return bytes(b).translate(_SWAP)


def two_tones(n_frames, channels, rate, seed=0):
    """int16 [n_frames, channels]: two tones a channel, loud enough that the step index moves through its range."""
    t = np.arange(n_frames, dtype=np.float64) / rate
    x = np.empty((n_frames, channels), np.float64)
    for c in range(channels):
        f0 = 220.0 * (1 + c) * (1 + 0.07 * seed)
        x[:, c] = 0.45 * np.sin(2 * np.pi * f0 * t) + 0.35 * np.sin(2 * np.pi * 2.51 * f0 * t + c)
    return np.round(x * 32767.0).astype(np.int16)


# ---- the block layouts ---------------------------------------------------------------------------------------------------------
def wav_block_frames(block_bytes, channels):
    return (block_bytes - 4 * channels) * 2 // channels + 1


def wav_blocks(pcm, block_bytes):
    """int16 [n, channels] -> the bytes of ceil(n / block_frames) blocks (the last one padded with its last frame)."""
    n, ch = pcm.shape
    bf = wav_block_frames(block_bytes, ch)
    assert (block_bytes - 4 * ch) > 0 and (block_bytes - 4 * ch) % (4 * ch) == 0
    n_blocks = -(-n // bf)
    if n_blocks * bf > n:
        pcm = np.concatenate([pcm, np.repeat(pcm[-1:], n_blocks * bf - n, axis=0)])
    index = [0] * ch
    out = bytearray()
    for b in range(n_blocks):
        blk = pcm[b * bf : (b + 1) * bf]
        codes = []
        for c in range(ch):
            first = int(blk[0, c])
            out += struct.pack("<hBB", first, index[c], 0)
            packed, (_, index[c]) = audioop.lin2adpcm(blk[1:, c].astype("<i2").tobytes(), 2, (first, index[c]))
            codes.append(swap_nibbles(packed))
        for g in range((bf - 1) // 8):
            for c in range(ch):
                out += codes[c][4 * g : 4 * g + 4]
    return bytes(out)


def ima4_packets(pcm):
    """int16 [n, channels] -> the bytes of ceil(n / 64) packets of 34 bytes a channel."""
    n, ch = pcm.shape
    n_packets = -(-n // 64)
    if n_packets * 64 > n:
        pcm = np.concatenate([pcm, np.repeat(pcm[-1:], n_packets * 64 - n, axis=0)])
    state = [(0, 0)] * ch
    out = bytearray()
    for p in range(n_packets):
        for c in range(ch):
            pred, index = state[c]
            h = (pred & 0xFF80) | index
            start = struct.unpack(">h", struct.pack(">H", h & 0xFF80))[0]  # what the decoder starts from
            packed, state[c] = audioop.lin2adpcm(pcm[p * 64 : (p + 1) * 64, c].astype("<i2").tobytes(), 2, (start, index))
            out += struct.pack(">H", h) + swap_nibbles(packed)
    return bytes(out)


def reference_decode(blocks, codec, channels, block_bytes, n_frames):
    """int16 [n_frames, channels] of whole blocks by `audioop.adpcm2lin`: chain by chain from the header's state (a step index
    above 88 is 88)."""
    blocks = bytes(blocks)
    nb = len(blocks) // block_bytes
    bf = wav_block_frames(block_bytes, channels) if codec == IMA_WAV else 64
    out = np.zeros((nb * bf, channels), np.int16)
    for b in range(nb):
        blk = blocks[b * block_bytes : (b + 1) * block_bytes]
        for c in range(channels):
            if codec == IMA_WAV:
                pred, index = struct.unpack_from("<hB", blk, 4 * c)
                body = blk[4 * channels :]
                codes = b"".join(body[4 * channels * g + 4 * c : 4 * channels * g + 4 * c + 4] for g in range(len(body) // (4 * channels)))
                out[b * bf, c] = pred
                first = 1
            else:
                h = struct.unpack_from(">H", blk, 34 * c)[0]
                pred, index = struct.unpack(">h", struct.pack(">H", h & 0xFF80))[0], h & 0x7F
                codes = blk[34 * c + 2 : 34 * c + 34]
                first = 0
            lin, _ = audioop.adpcm2lin(swap_nibbles(codes), 2, (pred, min(index, 88)))
            out[b * bf + first : (b + 1) * bf, c] = np.frombuffer(lin, "<i2")
    return out[:n_frames]


# ---- RIFF/WAVE -------------------------------------------------------------------------------------------------------------------
def _ima_fmt(channels, rate, block_bytes, bits=4, extensible=False, samples_field=True):
    bf = wav_block_frames(block_bytes, channels) if channels and block_bytes > 4 * channels else 0
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else TAG_IMA, channels, rate, rate * block_bytes // max(bf, 1), block_bytes, bits)
    if extensible:  # cbSize 22: valid bits, channel mask, the GUID whose first two bytes are the tag
        ext = struct.pack("<HI", bits, 0) + struct.pack("<H", TAG_IMA) + bytes.fromhex("000000001000800000aa00389b71")
        return _chunk(b"fmt ", base + struct.pack("<H", 22) + ext)
    extra = struct.pack("<HH", 2, bf) if samples_field else struct.pack("<H", 0)
    return _chunk(b"fmt ", base + extra)


def _chunk(cid, body):
    return struct.pack("<4sI", cid, len(body)) + body + (b"\0" if len(body) & 1 else b"")


def ima_wav_of(blocks, channels, rate, block_bytes, fact=None, bits=4, extensible=False, rf64=False, samples_field=True, tail=b""):
    """The file around `blocks` (+ `tail`: a trailing partial block).  fact: the fact chunk's sample count (None: no chunk)."""
    data = bytes(blocks) + bytes(tail)
    fmt = _ima_fmt(channels, rate, block_bytes, bits, extensible, samples_field)
    fact_chunk = b"" if fact is None else _chunk(b"fact", struct.pack("<I", fact))
    pad = b"\0" if len(data) & 1 else b""
    if rf64:
        body = fmt + fact_chunk + struct.pack("<4sI", b"data", 0xFFFFFFFF) + data + pad
        ds64 = struct.pack("<4sIQQQI", b"ds64", 28, 4 + 36 + len(body), len(data), fact or 0, 0)
        return struct.pack("<4sI4s", b"RF64", 0xFFFFFFFF, b"WAVE") + ds64 + body
    body = fmt + fact_chunk + struct.pack("<4sI", b"data", len(data)) + data + pad
    return struct.pack("<4sI4s", b"RIFF", 4 + len(body), b"WAVE") + body


def ima_wav(pcm, rate, block_bytes, fact="frames", **kw):
    """int16 [n, channels] -> an IMA ADPCM WAV file; fact="frames": the true count."""
    pcm = np.asarray(pcm, np.int16)
    pcm = pcm[:, None] if pcm.ndim == 1 else pcm
    return ima_wav_of(wav_blocks(pcm, block_bytes) if len(pcm) else b"", pcm.shape[1], rate, block_bytes,
                      len(pcm) if fact == "frames" else fact, **kw)


def g711_wav(codes, law, channels, rate, extensible=False, rf64=False):
    """G.711 bytes in RIFF/WAVE: tag 7 (mu-law) or 6 (A-law), 8 bits."""
    tag = 7 if law == "ulaw" else 6
    data = bytes(codes)
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels, channels, 8)
    if extensible:
        base += struct.pack("<HHI", 22, 8, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    else:
        base += struct.pack("<H", 0)
    fmt = _chunk(b"fmt ", base)
    pad = b"\0" if len(data) & 1 else b""
    if rf64:
        body = fmt + struct.pack("<4sI", b"data", 0xFFFFFFFF) + data + pad
        ds64 = struct.pack("<4sIQQQI", b"ds64", 28, 4 + 36 + len(body), len(data), len(data) // channels, 0)
        return struct.pack("<4sI4s", b"RF64", 0xFFFFFFFF, b"WAVE") + ds64 + body
    body = fmt + _chunk(b"fact", struct.pack("<I", len(data) // channels)) + struct.pack("<4sI", b"data", len(data)) + data + pad
    return struct.pack("<4sI4s", b"RIFF", 4 + len(body), b"WAVE") + body


# ---- CAF ---------------------------------------------------------------------------------------------------------------------------
def ima4_caf_of(packets, channels, rate, valid_frames=None, priming=0, packet_frames=64, packet_bytes=None, pakt=True, data_size=None):
    """The file around `packets`.  valid_frames: the pakt chunk's count (None: packets x 64); pakt=False: no such chunk."""
    packets = bytes(packets)
    pb = 34 * channels if packet_bytes is None else packet_bytes
    n_packets = len(packets) // (34 * channels) if channels else 0
    valid = n_packets * 64 if valid_frames is None else valid_frames
    desc = struct.pack(">d4sIIIII", float(rate), b"ima4", 0, pb, packet_frames, channels, 0)
    out = b"caff" + struct.pack(">HH", 1, 0) + K.caf_chunk(b"desc", desc)
    if pakt:
        out += K.caf_chunk(b"pakt", struct.pack(">qqii", n_packets, valid, priming, n_packets * 64 - valid - priming))
    return out + K.caf_chunk(b"data", struct.pack(">I", 0) + packets, data_size)


def ima4_caf(pcm, rate, **kw):
    """int16 [n, channels] -> a CAF ima4 file whose pakt chunk says n valid frames."""
    pcm = np.asarray(pcm, np.int16)
    pcm = pcm[:, None] if pcm.ndim == 1 else pcm
    kw.setdefault("valid_frames", len(pcm))
    return ima4_caf_of(ima4_packets(pcm) if len(pcm) else b"", pcm.shape[1], rate, **kw)


# ---- blocks of random codes under chosen headers: both rails clamp, the index walks its whole range -------------------------------
HEADER_STATES = [(p, i) for p in (-32768, 0, 32767) for i in (0, 40, 88, 200)]


def random_wav_blocks(channels, code_bytes=4096, seed=7):
    """(blocks, block_bytes): one block per header state, `code_bytes` random code bytes a channel (index 200 is clamped to 88)."""
    rng = np.random.default_rng(seed)
    block_bytes = 4 * channels + code_bytes * channels
    out = bytearray()
    for pred, index in HEADER_STATES:
        for c in range(channels):
            out += struct.pack("<hBB", pred, index, 0xA5)
        out += rng.integers(0, 256, code_bytes * channels, dtype=np.uint8).tobytes()
    return bytes(out), block_bytes


def random_ima4_packets(channels, n_packets=40, seed=9):
    """packets of random codes; the header words cycle through predictors at both rails and indices 0 ... 127 (above 88: 88)."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    k = 0
    for _ in range(n_packets):
        for _c in range(channels):
            pred, index = HEADER_STATES[k % len(HEADER_STATES)]
            k += 1
            out += struct.pack(">H", (pred & 0xFF80) | min(index, 127)) + rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    return bytes(out)
