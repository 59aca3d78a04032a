"""FLAC streams off the test-side encoder's usual operating point (tests/flac_writer.py), shared by the host decoder's tests
(test_audio_decode.py) and the device decoder's (test_flac_device.py): every stream is built once per process — the Python
encoder is the slow part — and comes with the PCM it was made from, which is the one expected value of every comparison.

Families: LPC coefficient precision x shift (one pair per stream, and all pairs mixed from frame to frame; coefficients at
both limits of their range), full-scale 24-bit stereo against 15-bit coefficients at their limits (sums of 2^41.6), variable-block-size streams (RFC 9639 9.1.1 / 9.1.5: sample numbers of one
to four bytes), the sample-rate codes 12 and 14, forced Rice parameters 0 / 1 / 14 / 30, escaped partitions of 0 bits, and
frame headers planted inside the payload of verbatim frames (valid files whose samples happen to spell a sync code, a
header without reserved values and its CRC-8)."""
import collections
import functools
import itertools

import numpy as np

import flac_writer as FW

Stream = collections.namedtuple("Stream", "data pcm sr bits plants")
Stream.__new__.__defaults__ = ((),)


def _limits(prec):
    """coefficients pinned at both ends of a precision's range, the negative one first: -2^(prec - 1), 2^(prec - 1) - 1"""
    return [-(1 << (prec - 1)), (1 << (prec - 1)) - 1]


def _assert_both_limits(log, prec, shifts):
    """the stream as written holds coefficients of `prec` bits at the negative AND the positive limit: a test of "either
    sign's limit" proves nothing otherwise (a fitted predictor of these signals saturates at the positive end only, and
    a 1-bit coefficient it fits is always 0)"""
    lo, hi = _limits(prec)
    seen = [v for q, _ in log for v in q]
    assert seen.count(lo) > 0 and seen.count(hi) > 0, (prec, shifts, seen.count(lo), seen.count(hi))

MODES = ("indep", "ms", "ls", "sr")
PREC_SHIFT = ((1, 0), (2, 1), (7, 8), (15, 0), (15, 14), (15, 15))
SCHEDULES = {"mixed": [1152, 576, 4096, 16, 300], "one": [4608], "tiny": [17, 4096]}


def _tonal(n, bits, seed, ch=2):
    """a sine plus noise per channel: loud and noisy, quiet and clean, ... (what linear prediction is good and bad at)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    full = 1 << (bits - 1)
    cols = []
    for c in range(ch):
        amp, noise = (0.3, full // 64) if c % 2 == 0 else (0.2, full // 4096 + 2)
        cols.append(amp * full * np.sin(t * (0.021 if c % 2 == 0 else 0.0057) * (1 + c // 2)) + rng.integers(-noise, noise, n))
    return np.stack(cols, 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def precision_shift(prec, shift, bits):
    """one (precision, shift) pair for every LPC subframe: stereo, 34 frames of 256 + 5 samples, the orders cycling through the
    register classes (1, 4, 8, 12), the generic path (13, 32) and the four stereo modes.  The fitted coefficients of this
    signal reach the positive limit only (a1 ~ +2) and a fitted 1-bit coefficient is always 0, so every fifth frame (5 is
    coprime to the cycles of orders and modes) carries coefficients of the caller's: the two limits of the precision
    alternating, -2^(prec - 1) first — asserted to be in the stream.  Not for (15, 0): 2^14 times a sample is no
    prediction whose residual fits 32 bits (RFC 9639 9.2.7.3); that pair checks whole-number coefficients as fitted."""
    orders = (1, 4, 8, 12, 13, 32)
    pcm = _tonal(256 * 34 + 5, bits, 100 * prec + shift + bits)
    pinned = prec - shift <= 1
    log = []

    def plan(fi):
        p = dict(kind="lpc", lpc_order=orders[fi % 6], stereo=MODES[fi % 4], prec=prec, shift=shift, log=log)
        if pinned and fi % 5 == 2:
            p.update(coefs=_limits(prec), rice2=True, escape=False)  # residuals of several times the signal: Rice2's parameters
        return p

    data = FW.encode(pcm, 48000, bits, blocksize=256, plan=plan)
    if pinned:
        _assert_both_limits(log, prec, shift)
    return Stream(data, pcm, 48000, bits)


@functools.lru_cache(maxsize=None)
def precision_shift_mixed(bits):
    """precision {1, 2, 3, 7, 12, 15} x shift {0, 1, 8, 14, 15} changing from frame to frame together with the order (1..32), so
    that the frames a device wave decodes side by side hold different shifts, coefficient widths and orders: 70 frames.  The
    frames of 15 bits at shift 14 / 15 carry coefficients pinned at both limits (see precision_shift), asserted."""
    combos = list(itertools.product((1, 2, 3, 7, 12, 15), (0, 1, 8, 14, 15)))
    orders = (1, 2, 4, 5, 8, 9, 12, 13, 20, 32, 3, 11, 7, 16, 6, 10)
    pcm = _tonal(256 * 70 + 31, bits, 7 + bits)

    def plan(fi):
        prec, shift = combos[(7 * fi) % len(combos)]
        p = dict(kind="lpc", lpc_order=orders[fi % len(orders)], stereo=MODES[fi % 4], prec=prec, shift=shift,
                 escape=(fi % 7 == 6), log=log if prec == 15 else None)
        if prec == 15 and shift >= 14:
            p.update(coefs=_limits(15), rice2=True, escape=False)
        return p

    log = []
    data = FW.encode(pcm, 48000, bits, blocksize=256, plan=plan)
    _assert_both_limits(log, 15, (14, 15))
    return Stream(data, pcm, 48000, bits)


@functools.lru_cache(maxsize=None)
def full_scale(mode):
    """The largest sums of products a valid stream asks of the predictor.  24-bit samples at full scale that change sign
    from sample to sample, the channels in opposite phase (the side channel is +-(2^24 - 1), 25 bits), the phase slipping
    at random every ~40 samples; order 12 with 15-bit coefficients at shift 14 pinned at -2^14, 2^14 - 1, -2^14, ...
    Against samples of alternating sign all twelve products have one sign: |sum| reaches 12 x 2^14 x 2^24 ~ 2^41.6 on the
    side channel and 2^40.6 on a plain one — asserted, with the count of pinned coefficients —, of the 2^51 that the device's
    float64 predictor has room for.  The prediction is 12 times the sample, the residual 11 times (2^28.5: it fits 32 bits,
    coded with Rice2 parameters)."""
    rng = np.random.default_rng(41)
    full = 1 << 23
    sign = np.where((np.arange(2000) + np.cumsum(rng.integers(0, 40, 2000) == 0)) % 2 == 0, 1, -1)
    pcm = np.stack([np.where(sign > 0, full - 1, -full), np.where(sign > 0, -full, full - 1)], 1).astype(np.int64)
    log = []
    plan = lambda fi: dict(kind="lpc", lpc_order=12, stereo=mode, prec=15, shift=14, coefs=_limits(15), rice2=True,
                           escape=False, log=log)
    data = FW.encode(pcm, 96000, 24, blocksize=500, plan=plan)
    # 4 frames x 2 subframes of 12 pinned coefficients each ("ms": the mid channel is the constant -1, 4 LPC subframes)
    assert len(log) == (4 if mode == "ms" else 8) and all(q == _limits(15) * 6 for q, _ in log)
    top = max(m for _, m in log)
    assert top >= (11 << 14 << (23 if mode == "indep" else 24)), (mode, top)  # >= 2^40.4 / 2^41.4 (a slip costs a product or two)
    return Stream(data, pcm, 96000, 24)


@functools.lru_cache(maxsize=None)
def variable(name, wide=False):
    """a variable-block-size stream on one of SCHEDULES: 30,000 stereo 16-bit samples, or (wide) 12,000 of three 24-bit
    channels"""
    pcm = _tonal(12000, 24, 52, ch=3) if wide else _tonal(30000, 16, 51)
    bits = 24 if wide else 16
    return Stream(FW.encode(pcm, 44100, bits, sizes=SCHEDULES[name]), pcm, 44100, bits)


@functools.lru_cache(maxsize=None)
def long_numbers(nbytes):
    """variable block size, mono 16-bit, with sample numbers of `nbytes` bytes in the frame headers (RFC 9639 9.1.5: three bytes
    from 2^11, four from 2^16, five from 2^21).  3: 70,000 samples.  4 (numbers of four and of five bytes): 33 silent frames
    of 65,535 samples, which cost a few bytes each, then four frames of signal where the numbers are longest"""
    if nbytes == 3:
        pcm = _tonal(70000, 16, 53, ch=1)
        sizes = [4096, 1152, 16]
    else:
        sizes = [65535] * 33 + [4096, 4608, 4096, 4096]
        pcm = np.zeros((sum(sizes) - 1500, 1), np.int64)
        pcm[33 * 65535 :] = _tonal(len(pcm) - 33 * 65535, 16, 54, ch=1)
    return Stream(FW.encode(pcm, 44100, 16, sizes=sizes), pcm, 44100, 16)


@functools.lru_cache(maxsize=None)
def rate_code(sr, code):
    """the sample rate written behind the coded number (code 12: kHz in 8 bits, 14: tens of Hz in 16) in every other frame —
    the CRC-8 moves by one or two bytes —, from the table in the frames between"""
    pcm = _tonal(256 * 10 + 3, 16, sr % 97, ch=1)
    plan = lambda fi: dict(sr_code=code if fi % 2 == 0 else None)
    return Stream(FW.encode(pcm, sr, 16, blocksize=256, plan=plan), pcm, sr, 16)


@functools.lru_cache(maxsize=None)
def rice_forced(k, rice2):
    """every Rice partition with parameter k.  0 and 1: order-0 residuals of +-200, unary runs of hundreds of zeros, ~25 KB per
    256-sample stereo frame.  14 (Rice) and 30 (Rice2): the largest parameters, every code is remainder bits"""
    rng = np.random.default_rng(60 + k)
    if k <= 1:
        pcm = rng.integers(-200, 201, (256 * 20, 2)).astype(np.int64)
        plan = lambda fi: dict(kind="fixed0", rice_k=k, rice2=rice2, escape=False, stereo="indep")
    else:
        pcm = _tonal(256 * 20 + 9, 16, 60 + k)
        plan = lambda fi: dict(rice_k=k, rice2=rice2, escape=False)
    return Stream(FW.encode(pcm, 44100, 16, blocksize=256, plan=plan), pcm, 44100, 16)


@functools.lru_cache(maxsize=None)
def escape_zero(esc0=True):
    """silent stretches of 300 samples in frames of 1024 with 8 partitions: some partitions — not whole subframes — hold only
    zero residuals and are written as escapes of 0 bits (esc0=False: the same signal without them, to compare the bytes)"""
    pcm = _tonal(1024 * 12 + 100, 16, 70)
    for at in range(500, len(pcm) - 400, 1400):
        pcm[at : at + 300] = 0
    plan = lambda fi: dict(porder=3, escape=False, esc0=esc0)
    return Stream(FW.encode(pcm, 44100, 16, blocksize=1024, plan=plan), pcm, 44100, 16)


# ---- frame headers inside the payload ----------------------------------------------------------------------------------------
def fake_header(number, variable=False, bs_code=8, sr_code=9, ch_code=0, sz_code=4):
    """A frame header as RFC 9639 9.1 lays it out — sync code, blocking strategy, block-size and sample-rate codes from the
    tables (8 = 256 samples, 9 = 44.1 kHz), channel and sample-size codes (0 = mono, 4 = 16 bits), the coded number, the
    CRC-8 — padded with one byte to an even length if need be, so that it can be written as big-endian 16-bit samples: six
    bytes for a one-byte number."""
    h = bytes([0xFF, 0xF8 | int(variable), (bs_code << 4) | sr_code, (ch_code << 4) | (sz_code << 1)]) + FW._utf8(number)
    h += bytes([FW.crc8(h)])
    return h + b"\x01" * (len(h) % 2)


def header_at(data, pos, bits, channels, max_block):
    """The frame header rules of RFC 9639 9.1 restated: (variable, number, block size, length with the CRC-8) if the bytes at
    `pos` are a sync code followed by a header without reserved values that fits the stream and whose CRC-8 is right."""
    d = data[pos : pos + 16]
    if len(d) < 6 or d[0] != 0xFF or d[1] & 0xFE != 0xF8 or d[3] & 1:
        return None
    bs_code, sr_code, ch_code, sz_code = d[2] >> 4, d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
    if bs_code == 0 or sr_code == 15 or ch_code > 10 or sz_code == 3:
        return None
    extra = 0 if d[4] < 0x80 else 8 - (d[4] ^ 0xFF).bit_length() - 1
    if not 0 <= extra <= 6 or d[4] & 0xC0 == 0x80 or len(d) < 5 + extra:
        return None
    number = d[4] & (0x7F if extra == 0 else 0x3F >> extra)
    for b in d[5 : 5 + extra]:
        if b & 0xC0 != 0x80:
            return None
        number = (number << 6) | (b & 0x3F)
    p = 5 + extra
    tail = {6: 1, 7: 2}.get(bs_code, 0) + {12: 1, 13: 2, 14: 2}.get(sr_code, 0)
    if len(d) < p + tail + 1:
        return None
    if bs_code in (6, 7):
        bs = int.from_bytes(d[p : p + bs_code - 5], "big") + 1
    else:
        bs = 192 if bs_code == 1 else 576 << (bs_code - 2) if bs_code <= 5 else 256 << (bs_code - 8)
    p += tail
    size = {0: bits, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}[sz_code]
    if size != bits or (ch_code + 1 if ch_code < 8 else 2) != channels or bs > max_block or FW.crc8(d[:p]) != d[p]:
        return None
    return bool(d[1] & 1), number, bs, p + 1


PLANTED = ("stray", "stray_late", "continues", "pair", "flood", "variable_stray", "variable_continues", "continues_long")


def planted_shape(case):
    """(block size, frames) of planted(case)"""
    return (4096, 6) if case == "flood" else (4096, 11) if case == "continues_long" else (256, 12)


@functools.lru_cache(maxsize=None)
def planted(case):
    """Mono 16-bit streams of verbatim frames (the payload is byte-aligned: the samples ARE the file's bytes) with frame
    headers written into the samples of one frame; one odd sample per frame, so that no wasted bits shift the payload, and
    positive samples everywhere else, so that no other sample starts with 0xff.  `plants`: (frame, sample in the frame,
    header bytes, number) per planted header.  12 frames of 256 samples (flood: 6 of 4096, continues_long: 11 of 4096):
      stray           number 100 in frame 5: neither continues frame 5 nor is continued by frame 6
      stray_late      the same in the next-to-last frame: the last frame's predecessor in the file is the false one
      continues       number 6 in frame 5: the number frame 5's successor carries
      pair            numbers 90 and 91 back to back: they continue each other
      flood           600 headers in one frame of 4096: more than a scan chunk's list of 512 candidates holds
      variable_*      stray / continues in a variable-block-size stream: the number is a sample number, a successor's is its
                      predecessor's plus the predecessor's block size (frame 5 starts at 1280: 1536, a two-byte number)
      continues_long  "continues" in a second of a 440 Hz tone (11 frames of 4096): long enough to hold a note, so that the
                      whole-path comparisons are of events and files that are not empty"""
    var = case.startswith("variable")
    bs, nf = planted_shape(case)
    rng = np.random.default_rng(len(case))
    n = bs * nf
    if case == "continues_long":
        pcm = (9000 + 8000 * np.sin(2 * np.pi * 440 / 44100 * np.arange(n)) + rng.integers(0, 500, n)).astype(np.int64)[:, None]
    else:
        pcm = (9000 + 6000 * np.sin(np.arange(n) * 0.05) + rng.integers(0, 2000, n)).astype(np.int64)[:, None]
    pcm[::bs] |= 1
    where = {"stray": [(5, 100)], "stray_late": [(nf - 2, 100)], "continues": [(5, 6)], "continues_long": [(5, 6)], "pair": [(5, 90), (5, 91)],
             "flood": [(2, 100)] * 600, "variable_stray": [(5, 100)], "variable_continues": [(5, 5 * bs + bs)]}[case]
    plants, at = [], 40
    for frame, number in where:
        h = fake_header(number, variable=var, bs_code=8)
        pcm[frame * bs + at : frame * bs + at + len(h) // 2, 0] = np.frombuffer(h, ">i2")
        plants.append((frame, at, h, number))
        at += len(h) // 2
    plan = lambda fi: dict(kind="verbatim")
    data = FW.encode(pcm, 44100, 16, blocksize=bs, plan=plan, sizes=[bs] if var else None)
    return Stream(data, pcm, 44100, 16, tuple(plants))


def check_planted(st, bs):
    """The planted bytes are where they should be and ARE headers — otherwise a test on them tests nothing.  Walks the real
    frames by arithmetic (a verbatim mono 16-bit frame is its header, one subframe header byte, 2 bytes per sample and the
    CRC-16), finds each plant at its offset, and counts every position of the file that passes header_at(): the real frames
    and the planted ones, nothing else.  Returns the offsets of the real frames."""
    data = st.data
    pos = data.index(b"fLaC") + 4 + 4 + 34 + 4 + 16  # STREAMINFO and the encoder's PADDING block
    starts, done = [], 0
    while pos < len(data):
        hdr = header_at(data, pos, 16, 1, bs)
        assert hdr is not None and hdr[1] == (done if hdr[0] else len(starts)), (pos, hdr)
        starts.append((pos, hdr[3]))
        pos += hdr[3] + 1 + 2 * hdr[2] + 2
        done += hdr[2]
    assert pos == len(data) and done == len(st.pcm)
    for frame, at, h, number in st.plants:
        off = starts[frame][0] + starts[frame][1] + 1 + 2 * at
        assert data[off : off + len(h)] == h, (frame, at)
        got = header_at(data, off, 16, 1, bs)
        assert got is not None and got[:3] == (bool(h[1] & 1), number, 256) and got[3] in (len(h) - 1, len(h)), got
    hits = [p for p in range(starts[0][0], len(data) - 5) if data[p] == 0xFF and header_at(data, p, 16, 1, bs)]
    assert len(hits) == len(starts) + len(st.plants), (len(hits), len(starts), len(st.plants))
    return [s for s, _ in starts]
