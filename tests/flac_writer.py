"""Test-side FLAC *encoder* written from the format specification (RFC 9639), used to make inputs for the product's
decoder (basic_pitch_amd/csrc/flac_decode.cpp).  Deliberately exercises every decoder branch: constant / verbatim /
fixed (orders 0-4) / LPC subframes, wasted bits, Rice and Rice2 residuals with several partition orders and escaped
partitions, independent / left-side / side-right / mid-side stereo, variable last block, 8 / 16 / 24-bit samples.
Frames carry valid CRC-8 / CRC-16 and STREAMINFO the MD5 of the PCM, so the decoder's integrity checks are live.

On request it also leaves the one operating point a simple encoder sits on: the precision and shift of the LPC
coefficients, a forced Rice parameter, escaped partitions of 0 bits, the sample-rate codes 12 and 14, and variable-block-size
streams (`encode(sizes=...)`).  No real encoder was at hand to anchor the variable-block-size coding against: it is a
restatement of RFC 9639 section 9.1.1 (blocking strategy bit) and 9.1.5 (coded number) as read from the RFC's text, not from
the decoders under test, and the tests that use it are written from the same text.
"""
import hashlib
import struct

import numpy as np


class BitWriter:
    def __init__(self):
        self.acc, self.nbits, self.out = 0, 0, bytearray()

    def write(self, value, bits):
        if bits == 0:
            return
        self.acc = (self.acc << bits) | (int(value) & ((1 << bits) - 1))
        self.nbits += bits
        while self.nbits >= 8:
            self.nbits -= 8
            self.out.append((self.acc >> self.nbits) & 0xFF)
        self.acc &= (1 << self.nbits) - 1

    def unary(self, q):
        while q >= 32:
            self.write(0, 32)
            q -= 32
        self.write(1, q + 1)

    def align(self):
        if self.nbits:
            self.write(0, 8 - self.nbits)

    def bytes(self):
        assert self.nbits == 0
        return bytes(self.out)


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data):
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def _utf8(n):
    if n < 0x80:
        return bytes([n])
    out, lead_bits = [], 6
    while n >= (1 << lead_bits):
        out.append(0x80 | (n & 0x3F))
        n >>= 6
        lead_bits -= 1
    lead = (0xFF << (lead_bits + 1)) & 0xFF
    return bytes([lead | n] + out[::-1])


def _zigzag(r):
    return [(v << 1) if v >= 0 else ((-v) << 1) - 1 for v in r]


def _write_residual(bw, res, order, blocksize, porder, rice2, escape, rice_k=None, esc0=False):
    bw.write(1 if rice2 else 0, 2)
    bw.write(porder, 4)
    pbits, esc = (5, 31) if rice2 else (4, 15)
    pos = 0
    for p in range(1 << porder):
        count = (blocksize >> porder) - (order if p == 0 else 0)
        part = res[pos : pos + count]
        pos += count
        if escape and p % 2 == 1:
            raw = max([1] + [int(v).bit_length() + 1 for v in part])
            bw.write(esc, pbits)
            bw.write(raw, 5)
            for v in part:
                bw.write(v, raw)
            continue
        if esc0 and not any(part):
            # RFC 9639 9.2.7.1: an escaped partition may hold 0 bits per residual: every residual of it is 0
            bw.write(esc, pbits)
            bw.write(0, 5)
            continue
        u = _zigzag(part)
        mean = (sum(u) / len(u)) if u else 0
        k = max(0, min(esc - 1, int(mean).bit_length() - 1 if mean >= 1 else 0))
        if rice_k is not None:  # RFC 9639 9.2.7.1 / 9.2.7.2: any parameter below the escape code (0..14, Rice2 0..30) is valid
            k = max(0, min(esc - 1, int(rice_k)))
        bw.write(k, pbits)
        for v in u:
            bw.unary(v >> k)
            bw.write(v & ((1 << k) - 1), k)
    assert pos == len(res)


_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _subframe(bw, s, bps, kind, porder=0, rice2=False, escape=False, lpc_order=8, prec=12, shift=9, rice_k=None, esc0=False,
              coefs=None, log=None):
    s = [int(v) for v in s]
    n = len(s)
    wasted = 0
    if kind != "constant" and any(s):
        while all((v >> wasted) & 1 == 0 for v in s):
            wasted += 1
    if wasted:
        s = [v >> wasted for v in s]
        bps -= wasted
    if kind == "constant":
        assert all(v == s[0] for v in s)
        code = 0
    elif kind == "verbatim":
        code = 1
    elif kind.startswith("fixed"):
        order = int(kind[5:])
        code = 8 + order
    else:
        order = lpc_order
        code = 31 + order
    bw.write(0, 1)
    bw.write(code, 6)
    if wasted:
        bw.write(1, 1)
        bw.unary(wasted - 1)
    else:
        bw.write(0, 1)
    if kind == "constant":
        bw.write(s[0], bps)
    elif kind == "verbatim":
        for v in s:
            bw.write(v, bps)
    elif kind.startswith("fixed"):
        c = _FIXED[order]
        for v in s[:order]:
            bw.write(v, bps)
        res = [s[i] - sum(c[j] * s[i - 1 - j] for j in range(order)) for i in range(order, n)]
        _write_residual(bw, res, order, n, porder, rice2, escape, rice_k, esc0)
    else:
        x = np.asarray(s, dtype=np.float64)
        r = np.array([np.dot(x[: n - l], x[l:]) for l in range(order + 1)])
        r[0] = r[0] * (1 + 1e-9) + 1e-9
        a = np.zeros(order)
        err = r[0]
        for i in range(order):  # Levinson-Durbin
            k = (r[i + 1] - np.dot(a[:i], r[i:0:-1])) / err
            a[:i], a[i] = a[:i] - k * a[:i][::-1], k
            err *= 1 - k * k
        # RFC 9639 9.2.6: precision 1..15 bits (the 4-bit field holds precision - 1, 0b1111 is invalid), the shift a 5-bit
        # signed field that must not be negative; coefficients beyond the precision's range saturate
        assert 1 <= prec <= 15 and 0 <= shift <= 15
        q = np.clip(np.round(a * (1 << shift)), -(1 << (prec - 1)), (1 << (prec - 1)) - 1).astype(np.int64)
        if coefs is not None:  # the caller's own quantised coefficients, cycled over the order, instead of the fitted ones
            q = np.array([int(coefs[j % len(coefs)]) for j in range(order)], dtype=np.int64)
            assert all(-(1 << (prec - 1)) <= int(v) < (1 << (prec - 1)) for v in q)
        for v in s[:order]:
            bw.write(v, bps)
        bw.write(prec - 1, 4)
        bw.write(shift, 5)
        for v in q:
            bw.write(int(v), prec)
        sums = [sum(int(q[j]) * s[i - 1 - j] for j in range(order)) for i in range(order, n)]
        res = [s[i] - (sums[i - order] >> shift) for i in range(order, n)]
        assert all(-(1 << 31) < v < (1 << 31) for v in res)  # RFC 9639 9.2.7.3: a residual fits a 32-bit signed integer
        if log is not None:
            log.append(([int(v) for v in q], max([abs(v) for v in sums] + [0])))
        _write_residual(bw, res, order, n, porder, rice2, escape, rice_k, esc0)


def encode(pcm, sample_rate, bits, blocksize=1152, plan=None, total_in_header=True, md5_in_header=True, id3=False,
           sizes=None):
    """pcm: int array [n, channels].  plan(frame_index) -> dict(kind=..., stereo="indep"|"ls"|"sr"|"ms", porder=..,
    rice2=.., escape=.., lpc_order=1..32) chooses how each frame is coded (cycled defaults exercise everything); it may
    also give prec=1..15 and shift=0..15 (LPC coefficients), rice_k (the parameter of every Rice partition), esc0=True
    (an all-zero partition becomes an escape of 0 bits), sr_code=12|14 (the rate at the header's end, in kHz / in tens
    of Hz), coefs=[...] (quantised LPC coefficients of the caller's choice, cycled over the order, in place of the fitted
    ones) and log=a list, to which every LPC subframe written appends (its coefficients, its largest |sum of products|).  sizes=[...]: a variable-block-size stream whose block sizes cycle through the list, the last block short."""
    pcm = np.asarray(pcm, dtype=np.int64)
    n, ch = pcm.shape
    if sizes:
        starts, at = [], 0
        while at < n:
            at += int(sizes[len(starts) % len(sizes)])
            starts.append(at)
        starts = [0] + starts[:-1]
        lo_block, hi_block = min(sizes), max(sizes)  # RFC 9639 8.2: STREAMINFO's minimum and maximum block size
    else:
        starts = list(range(0, n, blocksize))
        lo_block = hi_block = blocksize
    kinds = ["fixed2", "lpc", "fixed0", "fixed1", "verbatim", "fixed3", "fixed4", "lpc"]
    stereos = ["indep", "ms", "ls", "sr"]
    frames = bytearray()
    for fi, start in enumerate(starts):
        blk = pcm[start : (starts[fi + 1] if fi + 1 < len(starts) else n)]
        bs = len(blk)
        p = dict(kind=kinds[fi % len(kinds)], stereo=stereos[fi % 4] if ch == 2 else "indep", porder=fi % 3,
                 rice2=bool(fi % 2), escape=(fi % 5 == 4))
        if plan:
            p.update(plan(fi) or {})
        while p["porder"] and (bs % (1 << p["porder"]) or (bs >> p["porder"]) < 33):
            p["porder"] -= 1
        chans = [blk[:, c] for c in range(ch)]
        widths = [bits] * ch
        ch_code = ch - 1
        if ch == 2 and p["stereo"] != "indep":
            l, r = chans
            side = l - r
            if p["stereo"] == "ls":
                chans, widths, ch_code = [l, side], [bits, bits + 1], 8
            elif p["stereo"] == "sr":
                chans, widths, ch_code = [side, r], [bits + 1, bits], 9
            else:
                chans, widths, ch_code = [(l + r) >> 1, side], [bits, bits + 1], 10
        bw = BitWriter()
        bw.write(0b11111111111110, 14)
        bw.write(0, 1)
        # RFC 9639 9.1.1 blocking strategy: 0 = fixed block size, the frame number is coded; 1 = variable block size, the
        # number of the frame's first sample is coded
        bw.write(1 if sizes else 0, 1)
        bs_code = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12}.get(bs)
        if bs_code is None:
            bs_code = 6 if bs <= 256 else 7
        bw.write(bs_code, 4)
        sr_code = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
                   96000: 11}.get(sample_rate, 0 if fi % 2 else 13 if sample_rate < 65536 else 0)
        if p.get("sr_code") is not None:  # RFC 9639 9.1.2: 0b1100 = 8 bits of kHz, 0b1110 = 16 bits of tens of Hz behind the number
            sr_code = int(p["sr_code"])
            assert (sr_code == 12 and sample_rate % 1000 == 0 and sample_rate // 1000 < 256) or \
                   (sr_code == 14 and sample_rate % 10 == 0 and sample_rate // 10 < 65536), (sr_code, sample_rate)
        bw.write(sr_code, 4)
        bw.write(ch_code, 4)
        bw.write({8: 1, 12: 2, 16: 4, 20: 5, 24: 6}.get(bits, 0) if fi % 3 else 0, 3)
        bw.write(0, 1)
        for b in _utf8(start if sizes else fi):  # RFC 9639 9.1.5: the coded number, in the extended UTF-8 form
            bw.write(b, 8)
        if bs_code == 6:
            bw.write(bs - 1, 8)
        elif bs_code == 7:
            bw.write(bs - 1, 16)
        if sr_code == 12:
            bw.write(sample_rate // 1000, 8)
        elif sr_code == 13:
            bw.write(sample_rate, 16)
        elif sr_code == 14:
            bw.write(sample_rate // 10, 16)
        bw.write(crc8(bw.bytes()), 8)
        for c, (x, w) in enumerate(zip(chans, widths)):
            kind = p["kind"]
            if len(set(int(v) for v in x)) == 1:
                kind = "constant"
            elif kind == "lpc" and bs <= 40:
                kind = "fixed2"
            elif kind.startswith("fixed") and bs <= int(kind[5:]):
                kind = "verbatim"
            _subframe(bw, x, w, kind, p["porder"], p["rice2"], p["escape"], lpc_order=int(p.get("lpc_order", 8)),
                      prec=int(p.get("prec", 12)), shift=int(p.get("shift", 9)), rice_k=p.get("rice_k"),
                      esc0=bool(p.get("esc0", False)), coefs=p.get("coefs"), log=p.get("log"))
        bw.align()
        body = bw.bytes()
        frames += body + struct.pack(">H", crc16(body))
    bytes_per = (bits + 7) // 8
    # little-endian, interleaved, ceil(bits / 8) bytes per sample (RFC 9639 8.2): the low bytes of the 32-bit words, cut out
    # by numpy (a to_bytes() per sample takes seconds on the streams of millions of samples)
    raw = pcm.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :bytes_per].tobytes()
    md5 = hashlib.md5(raw).digest() if md5_in_header else b"\0" * 16
    total = n if total_in_header else 0
    si = struct.pack(">HH", lo_block, hi_block) + b"\0\0\0" + b"\0\0\0"
    packed = (sample_rate << 44) | ((ch - 1) << 41) | ((bits - 1) << 36) | total
    si += packed.to_bytes(8, "big") + md5
    out = bytearray()
    if id3:
        out += b"ID3\x04\x00\x00" + bytes([0, 0, 0, 10]) + b"\0" * 10
    out += b"fLaC" + bytes([0x00]) + len(si).to_bytes(3, "big") + si
    pad = b"\0" * 16
    out += bytes([0x81]) + len(pad).to_bytes(3, "big") + pad  # PADDING block, last
    return bytes(out + frames)
