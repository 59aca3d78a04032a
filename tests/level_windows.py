"""Input-level probes of the CQT front end: seeded windows from digital silence to int16 scale, the split-f16
representation of the default path emulated in numpy, and the bounds that tests/test_gpu_levels.py holds the device to.

The default path carries every CQT operand as x = hi + lo / 2^11 with hi = rn_f16(x), lo = rn_f16((x - hi) * 2^11)
(bp_common.h split_f16x2_rn).  Below 2^-14 (6.1e-5, -84 dBFS) a sample's hi is an f16 subnormal, and
lo / 2^11 has an absolute spacing of 2^-35 once lo is subnormal: quiet audio is represented to 22 bits only while f16
subnormals survive every conversion and every matrix instruction.  split_emulate() computes that representation with IEEE
subnormals or with them flushed to zero; test_host_cpu.py checks that the bounds below accept the first and reject the
second on every quiet window, so a flush-to-zero regression on the device cannot pass test_gpu_levels.py.

Bounds are module constants so that the CPU sensitivity test and the GPU tests use the same numbers."""
from __future__ import annotations

import numpy as np

SR = 22050
N = 43844
EXT_SR = 44100
EXT_N = 87688
LEAD_IN = 3840  # zeros in front of a track's first window (inference.py:222-244)
EXT_LEAD_IN = 7680
LSB16 = 1.0 / 32768.0

# ---- bounds ------------------------------------------------------------------------------------------------------------
# Pyramid levels: |level - fp64| <= PYR_REL * peak(window) + PYR_FLOOR.  PYR_REL is the fp32 accumulation of a 256-tap
# FIR on split operands, relative to the window's peak (test_stage_pyramid's 2e-6 on O(1) data).  PYR_FLOOR is what the
# split representation may lose on a silent-ish sample: half the 2^-35 spacing of a subnormal lo / 2^11, through the sum
# of |taps| of the 256-tap low-pass (2.71), once per level of the cascade (8 levels, each gain <= 1), rounded up to 2x.
LOWPASS_ABS_SUM = 2.71
PYR_REL = 2e-6
PYR_FLOOR = 2.0 * 8 * LOWPASS_ABS_SUM * 2.0 ** -36
# Filterbank magnitudes: |mag - fp64| <= FB_MAG_REL * max(mag64 of the window) + FB_MAG_FLOOR (fp32 accumulation of
# split products relative to the window's largest bin; the floor is PYR_FLOOR through the largest kernel gain).  Checked
# on bins with mag64^2 >= eps only: the kernel writes the log-power, and a magnitude recovered from an fp32 log-power of
# a bin far below eps is ill-conditioned (one ulp of -100 dB is 1.3e-8 of magnitude at mag = 0).
FB_MAG_REL = 1e-5
FB_MAG_FLOOR = 1e-9
# Log-power, on every bin: |lp - fp64| <= FB_LP_FLOOR_DB + the magnitude bound carried into dB at that bin,
# (10 / ln 10) (2 mag64 dmag + dmag^2) / (mag64^2 + eps).  FB_LP_FLOOR_DB is the rounding of the log itself near the
# -100 dB floor: the device's log2 instruction and the per-bin constants (cqt_planes_filterbank.hip) add a few ulp of 100 dB
# (ulp 7.6e-6 dB) beside the fp32 oracle's correctly rounded log.
FB_LP_FLOOR_DB = 4e-5  # measured on MI355X: the worst bin uses 0.28 of its bound (noise at -90 dBFS)
LP_EPS = 1e-10
# Whole path on quiet windows (peak <= -60 dBFS): the posteriorgrams within QUIET_GATE of fp64.  Measured on MI355X: at
# most 1.7e-5 (-120 dBFS tone: its log-power spans 5 dB, and the normalisation amplifies the log's rounding near the
# -100 dB floor, 5.2e-5 dB on the device against the fp32 oracle's 1.6e-5; fp32 oracle 1.0e-6 end to end), <= 9.0e-6 on
# every other quiet window.  Flushing f16 subnormals costs
# 2.7e-5 .. 3.7e-4 there in the emulation (test_host_cpu.py), and the pyramid bound catches it by 13x .. 42x.
QUIET_GATE = 3e-5
# Windows whose fp32 oracle is within TIGHT_FP32 of fp64 are held to the plain north-star 1e-4 and to TIGHT_GATE
# (measured on MI355X: <= 9.9e-6, clipped full-scale noise); the others to the noise-aware bound
# max(1e-4, 2 |fp32 - fp64|) of test_gpu_parity._noise_aware.
TIGHT_FP32 = 2e-5
TIGHT_GATE = 2e-5
NORTH_STAR = 1e-4


def db(level_dbfs: float) -> float:
    return float(10.0 ** (level_dbfs / 20.0))


def _tone(n: int, sr: int, peak: float, rng, f0=None) -> np.ndarray:
    """Two partials with random phases, scaled so that max |x| = peak exactly (in fp64, before the fp32 cast)."""
    t = np.arange(n) / float(sr)
    f0 = f0 if f0 is not None else 110.0 * 2 ** (rng.integers(0, 36) / 12.0)
    x = np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6.28)) + 0.5 * np.sin(2 * np.pi * 3.01 * f0 * t + rng.uniform(0, 6.28))
    return x * (peak / np.abs(x).max())


def _q16(x: np.ndarray) -> np.ndarray:
    """16-bit quantisation: what a decoded 16-bit file holds."""
    return np.round(np.clip(x, -1.0, 1.0 - LSB16) * 32768.0) / 32768.0


def windows_22k(seed: int = 0):
    """[(name, window float32 (43844,), quiet)] at 22.05 kHz.  quiet: peak at or below -60 dBFS, where the split
    representation is weakest and the emulation-sensitivity test applies."""
    rng = np.random.default_rng(seed)
    out = []
    for lvl in (-20, -40, -60, -80, -100, -120):
        out.append((f"tone {lvl} dBFS", _tone(N, SR, db(lvl), rng), lvl <= -60))
    for lvl in (-60, -90):
        out.append((f"noise {lvl} dBFS", rng.uniform(-1, 1, N) * db(lvl), True))
    out.append(("dither +-2 LSB", rng.integers(-2, 3, N) * LSB16, True))
    env = np.linspace(0.0, 1.0, N) ** 3
    out.append(("fade 16-bit", _q16(_tone(N, SR, db(-20), rng) * env), False))
    lead = _tone(N, SR, db(-20), rng)
    lead[:LEAD_IN] = 0.0
    out.append(("lead-in", lead, False))
    tail = _tone(N, SR, db(-20), rng)
    tail[9000:] = 0.0
    out.append(("tail", tail, False))
    imp = np.zeros(N)
    imp[N // 2] = 0.5
    out.append(("impulse", imp, False))
    out.append(("silence", np.zeros(N), True))
    out.append(("DC 0.25", np.full(N, 0.25), False))
    out.append(("DC 1.0", np.full(N, 1.0), False))
    out.append(("noise clipped +-1", np.clip(rng.standard_normal(N) * 0.7, -1.0, 1.0), False))
    out.append(("noise peak 2.0", rng.uniform(-2, 2, N), False))
    out.append(("int16 scale", np.round(rng.uniform(-32767, 32767, N)), False))
    return [(n, x.astype(np.float32), q) for n, x, q in out]


def windows_44k(seed: int = 1):
    """The same idea at 44.1 kHz for the extended mode (87,688-sample windows)."""
    rng = np.random.default_rng(seed)
    out = [("silence", np.zeros(EXT_N), True)]
    for lvl in (-60, -100):
        out.append((f"tone {lvl} dBFS", _tone(EXT_N, EXT_SR, db(lvl), rng), True))
    out.append(("dither +-2 LSB", rng.integers(-2, 3, EXT_N) * LSB16, True))
    lead = _tone(EXT_N, EXT_SR, db(-20), rng)
    lead[:EXT_LEAD_IN] = 0.0
    out.append(("lead-in", lead, False))
    return [(n, x.astype(np.float32), q) for n, x, q in out]


def quiet_track(seed: int = 2) -> np.ndarray:
    """A 16-bit quantised track of five windows: digital silence, a fade from -100 to -20 dBFS, a 3 s gap, a dither tail."""
    rng = np.random.default_rng(seed)
    sil = np.zeros(SR * 2)
    n_f = SR * 3
    fade = _tone(n_f, SR, 1.0, rng, f0=330.0) * 10.0 ** (np.linspace(-100, -20, n_f) / 20.0)
    gap = np.zeros(SR * 3)
    tail = rng.integers(-1, 2, SR * 2) * LSB16
    return _q16(np.concatenate([sil, fade, gap, tail])).astype(np.float32)


# ---- the split representation ------------------------------------------------------------------------------------------
F16_MIN_NORMAL = 2.0 ** -14


def split_emulate(x: np.ndarray, ftz: bool = False) -> np.ndarray:
    """hi + lo / 2^11 of fp32 samples (bp_common.h split_f16x2_rn), returned in fp64.  ftz=False: IEEE f16 with
    subnormals (the device's conversions and f16 MFMAs); ftz=True: every f16 result below 2^-14 flushed to zero, the
    regression the level tests exist to catch."""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16)
    if ftz:
        hi = np.where(np.abs(hi) < F16_MIN_NORMAL, np.float16(0), hi)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)  # x - hi is exact in fp32
    if ftz:
        lo = np.where(np.abs(lo) < F16_MIN_NORMAL, np.float16(0), lo)
    return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


# ---- the checks both test files apply ------------------------------------------------------------------------------------
def pyramid_excess(levels, levels64, peak: float) -> float:
    """max over the given levels (1, 2, ...) of |level - fp64| / (PYR_REL * peak + PYR_FLOOR): <= 1 passes."""
    bound = PYR_REL * peak + PYR_FLOOR
    return max(float(np.abs(np.asarray(a, np.float64) - b).max()) for a, b in zip(levels, levels64)) / bound


def _dmag(mag64) -> float:
    return FB_MAG_REL * float(mag64.max()) + FB_MAG_FLOOR


def mag_excess(mag, mag64) -> float:
    """max |mag - fp64| / the magnitude bound over bins with mag64^2 >= eps: <= 1 passes."""
    live = mag64 * mag64 >= LP_EPS
    if not live.any():
        return 0.0
    return float(np.abs(np.asarray(mag, np.float64)[live] - mag64[live]).max()) / _dmag(mag64)


def lp_excess(lp, lp64, mag64) -> float:
    """max over all bins of |lp - fp64| in dB / (FB_LP_FLOOR_DB + the magnitude bound in dB at that bin)"""
    d = _dmag(mag64)
    bound = FB_LP_FLOOR_DB + (10.0 / np.log(10.0)) * (2.0 * mag64 * d + d * d) / (mag64 * mag64 + LP_EPS)
    return float((np.abs(np.asarray(lp, np.float64) - lp64) / bound).max())


def out_err(a, b) -> float:
    """max |a - b| over the three posteriorgrams of one window"""
    return max(float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()) for k in ("note", "onset", "contour"))
