"""The CQT front end and the whole path across input level: digital silence, quiet tones and noise down to -120 dBFS,
16-bit dither and fades, lead-in / tail shapes, DC, clipped and over-range noise, int16-scale input
(tests/level_windows.py).  The rest of the suite feeds -40 .. 0 dBFS only, where a flush of f16 subnormals in the
split-f16 operands stays inside its gates; the bounds here are the ones test_host_cpu.py shows to
reject that flush on every quiet window.  Inputs at or above 65504 are out of scope: there the f16 hi of the split
overflows by design.  -s prints a per-window table."""
import ctypes as C

import numpy as np
import pytest
import torch

import level_windows as L
from oracle import bp_oracle as O

pytestmark = pytest.mark.gpu

F32 = torch.float32
KEYS = ("note", "onset", "contour")


def _oracle(ws, weights, ext):
    x = np.stack([w for _, w, _ in ws])
    r64 = O.forward(x.astype(np.float64), weights, np.float64, intermediates=True, ext=ext)
    r32 = O.forward(x, weights, np.float32, intermediates=True, ext=ext)
    return x, r32, r64


@pytest.fixture(scope="module")
def lv22(weights):
    ws = L.windows_22k()
    return (ws,) + _oracle(ws, weights, False)


@pytest.fixture(scope="module")
def lv44(weights):
    ws = L.windows_44k()
    return (ws,) + _oracle(ws, weights, True)


def _win(r, i):
    return {k: r[k][i] for k in KEYS}


def _ext_layout(lib):
    """(offset, length) of the extended mode's pyramid levels 1..9 in its 87,556-float row: level 1 (the 22.05 kHz
    signal, 43,844 samples) at 0, level k >= 2 at 43,844 + the default layout's offset of level k - 1 (bp_api.hip
    pyr_level_off)."""
    lay = {1: (0, 43844)}
    for k in range(2, 10):
        off, ln = C.c_int64(), C.c_int64()
        assert lib.bp_pyramid_layout(k - 1, C.byref(off), C.byref(ln)) == 0
        lay[k] = (43844 + off.value, ln.value)
    return lay


EXT_PYR_STRIDE = 87556


def _stages(runner, x, r32, ext):
    """pyramid and filterbank of the handle on x; the filterbank fed with the oracle's fp32 levels"""
    from stage_harness import pyr_pack, pyr_unpack

    n = x.shape[0]
    if ext:
        lay = _ext_layout(runner.lib)
        pyr = runner.run("pyramid", n, {"audio": x}, {"pyr": ((n, EXT_PYR_STRIDE), F32)})["pyr"]
        levels = [None] + [pyr[:, o : o + ln] for o, ln in (lay[k] for k in range(1, 10))]
        feed = np.zeros((n, EXT_PYR_STRIDE), np.float32)
        for k in range(1, 10):
            o, ln = lay[k]
            assert r32["levels"][k].shape[1] == ln
            feed[:, o : o + ln] = r32["levels"][k]
    else:
        pyr = runner.run("pyramid", n, {"audio": x}, {"pyr": ((n, 43712), F32)})["pyr"]
        levels = pyr_unpack(pyr, runner.lib)
        feed = pyr_pack(r32["levels"], runner.lib)
    nb = r32["lp"].shape[2]
    fb = runner.run("filterbank", n, {"audio": x, "pyr": feed}, {"lp": ((n, 172, nb), F32), "mm": ((n, 2), torch.int32)})
    return levels, fb["lp"], fb["mm"]


def _check_stages(ws, x, r32, r64, levels, lp, mm, tag):
    """Per window: pyramid, filterbank magnitudes and log-power against fp64, extrema of the log-power, silence exact."""
    from stage_harness import ord_decode

    assert np.isfinite(lp).all(), tag
    mag = np.sqrt(np.maximum(10.0 ** (lp.astype(np.float64) / 10.0) - L.LP_EPS, 0))
    mmd = ord_decode(mm)
    print(f"\n{tag}: stage errors as fractions of their bounds (<= 1 passes); the fp32 oracle's in brackets")
    print(f"{'window':20s} {'peak':>9s} {'pyramid':>15s} {'magnitude':>15s} {'log-power':>15s}   max|dlp| dB [fp32]  lp64 range dB")
    bad = []
    for i, (name, w, quiet) in enumerate(ws):
        pk = float(np.abs(w).max())
        ep = L.pyramid_excess([lv[i] for lv in levels[1:]], [lv[i] for lv in r64["levels"][1:]], pk)
        ep32 = L.pyramid_excess([lv[i] for lv in r32["levels"][1:]], [lv[i] for lv in r64["levels"][1:]], pk)
        em, em32 = L.mag_excess(mag[i], r64["mag"][i]), L.mag_excess(r32["mag"][i], r64["mag"][i])
        el, el32 = L.lp_excess(lp[i], r64["lp"][i], r64["mag"][i]), L.lp_excess(r32["lp"][i], r64["lp"][i], r64["mag"][i])
        dl, dl32 = np.abs(lp[i] - r64["lp"][i]).max(), np.abs(r32["lp"][i] - r64["lp"][i]).max()
        print(f"{name:20s} {pk:9.2e} {ep:6.2f} [{ep32:6.2f}] {em:6.2f} [{em32:6.2f}] {el:6.2f} [{el32:6.2f}]   {dl:8.2e} "
              f"[{dl32:8.2e}]  {np.ptp(r64['lp'][i]):9.2e}")
        assert mmd[i, 0] == lp[i].min() and mmd[i, 1] == lp[i].max(), (tag, name)
        if name.startswith("DC"):
            # a constant window is all cancellation: every bin but the lowest few is fp32 rounding noise of the same
            # size in the fp32 oracle (1.3 x the magnitude bound there) -- held to 2 x what the oracle itself does
            em, el = em / max(1.0, 2.0 * em32), el / max(1.0, 2.0 * el32)
        if max(ep, em, el) > 1.0:
            bad.append((name, ep, em, el))
        if name == "silence":
            # every bin of a silent window evaluates to the one value v0 = 10 log10(eps): the range is exactly 0
            v0 = lp[i].flat[0]
            assert (lp[i].view(np.int32) == v0.view(np.int32)).all(), tag
            assert mmd[i, 0].view(np.int32) == mmd[i, 1].view(np.int32) == v0.view(np.int32), tag
            assert abs(float(v0) - 10.0 * np.log10(L.LP_EPS)) <= 1e-4, (tag, v0)
    assert not bad, (tag, bad)


def test_front_end_stages_across_levels(lv22):
    """Pyramid and filterbank of the default path on every level window.  Measured on MI355X, as fractions of the
    bounds of level_windows.py: pyramid <= 0.28, magnitude <= 0.34, log-power <= 0.28, except DC (1.46 / 1.37, where the
    fp32 oracle itself is at 1.30 / 1.23 and the gate is 2 x the oracle's).  With f16 subnormals flushed in the operand
    split the quiet windows breach the pyramid bound 12x .. 50x."""
    from stage_harness import StageRunner

    ws, x, r32, r64 = lv22
    runner = StageRunner()
    levels, lp, mm = _stages(runner, x, r32, False)
    _check_stages(ws, x, r32, r64, levels, lp, mm, "22.05 kHz")
    runner.model.close()


def test_extended_mode_stages_across_levels(lv44):
    """The extended mode's 10-level pyramid and 345-bin filterbank on the device against O.forward(ext=True).  Measured
    on MI355X: pyramid <= 0.25, magnitude <= 0.24, log-power <= 0.23 of the bounds."""
    from basic_pitch_amd import Model
    from stage_harness import StageRunner

    ws, x, r32, r64 = lv44
    runner = StageRunner(Model(max_windows=8, ext_cqt_44k=True))
    levels, lp, mm = _stages(runner, x, r32, True)
    assert lp.shape == (len(ws), 172, 345)
    _check_stages(ws, x, r32, r64, levels, lp, mm, "44.1 kHz extended")
    runner.model.close()


def _two_regimes(x, **kw):
    """predict on a small handle (strided filterbank, zpack, wide decimators) and on a handle launched with at least a
    window for every second CU (one-launch pyramid, fused filterbank + normalise); both results, which must agree"""
    from basic_pitch_amd import Model

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = x.shape[0]
    reps = -(-max(n_cu // 2 + 1, n) // n)
    small = Model(max_windows=8, **kw)
    a = small.predict(x)
    small.close()
    big = Model(max_windows=reps * n, **kw)
    b = big.predict(np.concatenate([x] * reps))
    big.close()
    for k in KEYS:
        for r in range(reps):
            assert np.array_equal(a[k], b[k][r * n : (r + 1) * n]), (kw, k, r)
    return a


def _report_and_gate(ws, got, r32, r64, tag):
    print(f"\n{tag}: whole path per window")
    print(f"{'window':20s} {'|hip-fp64|':>11s} {'|fp32-fp64|':>12s} {'|hip-fp32|':>11s}  gate")
    bad = []
    for i, (name, w, quiet) in enumerate(ws):
        g = _win(got, i)
        for k in KEYS:
            assert np.isfinite(g[k]).all(), (tag, name, k)
        h64, o64, h32 = L.out_err(g, _win(r64, i)), L.out_err(_win(r32, i), _win(r64, i)), L.out_err(g, _win(r32, i))
        if quiet:
            gate, what = L.QUIET_GATE, "quiet"
        elif o64 <= L.TIGHT_FP32:
            gate, what = L.TIGHT_GATE, "tight"
        else:
            gate, what = max(L.NORTH_STAR, 2.0 * o64), "noise-aware"
        print(f"{name:20s} {h64:11.2e} {o64:12.2e} {h32:11.2e}  {what} {gate:.1e}")
        if h64 > gate:
            bad.append((name, h64, gate))
    assert not bad, (tag, bad)


def test_level_windows_both_regimes_and_oracle(lv22):
    """Every level window through predict on both dispatch regimes (bit-equal), then against the fp64 / fp32 oracles:
    quiet windows (<= -60 dBFS) to QUIET_GATE, windows whose fp32 oracle is within 2e-5 of fp64 to the plain 1e-4, the
    rest (DC, fades, lead-in / tail, over-range and int16-scale noise) to the noise-aware bound.  The reference
    normalises each window, so int16-scale input follows the oracle like any other.  Measured on MI355X: quiet <= 1.7e-5
    (-120 dBFS tone), tight <= 9.9e-6, and every noise-aware window closer to fp64 than the fp32 oracle."""
    ws, x, r32, r64 = lv22
    got = _two_regimes(x)
    _report_and_gate(ws, got, r32, r64, "22.05 kHz")


def test_extended_mode_level_windows_both_regimes_and_oracle(lv44):
    """The same in the extended mode.  Measured on MI355X: quiet <= 3.5e-6, lead-in 9.9e-5 (fp32 oracle 2.0e-4)."""
    ws, x, r32, r64 = lv44
    got = _two_regimes(x, ext_cqt_44k=True)
    _report_and_gate(ws, got, r32, r64, "44.1 kHz extended")


def _silence_chain(model, n_bins, bn_b):
    """contour -> note -> onset of the handle's own stage hook on the packed constant map z = bn_b (n_bins bins)"""
    from stage_harness import StageRunner, zp_pack

    runner = StageRunner(model)
    zp = zp_pack(np.full((1, 172, n_bins), bn_b, np.float32)).view(np.int32)
    contour = runner.run("contour", 1, {"zp": zp}, {"contour": ((1, 172, 264), F32)})["contour"]
    note = runner.run("note", 1, {"contour": contour}, {"note": ((1, 172, 88), F32)})["note"]
    onset = runner.run("onset", 1, {"zp": zp, "note": note}, {"onset": ((1, 172, 88), F32)})["onset"]
    return {"contour": contour, "note": note, "onset": onset}


@pytest.mark.parametrize("mode", ["default", "ext_cqt_44k", "bf16_weights"])
def test_silent_window_is_the_constant_map_exactly(weights, mode):
    """A silent window normalises to z = bn_b exactly (range 0: divide_no_nan's constant map), so its posteriorgrams are
    bit for bit the stage chain on that constant map -- alone (n = 1, the strided filterbank + zpack) and inside a
    fused batch (a window for every second CU) -- and within 1e-5 of fp64 (bf16 weights: its own stage chain only)."""
    from basic_pitch_amd import Model

    kw = {} if mode == "default" else {mode: True}
    ext = mode == "ext_cqt_44k"
    n_s = O.EXT_AUDIO_N_SAMPLES if ext else O.AUDIO_N_SAMPLES
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    bn_b = np.float32(weights["bn_affine"][1])
    m = Model(max_windows=n_cu, **kw)
    n_bins = 345 if ext else 309
    want = _silence_chain(m, n_bins, bn_b)
    alone = m.predict(np.zeros((1, n_s), np.float32))
    rng = np.random.default_rng(3)
    xb = rng.uniform(-1, 1, (n_cu, n_s)).astype(np.float32)
    xb[[0, n_cu // 2, n_cu - 1]] = 0.0
    batch = m.predict(xb)
    m.close()
    for k in KEYS:
        assert np.array_equal(alone[k], want[k]), (mode, k, float(np.abs(alone[k] - want[k]).max()))
        for i in (0, n_cu // 2, n_cu - 1):
            assert np.array_equal(batch[k][i], want[k][0]), (mode, k, i)
    if mode != "bf16_weights":
        r64 = O.forward(np.zeros((1, n_s)), weights, np.float64, ext=ext)
        err = L.out_err(_win(alone, 0), _win(r64, 0))
        print(f"silence ({mode}): |hip - fp64| = {err:.2e}")
        assert err <= 1e-5, (mode, err)


def test_quiet_track(weights):
    """A 16-bit track of silence, a fade from -100 to -20 dBFS, a 3 s gap and a dither tail, through predict_track and as
    16-bit PCM through predict_pcm_raw, against O.run_track at fp64 / fp32 with the noise-aware bound.  Measured on
    MI355X: 6.2e-5 from fp64 (fp32 oracle 1.25e-4); the two entry points agree bit for bit."""
    from basic_pitch_amd import Model, _native
    from test_gpu_parity import _noise_aware

    y = L.quiet_track()
    assert O.window_track(y)[0].shape[0] >= 4
    m = Model(max_windows=8)
    a = m.predict_track(y)
    pcm = np.round(y * 32768.0).astype(np.int16)
    b = m.predict_pcm_raw(pcm.tobytes(), _native.BP_PCM_S16, len(pcm), 1, 22050)
    m.close()
    r64 = O.run_track(y, weights, np.float64)
    r32 = O.run_track(y, weights, np.float32)
    for name, got in (("track", a), ("pcm s16", b)):
        for k in KEYS:
            assert got[k].shape == r64[k].shape, (name, k)
        print(f"quiet track, {name}: |hip-fp64| {L.out_err(got, r64):.2e}, |fp32-fp64| {L.out_err(r32, r64):.2e}, "
              f"|track - pcm| {L.out_err(a, b):.2e}")
        _noise_aware(got, r32, r64)
        for k in KEYS:
            assert np.array_equal(got[k], a[k]), (name, k)
