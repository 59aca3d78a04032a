"""Pin the oracle: reference golden vectors (tests/golden, from the reference's own known-answer test
`tests/test_inference.py:43-76,164-194`) and the frozen-graph constants.  CPU only."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_windows
from oracle import bp_oracle as O


def test_weights_blob_tensors(weights):
    shapes = {k: v.shape for k, v in weights.items()}
    assert shapes["cqt_kernel_re"] == (36, 256) and shapes["cqt_kernel_im"] == (36, 256)
    assert shapes["cqt_lowpass"] == (256,) and shapes["cqt_sqrt_len"] == (309,)
    assert shapes["contour1_w"] == (8, 8, 3, 39) and shapes["onset2_w"] == (1, 33, 3, 3)
    assert shapes["note1_w"] == (32, 1, 7, 7) and shapes["note2_w"] == (1, 32, 7, 3)
    # folded BatchNorm affine and log constants of the frozen graph
    np.testing.assert_allclose(weights["bn_affine"], [2.480741024017334, -0.8769183158874512], rtol=0, atol=0)
    np.testing.assert_allclose(weights["log_scale"], [0.4342944622039795, 10.0], rtol=0, atol=0)
    assert abs(float(weights["log_eps"][0]) - 1e-10) < 1e-17


def test_cqt_constants_match_reference_formulas(weights):
    """nnaudio.py:45-76 (firwin2 low-pass), 158-213 (kernels), 590-593 (lengths) regenerated with scipy."""
    import scipy.signal

    sr, fmin, bpo, n_bins = 22050.0, 27.5, 36, 309
    Q = 1.0 / (2 ** (1 / bpo) - 1)
    lowpass = scipy.signal.firwin2(256, [0.0, 0.5 / 1.001, 0.5 * 1.001, 1.0], [1.0, 1.0, 0.0, 0.0]).astype(np.float32)
    assert np.array_equal(lowpass, weights["cqt_lowpass"])
    lengths = np.ceil(Q * sr / (fmin * 2.0 ** (np.arange(n_bins) / bpo)))
    assert np.array_equal(np.sqrt(lengths.astype(np.float32)), weights["cqt_sqrt_len"])
    fmax_t = fmin * 2 ** 8 * 2 ** (20 / bpo)
    fmin_t = fmax_t / 2 ** (1 - 1 / bpo)
    k = 7
    f = fmin_t * 2.0 ** (k / bpo)
    ln = np.ceil(Q * sr / f)
    start = int(np.ceil(128 - ln / 2.0)) - int(ln % 2)
    sig = scipy.signal.get_window("hann", int(ln), fftbins=True) * np.exp(np.r_[-ln // 2 : ln // 2] * 1j * 2 * np.pi * f / sr) / ln
    sig = (sig / np.linalg.norm(sig, 1)).astype(np.complex64)
    assert np.array_equal(weights["cqt_kernel_re"][k, start : start + int(ln)], sig.real)
    assert np.array_equal(weights["cqt_kernel_im"][k, start : start + int(ln)], sig.imag)


def test_windowing_known_answers(clip_22k):
    """tests/test_inference.py:164-194: 6 windows, original_length == 200607, first window = first samples."""
    assert clip_22k.shape[0] == 200607
    wins, n = O.window_track(clip_22k)
    assert n == 200607 and wins.shape == (6, O.AUDIO_N_SAMPLES)
    assert np.array_equal(wins[0][3840:], clip_22k[: O.AUDIO_N_SAMPLES - 3840])
    assert not wins[0][:3840].any()


def _golden_distance(samples_22k, weights):
    g = np.load(os.path.join(GOLDEN, "vocadito_10_model_output.npz"))
    r = O.run_track(samples_22k, weights, np.float32, batch=6)
    out = {}
    for k in ("note", "onset", "contour"):
        assert r[k].shape == g[k].shape == ((787, 88) if k != "contour" else (787, 264))
        out[k] = np.abs(r[k] - g[k])
    return out


def test_oracle_reproduces_golden_posteriorgrams(weights):
    """The reference's own known-answer test (tests/test_inference.py:66-70): vocadito_10.wav -> model_output.npz at
    atol = 1e-4.  The oracle chain = WAV decode -> oracle/soxr_oracle.py (restatement of librosa's soxr_hq resampler)
    -> oracle/bp_oracle.py in fp32.  Measured: 2.2e-5 / 4.6e-5 / 3.4e-5 max-abs (note / onset / contour)."""
    from basic_pitch_amd import audio
    from oracle import soxr_oracle as S

    pcm, sr = audio.read_wav(os.path.join(GOLDEN, "vocadito_10.wav"))
    assert sr == 44100 and pcm.shape == (401214, 1)
    d = _golden_distance(S.resample(pcm[:, 0], sr), weights)
    for k, v in d.items():
        assert v.max() <= 1e-4, (k, v.max())  # the reference's own tolerance, every element
        assert v.mean() <= 2e-6, (k, v.mean())


def test_golden_residual_is_the_resampler(weights):
    """The same graph oracle behind scipy's default polyphase design (Kaiser beta 5, the round-1 stand-in) is 1e-3 ..
    4e-3 from the golden file, with >85 % of the elements still inside 1e-4: the only thing that changed between this
    and the test above is the resampler, so the round-1 residual was the resampler and not the graph."""
    import scipy.signal

    from basic_pitch_amd import audio

    pcm, sr = audio.read_wav(os.path.join(GOLDEN, "vocadito_10.wav"))
    y = scipy.signal.resample_poly(pcm[:, 0].astype(np.float64), 1, 2).astype(np.float32)[:200607]
    d = _golden_distance(y, weights)
    assert 5e-4 <= d["note"].max() <= 5e-3 and 1e-3 <= d["onset"].max() <= 5e-3 and 1e-3 <= d["contour"].max() <= 5e-3
    for k, v in d.items():
        assert (v <= 1e-4).mean() >= 0.85, k


def test_host_resampler_equals_soxr_restatement():
    """basic_pitch_amd/audio.py (product, polyphase upfirdn) vs oracle/soxr_oracle.py (direct form) on the rate pairs
    that occur in practice; length = ceil(n * 22050 / sr) (librosa.resample)."""
    from basic_pitch_amd import audio
    from oracle import soxr_oracle as S

    fp, fs, att = S.hq_spec()
    assert abs(fp - 0.913628) < 1e-6 and fs == 1.0 and abs(att - 126.4326) < 1e-4
    h = S.design_lpf(fp, fs, 2.0, att)
    assert len(h) == 389 and abs(h.sum() - 1.0) < 1e-6 and np.array_equal(h, h[::-1])
    # frequency response of the 2 : 1 filter: flat pass-band to 0.9136 x 11025 Hz, >= 120 dB down from 11025 Hz
    H = np.abs(np.fft.rfft(h, 1 << 16))
    f = np.fft.rfftfreq(1 << 16, 1 / 44100.0)
    assert np.abs(H[f <= fp * 11025] - 1.0).max() <= 2e-6
    assert 20 * np.log10(H[f >= 11025].max()) <= -120.0
    rng = np.random.default_rng(0)
    for sr, n in ((44100, 30001), (48000, 2000), (16000, 1500), (8000, 999), (32000, 1), (11025, 700), (96000, 4000),
                  (176400, 8000), (352800, 16000)):  # 8 : 1 and 16 : 1 (1,541 and 3,077 taps)
        x = rng.uniform(-1, 1, n).astype(np.float32)
        a, b = audio.resample(x, sr), S.resample(x, sr)
        assert a.shape == b.shape == (int(np.ceil(n * 22050 / sr)),), sr
        assert np.abs(a - b).max() <= 1e-6, (sr, np.abs(a - b).max())
    # a 1 kHz sine keeps its amplitude and phase (zero-phase filter, output k at input time k * down / up)
    t = np.arange(44100) / 44100.0
    y = audio.resample(np.sin(2 * np.pi * 1000 * t).astype(np.float32), 44100)
    t2 = np.arange(22050) / 22050.0
    assert np.abs(y[500:-500] - np.sin(2 * np.pi * 1000 * t2)[500:-500]).max() <= 1e-5


@pytest.mark.parametrize("kind,bound", [("uniform", 2e-4), ("normal", 2e-5), ("tones", 2e-3)])
def test_fp32_vs_fp64_noise_floor(weights, kind, bound):
    """SURVEY.md §7 hard part 1: the same graph in fp32 vs fp64 differs by up to ~1e-4 on noise-like
    input and ~1e-3 on tonal input; the parity tolerance in the GPU tests is derived from this."""
    x = make_windows(kind, 2, seed=3)
    a = O.forward(x, weights, np.float32)
    b = O.forward(x, weights, np.float64)
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= bound, (kind, k, np.abs(a[k] - b[k]).max())


def test_all_zero_window_is_finite(weights):
    """divide_no_nan (signal.py:183): a silent window gives finite, constant-ish outputs."""
    r = O.forward(np.zeros((1, O.AUDIO_N_SAMPLES), np.float32), weights, np.float32, intermediates=True)
    for k in ("note", "onset", "contour"):
        assert np.isfinite(r[k]).all()
    assert np.allclose(r["z"], weights["bn_affine"][1])


def test_harmonic_stack_shifts():
    import torch

    z = torch.arange(309, dtype=torch.float64).reshape(1, 1, 309) + 1.0
    s = O.harmonic_stack(z)[0, :, 0, :]
    for c, sh in enumerate(O.HARMONIC_SHIFTS):
        for f in (0, 1, 40, 200, 263):
            expect = f + sh + 1.0 if 0 <= f + sh < 309 else 0.0
            assert s[c, f].item() == expect


def test_c_restatement_agrees_with_torch_oracle(weights):
    """oracle/bp_oracle.c (the CPU baseline bench.py times) is an independent restatement of the same graph:
    it must agree with the torch fp32 oracle to summation-order noise, and be as close to fp64 as it is."""
    import subprocess

    from conftest import make_windows

    subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")], check=True)
    x = np.concatenate([make_windows("uniform", 2, 0), make_windows("normal", 1, 1)])
    r32 = O.forward(x, weights, np.float32)
    r64 = O.forward(x, weights, np.float64)
    rc = O.forward_c(x, 4)
    for k in ("note", "onset", "contour"):
        assert rc[k].shape == r32[k].shape
        assert np.abs(rc[k] - r32[k]).max() <= 5e-5, k
        assert np.abs(rc[k] - r64[k]).max() <= 2 * np.abs(r32[k] - r64[k]).max() + 2e-5, k


def test_extended_cqt_restatement_is_consistent(weights):
    """The 44.1 kHz / 345-bin re-parametrisation (BASELINE.json configs[4]) has no reference
    fixture; it is pinned to the pinned 22.05 kHz restatement instead: its sqrt(lengths) table continues the model's
    (bin b + 36 == bin b), and its bins 0..308 are the 22.05 kHz CQT of its own first pyramid level up to that ratio."""
    import torch

    ext = O.ext_sqrt_len()
    assert ext.shape == (345,) and np.array_equal(ext[36:], weights["cqt_sqrt_len"])
    x = np.random.default_rng(4).uniform(-1, 1, (1, O.EXT_AUDIO_N_SAMPLES)).astype(np.float32)
    r = O.forward(x, weights, np.float64, intermediates=True, ext=True)
    assert r["mag"].shape == (1, 172, 345) and r["contour"].shape == (1, 172, 264) and len(r["levels"]) == 10
    assert r["levels"][1].shape[1] == O.AUDIO_N_SAMPLES
    std = O.cqt(torch.from_numpy(r["levels"][1]), weights, np.float64).numpy()
    ratio = ext[:309].astype(np.float64) / weights["cqt_sqrt_len"].astype(np.float64)
    assert np.abs(r["mag"][:, :, :309] - std * ratio).max() <= 1e-12
    assert r["mag"][:, :, 309:].max() > 0  # the new top octave carries data


def test_soxr_stage_plan_restatement():
    """oracle/soxr_oracle.py::stage_plan restates libsoxr's stage determination (cr.c): the 2 : 1 ratio of the
    reference's golden clip is ONE single-rate stage (what the golden pin rests on); 48 kHz, 16 kHz and 8 kHz are one
    rational poly-phase stage each; 88.2 / 96 kHz put a half-band decimation in front, 32 kHz a 2 x interpolation.  The two
    design rules give the tap counts the restatement documents."""
    from oracle import soxr_oracle as S

    p = S.stage_plan(44100 / 22050)
    assert (p["shr"], p["preL"], p["preM"], p["arbL"], p["single_stage"]) == (0, 1, 2, 1, True)
    for sr, (L, M) in ((48000, (147, 320)), (16000, (441, 320)), (8000, (441, 160))):
        p = S.stage_plan(sr / 22050)
        assert (p["shr"], p["preL"], p["arbL"], int(p["arbM"]), p["rational"], p["single_stage"]) == (0, 1, L, M, True, True), sr
    assert S.stage_plan(88200 / 22050)["shr"] == 1 and S.stage_plan(96000 / 22050)["shr"] == 1
    assert S.stage_plan(32000 / 22050)["preL"] == 2 and not S.stage_plan(32000 / 22050)["single_stage"]
    assert len(S.taps(1, 2)) == 389
    odd, poly = S.taps(147, 320, poly_rule=False), S.taps(147, 320, poly_rule=True)
    assert len(odd) % 2 == 1 and len(odd) % 4 == 1 and (len(poly) + 1) % 147 == 0
    for h in (odd, poly):
        assert abs(h.sum() / 147 - 1.0) < 1e-6 and np.allclose(h, h[::-1])
