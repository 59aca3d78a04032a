"""FLAC decoded ON THE DEVICE (csrc/flac_device.hip) against the host decoder (csrc/flac_decode.cpp,
itself pinned to RFC 9639's worked example and to WAV <-> FLAC pairs in tests/test_audio_decode.py): the same integers,
sample for sample, on the RFC's example file, on streams from the test-side encoder that exercise every subframe type /
stereo mode / residual coding / sample size, and on the reference's second recording; the MD5 of STREAMINFO is checked
here on the device's output; corrupt and truncated streams are errors; `predict()` on a .flac file goes through it.  The
streams of tests/flac_streams.py take it off the encoder's usual operating point: LPC precision and shift, variable block
sizes, long sample numbers, sample-rate codes 12 / 14, forced Rice parameters, escapes of 0 bits — all decoded, none refused
— and frame headers planted in the payload, which the scan -> chain design either sees through or hands to the host."""
import hashlib
import os

import numpy as np
import pytest

import flac_streams as FS
import flac_writer as FW
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import Model

    m = Model(max_windows=32)
    yield m
    m.close()


def _host_ints(data, bits):
    """the host decoder's floats back as the integers they were made of"""
    from basic_pitch_amd import _native

    import ctypes as C

    lib = _native.load_library()
    ch, sr, b, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    assert lib.bp_flac_info(data, len(data), C.byref(ch), C.byref(sr), C.byref(b), C.byref(n)) == 0
    pcm = np.empty((n.value, ch.value), np.float32)
    got = C.c_int64()
    rc = lib.bp_flac_decode(data, len(data), pcm.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(got))
    assert rc == 0 and got.value == n.value
    return np.round(pcm.astype(np.float64) * (1 << (bits - 1))).astype(np.int64), sr.value


def _md5_of(pcm, bits):
    bps = (bits + 7) // 8
    raw = b"".join(int(v).to_bytes(bps, "little", signed=True) for v in pcm.reshape(-1))
    return hashlib.md5(raw).digest()


def test_rfc9639_example_on_the_device(model):
    data = bytes.fromhex(
        "664c6143" "80000022" "10001000" "00000f00000f" "0ac442f000000001" "3e84b41807dc690307586a3dad1a2e0f"
        "fff869180000bf" "0358fd03128b" "aa9a"
    )
    pcm, sr = model.flac_decode_device(data)
    assert sr == 44100 and pcm.tolist() == [[25588, 10416]]
    assert _md5_of(pcm, 16) == data[26:42]
    for pos in (0x2C, 0x30, 0x33, 0x38):  # a flipped bit in the frame: CRC-8 / CRC-16 / chain
        bad = bytearray(data)
        bad[pos] ^= 0x04
        with pytest.raises(ValueError):
            model.flac_decode_device(bytes(bad))


@pytest.mark.parametrize(
    "bits,ch,sr,n,bs",
    [(16, 1, 44100, 5000, 1152), (16, 2, 44100, 9000, 1152), (24, 2, 48000, 4000, 576), (8, 1, 8000, 3000, 192),
     (16, 3, 22050, 2500, 1000), (16, 2, 12345, 700, 300), (20, 2, 96000, 2000, 4096), (12, 1, 16000, 1200, 256)],
)
def test_device_decoder_equals_host_decoder_on_the_round_trip_matrix(model, bits, ch, sr, n, bs):
    """tests/test_audio_decode.py::test_flac_round_trip's streams (the test-side encoder cycles through constant / verbatim /
    fixed 0..4 / LPC subframes, Rice and Rice2 with several partition orders, escaped partitions, all four stereo modes,
    wasted bits, an ID3 tag in front): device == source PCM == host decoder, and the MD5 of STREAMINFO holds."""
    rng = np.random.default_rng(bits * 100 + ch)
    t = np.arange(n) / sr
    x = np.stack([0.4 * np.sin(2 * np.pi * 220 * (c + 1) * t) + 0.05 * rng.standard_normal(n) for c in range(ch)], 1)
    full = 1 << (bits - 1)
    pcm = np.clip(np.round(x * full), -full, full - 1).astype(np.int64)
    pcm[100:400] = 0
    pcm[1200:1500] = (pcm[1200:1500] >> 3) << 3
    pcm[50] = -full
    data = FW.encode(pcm, sr, bits, blocksize=bs, id3=(ch == 3))
    got, sr2 = model.flac_decode_device(data)
    assert sr2 == sr and got.shape == (n, ch)
    assert np.array_equal(got, pcm)
    host, _ = _host_ints(data, bits)
    assert np.array_equal(got, host)
    lay = model.flac_layout(data)
    md5_at = data.index(b"fLaC") + 8 + 18
    assert _md5_of(got, bits) == data[md5_at : md5_at + 16] and lay["n_frames"] == n
    # truncation and corruption are errors, not silence
    with pytest.raises(ValueError):
        model.flac_decode_device(data[: len(data) - 7])
    bad = bytearray(data)
    bad[len(data) // 2] ^= 0x10
    with pytest.raises(ValueError):
        model.flac_decode_device(bytes(bad))


def test_second_recording_and_whole_path(model, tmp_path):
    """tests/golden/vocadito_14.flac (537,924 frames, 132 frames of 4096): device == host decoder on every sample, MD5 of
    STREAMINFO on the device's output; its posteriorgrams through bp_infer_flac equal those of the host-decoded samples
    through bp_infer_pcm bit for bit (the same ingest kernels run on the same integers); `predict()` takes the device path
    for a .flac file and returns the same events as for the host-decoded samples."""
    from basic_pitch_amd import audio, inference as inf

    path = os.path.join(GOLDEN, "vocadito_14.flac")
    data = open(path, "rb").read()
    got, sr = model.flac_decode_device(data)
    host, sr2 = _host_ints(data, 16)
    assert sr == sr2 == 44100 and got.shape == host.shape == (537924, 1) and np.array_equal(got, host)
    md5_at = data.index(b"fLaC") + 8 + 18
    assert _md5_of(got, 16) == data[md5_at : md5_at + 16]
    a = model.predict_flac(data)
    pcm, _ = audio.read_audio(path)
    b = model.predict_pcm(pcm, sr)
    for k in ("note", "onset", "contour"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    calls = []
    orig = model.predict_flac
    model.predict_flac = lambda blob: (calls.append(len(blob)), orig(blob))[1]
    try:
        mo, _, ev = inf.predict(path, model)
    finally:
        del model.predict_flac
    assert calls == [len(data)] and all(np.array_equal(mo[k], a[k]) for k in a) and len(ev) > 20
    # a stream without a sample count in STREAMINFO is left to the host decoder — predict() still works
    rng = np.random.default_rng(5)
    pcm16 = (3000 * np.sin(np.arange(30000) * 0.05) + rng.integers(-200, 200, 30000)).astype(np.int64)[:, None]
    nohdr = FW.encode(pcm16, 22050, 16, blocksize=1024, total_in_header=False)
    p = tmp_path / "nototal.flac"
    p.write_bytes(nohdr)
    from basic_pitch_amd._native import NativeLibraryError

    with pytest.raises((ValueError, NativeLibraryError)):
        model.flac_decode_device(nohdr)
    mo2 = inf.run_inference(str(p), model)
    assert mo2["note"].shape[0] == int(30000 / 36164 * 142)


def test_long_random_streams_with_every_coding_choice(model):
    """Fuzz: noise-like and tonal 16-bit stereo material, 20 frames each, block sizes 192..4608, the encoder's coding
    choices cycling per frame — device == host on every sample."""
    for seed, bs in ((1, 192), (2, 1024), (3, 4608), (4, 2304)):
        rng = np.random.default_rng(seed)
        n = bs * 20 + 77
        t = np.arange(n)
        x = np.stack([6000 * np.sin(t * 0.01 * (seed + 1)) + rng.integers(-3000, 3000, n),
                      5000 * np.sin(t * 0.013) + rng.integers(-30, 30, n)], 1).astype(np.int64)
        data = FW.encode(x, 44100, 16, blocksize=bs)
        got, _ = model.flac_decode_device(data)
        assert np.array_equal(got, x), (seed, bs)


def test_bench_corpus_encoder(model, tmp_path):
    """tools/flac_synth.c (the encoder `bench.py --workload files --native --flac` makes its corpus with: LPC order 8, Rice
    partitions, block size 4096, a short last block) writes streams both decoders accept: host (every CRC checked) == device
    == the WAV it was given; and the native pipeline transcribes the .flac through the device decoder to the bytes it
    writes for the .wav."""
    import subprocess
    import wave

    from basic_pitch_amd import audio, transcribe_files

    exe = str(tmp_path / "flac_synth")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-O2", "-o", exe, os.path.join(root, "tools", "flac_synth.c"), "-lm"], check=True)
    rng = np.random.default_rng(9)
    n = 44100 * 12 + 333
    t = np.arange(n) / 44100.0
    x = 0.3 * np.sin(2 * np.pi * 330.0 * t) * (np.sin(2 * np.pi * 1.1 * t) > 0) + 0.01 * rng.standard_normal(n)
    pcm = (np.clip(np.stack([x, x[::-1]], 1), -1, 1) * 32767).astype("<i2")
    wav, flac = tmp_path / "tone.wav", tmp_path / "tone.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm.tobytes())
    subprocess.run([exe, str(wav), str(flac)], check=True, stderr=subprocess.DEVNULL)
    data = flac.read_bytes()
    assert len(data) < 0.9 * pcm.nbytes
    y, sr = audio.read_audio(flac)
    assert sr == 44100 and np.array_equal(np.round(y * 32768).astype(np.int64), pcm.astype(np.int64))
    got, _ = model.flac_decode_device(data)
    assert np.array_equal(got, pcm.astype(np.int32))
    outs = {}
    before = model._lib.bp_files_direct_reads()
    for name, src, kw in (("wav", wav, {}), ("flac_dev", flac, {}), ("flac_host", flac, {"host_flac": True})):
        o = tmp_path / name
        o.mkdir()
        (rep,) = transcribe_files([str(src)], o, models=[model], threads=1, **kw)
        assert rep["status"] == 0 and rep["n_note_events"] > 5, rep
        outs[name] = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o))}
    assert model._lib.bp_files_direct_reads() == before
    names = [sorted(v) for v in outs.values()]
    assert names[0] == names[1] == names[2] == ["tone_basic_pitch.csv", "tone_basic_pitch.mid"]
    for f in names[0]:
        assert outs["wav"][f] == outs["flac_dev"][f] == outs["flac_host"][f], f


def test_every_lpc_order_with_the_classes_mixed_in_one_wave(model):
    """LPC orders 1..32 cycling from frame to frame (the lanes of one wave are frames): the register predictors of 4 / 8 / 12
    products — the widest class present in the wave serves all its lanes —, the generic path of the orders above 12, partition
    orders 0..2, Rice and Rice2, escaped partitions; 16- and 24-bit.  device == source == host decoder."""
    orders = [1, 2, 4, 5, 8, 9, 12, 13, 20, 32, 3, 11, 7, 16, 6, 10]
    for bits, bs, seed in ((16, 256, 11), (24, 192, 12), (16, 1000, 13)):
        rng = np.random.default_rng(seed)
        n = bs * 70 + 31
        t = np.arange(n)
        full = 1 << (bits - 1)
        x = np.stack([0.3 * full * np.sin(t * 0.021) + rng.integers(-full // 64, full // 64, n),
                      0.2 * full * np.sin(t * 0.0057) + rng.integers(-full // 4096 - 2, full // 4096 + 2, n)], 1).astype(np.int64)
        plan = lambda fi: dict(kind="lpc", lpc_order=orders[fi % len(orders)], porder=fi % 3, rice2=bool(fi % 2),
                               escape=(fi % 7 == 6), stereo=("indep", "ms", "ls", "sr")[fi % 4])
        data = FW.encode(x, 48000, bits, blocksize=bs, plan=plan)
        got, _ = model.flac_decode_device(data)
        assert np.array_equal(got, x), (bits, bs)
        host, _ = _host_ints(data, bits)
        assert np.array_equal(got, host), (bits, bs)


def test_blocking_wait_lane_sleeps_while_the_device_decodes():
    """BP_FLAG_BLOCKING_WAIT (the lanes of a file job): the end of a call sleeps between event queries — a blocking-sync event
    wait polls on this runtime, user time == wall time (tools/experiments/host_cpu.py) — so a lane that waits for 20 decodes
    of a 20-second stream costs its core a fraction of the wall time, and decodes the same samples."""
    import ctypes as C
    import resource
    import time

    from basic_pitch_amd import Model

    rng = np.random.default_rng(21)
    n = 20 * 44100
    t = np.arange(n)
    x = np.stack([8000 * np.sin(t * 0.02) + rng.integers(-500, 500, n), 6000 * np.sin(t * 0.013) + rng.integers(-300, 300, n)],
                 1).astype(np.int64)
    data = FW.encode(x, 44100, 16, blocksize=4096, plan=lambda fi: dict(kind="lpc", porder=3, rice2=False,
                                                                                          escape=False, stereo="indep"))
    spin, sleep = Model(max_windows=16), Model(max_windows=16, blocking_wait=True)
    a, _ = spin.flac_decode_device(data)
    b, _ = sleep.flac_decode_device(data)
    assert np.array_equal(a, b) and np.array_equal(a, x)
    nf = C.c_int64()

    def cost(m):
        for _ in range(3):
            m._lib.bp_flac_decode_device(m._handle, data, len(data), None, 0, C.byref(nf))
        r0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
        for _ in range(20):
            assert m._lib.bp_flac_decode_device(m._handle, data, len(data), None, 0, C.byref(nf)) == 0
        r1, t1 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
        return (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime), t1 - t0

    cpu_spin, wall_spin = cost(spin)
    cpu_sleep, wall_sleep = cost(sleep)
    assert cpu_sleep < 0.6 * wall_sleep, (cpu_sleep, wall_sleep)
    assert wall_sleep < 2.0 * wall_spin + 0.01, (wall_sleep, wall_spin)
    spin.close()
    sleep.close()


def test_corrupt_small_files_are_errors_or_the_host_decoders_samples(model):
    """A lane that loses a corrupt stream runs ahead of its frame (long unary runs: kilobytes per burst) — it must stay inside
    the file's buffer (its block loads are clamped to the padding behind the file) and the call must end in an error or, if
    the damage happens to be decodable, in exactly what the host decoder makes of the same bytes.  Small files: the buffer's
    slack behind them is smallest."""
    rng = np.random.default_rng(99)
    n = 700
    x = np.stack([3000 * np.sin(np.arange(n) * 0.05) + rng.integers(-200, 200, n)], 1).astype(np.int64)
    good = FW.encode(x, 16000, 16, blocksize=256, plan=lambda fi: dict(kind="lpc", porder=1, rice2=False, escape=False))
    start = good.index(b"fLaC") + 42
    outcomes = {"error": 0, "decoded": 0}
    for trial in range(150):
        bad = bytearray(good)
        for _ in range(1 + trial % 4):
            pos = int(rng.integers(start, len(bad)))
            bad[pos] = 0 if trial % 3 == 0 else int(rng.integers(0, 256))  # zeros make long unary runs
        if trial % 5 == 0:
            del bad[int(rng.integers(start + 10, len(bad))):]
        try:
            got, _ = model.flac_decode_device(bytes(bad))
        except ValueError:
            outcomes["error"] += 1
            continue
        outcomes["decoded"] += 1
        host, _ = _host_ints(bytes(bad), 16)
        assert np.array_equal(got, host), trial
    assert outcomes["error"] > 100, outcomes


# ---- the streams of tests/flac_streams.py: valid files, every expected value is the PCM the stream was made from ------------
def _device_decodes_to_the_source(model, st):
    """device == source PCM == host decoder, the MD5 of STREAMINFO on the device's output, the sample count; no refusal"""
    got, sr = model.flac_decode_device(st.data)
    assert sr == st.sr and got.shape == st.pcm.shape
    assert np.array_equal(got, st.pcm)
    host, _ = _host_ints(st.data, st.bits)
    assert np.array_equal(got, host)
    md5_at = st.data.index(b"fLaC") + 8 + 18
    assert _md5_of(got, st.bits) == st.data[md5_at : md5_at + 16]
    assert model.flac_layout(st.data)["n_frames"] == len(st.pcm)


@pytest.mark.parametrize("bits", [16, 24])
def test_lpc_precision_and_shift_mixed_in_one_wave(model, bits):
    """70 frames = lanes of two waves, and from lane to lane another precision (1..15 bits), shift (0..15, both ends of the funnel
    shift that cuts the prediction out of the float64 sum) and order (the three register classes and the generic path)."""
    _device_decodes_to_the_source(model, FS.precision_shift_mixed(bits))


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("prec,shift", FS.PREC_SHIFT)
def test_lpc_precision_and_shift(model, prec, shift, bits):
    _device_decodes_to_the_source(model, FS.precision_shift(prec, shift, bits))


@pytest.mark.parametrize("mode", FS.MODES)
def test_full_scale_24_bit_with_saturated_coefficients(model, mode):
    """the largest sums the register predictor's float64 arithmetic meets in a valid stream: twelve 15-bit coefficients pinned
    at -16384 / 16383 against 24- / 25-bit samples at full scale whose signs line up with them — |sum| = 2^40.6 and 2^41.6
    (tests/flac_streams.py full_scale asserts the figure), cut out by the funnel shift at 14"""
    _device_decodes_to_the_source(model, FS.full_scale(mode))


@pytest.mark.parametrize("name,wide", [("mixed", False), ("one", False), ("tiny", False), ("mixed", True)])
def test_variable_block_size(model, name, wide):
    """The variable branch of the header parse, of the chain (a successor's number is its predecessor's plus the predecessor's
    block size) and of the frames' places in the output; "mixed" and "tiny" put frames of 16 / 17 samples — less than one
    burst of residuals — beside frames of 4,096 in one wave."""
    _device_decodes_to_the_source(model, FS.variable(name, wide))


@pytest.mark.parametrize("nbytes", [3, 4])
def test_sample_numbers_of_three_and_four_bytes(model, nbytes):
    """Coded numbers of three bytes, and of four and five in a stream of 2.2 million samples whose first 33 frames are
    constant subframes of 65,535 samples (the largest block size a frame header can state)."""
    _device_decodes_to_the_source(model, FS.long_numbers(nbytes))


@pytest.mark.parametrize("sr,code", [(48000, 12), (8000, 12), (44100, 14), (22050, 14)])
def test_sample_rate_codes_12_and_14(model, sr, code):
    _device_decodes_to_the_source(model, FS.rate_code(sr, code))


@pytest.mark.parametrize("k,rice2", [(0, False), (1, True), (14, False), (30, True)])
def test_rice_parameter_extremes(model, k, rice2):
    """Parameter 0 / 1 on residuals of hundreds: every burst of sixteen codes holds codes beyond the 32-bit window and is
    replayed code by code, each code refuels the lane's ring several times.  14 / 30: codes of 15+ and 31+ bits."""
    _device_decodes_to_the_source(model, FS.rice_forced(k, rice2))


def test_escaped_partitions_of_zero_bits(model):
    _device_decodes_to_the_source(model, FS.escape_zero())


# what flac_decode_device makes of the files with planted headers (test_frame_headers_inside_the_payload): the chain keeps a
# false header that a real frame "continues" or that continues a real frame, and then fails as a whole; the last real frame
# behind a stray header has neither a predecessor it continues nor a successor, is dropped, and the sample count falls short
OUTCOMES = {"stray": "decoded", "stray_late": "refused", "continues": "refused", "pair": "refused", "flood": "refused",
            "variable_stray": "decoded", "variable_continues": "refused", "continues_long": "refused"}


def _planted_outcome(model, st):
    """the contract of a valid file with false sync codes: exactly the source PCM, or a refusal — never other samples"""
    from basic_pitch_amd._native import NativeLibraryError

    try:
        got, sr = model.flac_decode_device(st.data)
    except (ValueError, NativeLibraryError):
        return "refused"
    assert sr == st.sr and np.array_equal(got, st.pcm)
    return "decoded"


def test_frame_headers_inside_the_payload(model, tmp_path):
    """Verbatim samples that spell complete frame headers (tests/flac_streams.py planted(): each checked to sit where it should
    and to pass the sync, reserved-value and CRC-8 rules).  The chain drops a candidate that neither continues its predecessor
    nor is continued by its successor: the stray ones in the middle of a stream must be decoded, fixed and variable block
    size; the others (a false header that carries its predecessor's number + 1, a pair that continue each other, more
    candidates than a chunk's list holds, a stray one in front of the last frame) may be refused, never decoded to other
    samples.  Whatever the device decoder does, `predict()` on the file returns what the host-decoded samples give, and the
    native file job falls back to the host decoder (file_pipeline.cpp Worker::infer, "a FLAC stream the device decoder could not follow")
    and writes the bytes it writes with host_flac=True.

    What happens to each file is recorded in OUTCOMES above (the stray header in the next-to-last frame: refused) and asserted,
    so that a change of behaviour is noticed."""
    from basic_pitch_amd import inference as inf, transcribe_files

    outcomes = {}
    for case in FS.PLANTED:
        st = FS.planted(case)
        FS.check_planted(st, FS.planted_shape(case)[0])
        outcomes[case] = _planted_outcome(model, st)
        path = tmp_path / (case + ".flac")
        path.write_bytes(st.data)
        calls, orig = [], model.predict_flac

        def recorded(blob):
            calls.append("refused")
            maps = orig(blob)
            calls[-1] = "decoded"
            return maps

        model.predict_flac = recorded
        try:
            mo, _, ev = inf.predict(str(path), model)
        finally:
            del model.predict_flac
        assert calls == [outcomes[case]], (case, calls)  # predict() went to the device, and to the host where that refused
        pcm = (st.pcm / 32768.0).astype(np.float32)
        want = model.predict_pcm(pcm, st.sr)
        assert all(np.array_equal(mo[k], want[k]) for k in want), case
        _, ev_host = inf._output_to_notes(want, inf.DEFAULT_ONSET_THRESHOLD, inf.DEFAULT_FRAME_THRESHOLD,
                                          inf.DEFAULT_MINIMUM_NOTE_LENGTH_MS, None, None, False, True, inf.DEFAULT_MINIMUM_MIDI_TEMPO)
        assert ev == ev_host, case
        if case == "continues_long":  # (the other clips are 70 ms, too short for a note: their event lists are empty)
            assert len(ev) > 0
    assert outcomes["stray"] == outcomes["variable_stray"] == "decoded", outcomes
    assert OUTCOMES == outcomes
    # the native job on the second of tone with a "continues" header, which the device decoder refuses (asserted above through
    # flac_decode_device and predict_flac on the same bytes; the job's report does not say which decoder ran): status 0 and
    # the same note events in the same files as with the host decoder asked for
    written = {}
    for name, kw in (("device_first", {}), ("host", {"host_flac": True})):
        o = tmp_path / name
        o.mkdir()
        (rep,) = transcribe_files([str(tmp_path / "continues_long.flac")], o, models=[model], threads=1, **kw)
        assert rep["status"] == 0 and rep["n_note_events"] > 0, rep
        written[name] = {f: open(os.path.join(o, f), "rb").read() for f in sorted(os.listdir(o))}
    assert sorted(written["host"]) == ["continues_long_basic_pitch.csv", "continues_long_basic_pitch.mid"]
    assert written["device_first"] == written["host"]
