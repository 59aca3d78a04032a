"""Streaming sessions on the GPU (bp_stream_*, basic_pitch_amd/streaming.py): the rows a stream emits, concatenated, are bit
for bit the one-shot call's on the concatenated input — for any chunking, through the ingest, for many streams per step
and on the other kinds of handle.  Every test does ordinary work; the argument errors are all rejected before anything
is queued."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_windows

pytestmark = pytest.mark.gpu

HOP, WIN, LEAD = 36164, 43844, 3840
MAPS = ("note", "onset", "contour")
WIDTH = {"note": 88, "onset": 88, "contour": 264}


@pytest.fixture(scope="module")
def nat():
    from basic_pitch_amd import _native

    return _native


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    m = Model(max_windows=8)
    yield m
    m.close()


def chunkings(n_frames, seed):
    """The ways a signal of n_frames is cut into pushes: all at once, 512 frames, exactly hop-sized, seeded random sizes
    in 0 ... 100 000 with zero-length pushes among them."""
    rng = np.random.default_rng(seed)
    rand, left = [], n_frames
    while left > 0:
        k = 0 if rng.random() < 0.15 else int(rng.integers(0, 100_001))
        rand.append(min(k, left))
        left -= rand[-1]
    rand.append(0)
    fixed = lambda k: [min(k, n_frames - a) for a in range(0, n_frames, k)]  # noqa: E731
    return {"one push": [n_frames], "512": fixed(512), "hop": fixed(HOP), "random": rand}


def run_stream(stream, data, sizes, frame_items=1, after_push=None):
    """Push `data` (a flat array, frame_items items per frame) in pieces of `sizes` frames, finish; the concatenated rows."""
    parts, at = [], 0
    for k in sizes:
        parts.append(stream.push(data[at * frame_items : (at + k) * frame_items]))
        at += k
        if after_push:
            after_push(at, stream.rows)
    assert at * frame_items == len(data)
    parts.append(stream.finish())
    return {m: np.concatenate([p[m] for p in parts]) for m in MAPS}


def assert_same(got, ref, what):
    for m in MAPS:
        assert got[m].shape == ref[m].shape, (what, m, got[m].shape, ref[m].shape)
        assert np.array_equal(got[m].view(np.uint32), ref[m].view(np.uint32)), (what, m)


def signal(kind, n, seed):
    if kind == "noise":
        return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)
    pieces = make_windows("tones", n // WIN + 1, seed)
    return np.ascontiguousarray(pieces.reshape(-1)[:n])


# ---- 1. bit-equality, 22.05 kHz mono float -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "tones"])
def test_stream_rows_equal_the_one_shot_track_for_any_chunking(model, nat, kind):
    from basic_pitch_amd import streaming

    for li, n in enumerate([0, 1, 40003, 40004, 40005, HOP * 3, HOP * 3 + 1, HOP * 24 + 12345]):
        x = signal(kind, n, 100 + li)
        ref = model.predict_track(x)
        for name, sizes in chunkings(n, 7 + li).items():
            def rows_are_final(pushed, rows):
                assert rows == streaming.rows_after(pushed), (kind, n, name, pushed, rows)

            with model.open_stream(22050) as s:
                got = run_stream(s, x, sizes, after_push=rows_are_final)
                assert s.rows == streaming.rows_after(n, finished=True) == ref["note"].shape[0]
            assert_same(got, ref, (kind, n, name))


# ---- 2. bit-equality through the ingest ----------------------------------------------------------------------------------
def _ingest_cases(nat):
    from basic_pitch_amd import audio, inference

    raw, tag, bits, channels, sr = audio.wav_raw(os.path.join(GOLDEN, "vocadito_10.wav"))
    fmt = inference._WAV_PCM[(tag, bits)]
    dtype = {nat.BP_PCM_S16: np.int16, nat.BP_PCM_F32: np.float32, nat.BP_PCM_S32: np.int32, nat.BP_PCM_U8: np.uint8,
             nat.BP_PCM_S24: np.uint8, nat.BP_PCM_F64: np.float64}[fmt]
    items = channels * (3 if fmt == nat.BP_PCM_S24 else 1)
    clip = np.frombuffer(raw, dtype=np.uint8).view(dtype)
    assert sr == 44100
    rng = np.random.default_rng(31)
    return [
        ("golden clip", clip, fmt, channels, sr, items),
        ("s16 stereo 48000", rng.integers(-32768, 32768, 2 * 300_017).astype(np.int16), nat.BP_PCM_S16, 2, 48000, 2),
        ("s16 stereo 16000", rng.integers(-32768, 32768, 2 * 120_011).astype(np.int16), nat.BP_PCM_S16, 2, 16000, 2),
        ("f64 mono 96000", rng.uniform(-1, 1, 500_009), nat.BP_PCM_F64, 1, 96000, 1),
    ]


def test_stream_rows_equal_the_one_shot_pcm_call_through_the_ingest(model, nat):
    """Downmix and resampling at absolute output indices from the input history + the chunk.  (Rates whose filter the
    one-shot call evaluates in the kernel — more than 2^22 taps — are not streamed: bp_stream_open refuses them.)"""
    for what, data, fmt, channels, sr, items in _ingest_cases(nat):
        n = len(data) // items
        ref = model.predict_pcm_raw(data, fmt, n, channels, sr)
        for name, sizes in chunkings(n, 5).items():
            with model.open_stream(sr, channels, fmt) as s:
                got = run_stream(s, data, sizes, frame_items=items)
            assert_same(got, ref, (what, name))
        if what == "golden clip":  # the reference's own known answer for this clip, at its tolerance
            g = np.load(os.path.join(GOLDEN, "vocadito_10_model_output.npz"))
            for m in MAPS:
                assert ref[m].shape == g[m].shape
                assert np.abs(got[m] - g[m]).max() <= 1e-4, m


def test_open_refuses_a_rate_whose_filter_is_not_tabulated(model):
    with pytest.raises(ValueError, match="44101"):
        model.open_stream(44101)


# ---- 3. notes --------------------------------------------------------------------------------------------------------------
def test_streaming_transcriber_reproduces_the_golden_note_events(nat):
    from basic_pitch_amd import audio, inference
    from basic_pitch_amd.streaming import StreamingTranscriber

    wav = os.path.join(GOLDEN, "vocadito_10.wav")
    raw, tag, bits, channels, sr = audio.wav_raw(wav)
    fmt = inference._WAV_PCM[(tag, bits)]
    frame = channels * bits // 8
    raw = bytes(raw)
    with StreamingTranscriber(inference.ICASSP_2022_MODEL_PATH, sr, channels, fmt) as t:
        for a in range(0, len(raw), 4096 * frame):
            t.push(raw[a : a + 4096 * frame])
        model_output, midi, events = t.finish()
    g = np.load(os.path.join(GOLDEN, "vocadito_10_note_events.npz"))
    assert len(events) == len(g["pitch"]) == 28
    for i, e in enumerate(events):
        assert e[0] == g["start_s"][i] and e[1] == g["end_s"][i] and e[2] == g["pitch"][i], i
        assert abs(float(e[3]) - float(g["amplitude"][i])) <= 1e-4, i
        assert list(e[4]) == list(g["bend_values"][g["bend_offsets"][i] : g["bend_offsets"][i + 1]]), i
    assert len(midi.instruments) == 1 and len(midi.instruments[0].notes) == 28
    assert_same(model_output, inference.run_inference(wav), "run_inference")


# ---- 4. many streams per step ----------------------------------------------------------------------------------------------
def _random_pcm(rng, nat, fmt, n_items):
    if fmt == nat.BP_PCM_F32:
        return rng.uniform(-1, 1, n_items).astype(np.float32)
    if fmt == nat.BP_PCM_F64:
        return rng.uniform(-1, 1, n_items)
    if fmt == nat.BP_PCM_S16:
        return rng.integers(-32768, 32768, n_items).astype(np.int16)
    if fmt == nat.BP_PCM_S32:
        return rng.integers(-2**31, 2**31, n_items).astype(np.int32)
    return rng.integers(0, 256, n_items).astype(np.uint8)  # BP_PCM_U8, BP_PCM_S24 (3 items per sample)


def test_many_streams_in_lock_step_get_the_rows_they_get_alone(model, nat):
    """40 streams of seeded lengths, formats and rates advance through bp_streams_push with unequal chunks, empty entries
    among them; streams that run out are finished and leave.  The handle holds 8 windows and a step completes more, so the
    batches of a step are several.  A one-shot call on the same handle in the middle changes nothing on either side."""
    rng = np.random.default_rng(44)
    kinds = [(nat.BP_PCM_F32, 1, 22050), (nat.BP_PCM_S16, 2, 44100), (nat.BP_PCM_S16, 2, 48000), (nat.BP_PCM_F64, 1, 96000),
             (nat.BP_PCM_S16, 1, 16000), (nat.BP_PCM_U8, 1, 22050), (nat.BP_PCM_S32, 2, 44100), (nat.BP_PCM_S24, 1, 22050),
             (nat.BP_PCM_F32, 3, 44100)]
    streams = []
    for i in range(40):
        fmt, ch, sr = kinds[i % len(kinds)] if i < 2 * len(kinds) else kinds[int(rng.integers(0, len(kinds)))]
        n = int(rng.uniform(0.5, 7.0) * sr)
        items = ch * (3 if fmt == nat.BP_PCM_S24 else 1)
        data = _random_pcm(rng, nat, fmt, n * items)
        sizes, left = [], n
        while left > 0:
            k = 0 if rng.random() < 0.2 else int(rng.uniform(0.2, 2.2) * sr)
            sizes.append(min(k, left))
            left -= sizes[-1]
        streams.append({"fmt": fmt, "ch": ch, "sr": sr, "n": n, "items": items, "data": data, "sizes": sizes})
    # each stream alone, the same chunks
    for st in streams:
        per_push = []
        with model.open_stream(st["sr"], st["ch"], st["fmt"]) as s:
            st["alone"] = run_stream(s, st["data"], st["sizes"], st["items"], after_push=lambda at, rows: per_push.append(rows))
        st["alone_rows"] = per_push
        assert_same(st["alone"], model.predict_pcm_raw(st["data"], st["fmt"], st["n"], st["ch"], st["sr"]), "alone")
    probe = signal("noise", 3 * HOP + 77, 5)
    probe_ref = model.predict_track(probe)
    # in lock-step
    for st in streams:
        st["s"] = model.open_stream(st["sr"], st["ch"], st["fmt"])
        st["at"], st["step"], st["parts"] = 0, 0, []
    live, step, most_windows = list(streams), 0, 0
    while live:
        chunks = []
        for st in live:
            k = st["sizes"][st["step"]]
            chunks.append(st["data"][st["at"] * st["items"] : (st["at"] + k) * st["items"]])
            st["at"] += k
        outs = model.push_streams([st["s"] for st in live], chunks)
        most_windows = max(most_windows, sum(o["note"].shape[0] for o in outs) // 142)
        for st, o in zip(live, outs):
            st["parts"].append(o)
            assert st["s"].rows == st["alone_rows"][st["step"]]
            st["step"] += 1
        for st in [st for st in live if st["step"] == len(st["sizes"])]:
            st["parts"].append(st["s"].finish())
            st["s"].close()
            live.remove(st)
        step += 1
        if step == 2:
            assert_same(model.predict_track(probe), probe_ref, "one-shot call between the steps")
    assert most_windows > model.max_windows, most_windows  # a step ran more than one batch
    for i, st in enumerate(streams):
        assert_same({m: np.concatenate([p[m] for p in st["parts"]]) for m in MAPS}, st["alone"], i)
    assert_same(model.predict_track(probe), probe_ref, "one-shot call afterwards")


# ---- 5. the other handles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["bf16_weights", "ext_cqt_44k"])
def test_streams_of_the_other_handles_equal_their_own_one_shot_calls(nat, flag):
    from basic_pitch_amd.inference import Model

    rng = np.random.default_rng(9)
    with Model(max_windows=8, **{flag: True}) as m:
        rate = m.sample_rate  # 22050, or 44100 for the extended range
        x = signal("tones", 5 * HOP + 999, 3) if flag == "bf16_weights" else rng.uniform(-1, 1, 4 * 2 * HOP + 999).astype(np.float32)
        ref = m.predict_track(x)
        for name, sizes in chunkings(len(x), 2).items():
            if name == "512":
                continue
            with m.open_stream(rate) as s:
                assert_same(run_stream(s, x, sizes), ref, (flag, name))
        pcm = rng.integers(-32768, 32768, 2 * 400_001).astype(np.int16)
        ref = m.predict_pcm_raw(pcm, nat.BP_PCM_S16, 400_001, 2, 48000)
        with m.open_stream(48000, 2, nat.BP_PCM_S16) as s:
            assert_same(run_stream(s, pcm, chunkings(400_001, 3)["random"], 2), ref, (flag, "48000"))


# ---- 6. the state bound ------------------------------------------------------------------------------------------------------
def test_stream_state_is_bounded_and_independent_of_the_audio_that_has_passed(model, nat):
    """DESIGN.md "Streaming sessions": a stream holds a ring of window + 4 hops samples of the model-rate signal and two
    copies of the resampler's input history of ceil(n_taps / up) frames (2 : 1: 389 taps, up = 1), 4 bytes each — and
    nothing that grows.  The bound is that sum; the figure must be the same after 3 and after 300 windows."""
    bound = 4 * (WIN + 4 * HOP) + 2 * 4 * 389
    block = np.random.default_rng(1).integers(-3000, 3000, 2 * 8 * HOP).astype(np.int16)  # 8 windows of 44.1 kHz mono
    with model.open_stream(44100, 1, nat.BP_PCM_S16) as s:
        at_open = s.state_bytes()
        s.push(block[: 2 * 3 * HOP + 2 * WIN])
        assert s.rows >= 3 * 142
        after_3 = s.state_bytes()
        while s.rows < 300 * 142:
            s.push(block)
        after_300 = s.state_bytes()
        s.finish()
    assert at_open == after_3 == after_300, (at_open, after_3, after_300)
    assert 0 < after_300 <= bound, (after_300, bound)
    with model.open_stream(22050) as s:  # no resampler, no history
        assert 0 < s.state_bytes() <= 4 * (WIN + 4 * HOP)


# ---- 7. errors, all without queued work ----------------------------------------------------------------------------------
def _raw_push(s, data, n, out, capacity):
    rows = C.c_int64(-1)
    rc = s._lib.bp_stream_push(s._s, data.ctypes.data, n, 0, out["note"].ctypes.data, out["onset"].ctypes.data,
                               out["contour"].ctypes.data, capacity, 0, C.byref(rows))
    return rc, int(rows.value)


def test_a_buffer_that_is_too_small_is_refused_and_the_push_can_be_repeated(model, nat):
    x = signal("noise", 4 * HOP + 5000, 12)
    ref = model.predict_track(x)
    out = {m: np.full((4 * 142, WIDTH[m]), np.nan, np.float32) for m in MAPS}
    with model.open_stream(22050) as s:
        first = s.push(x[:1000])
        assert first["note"].shape == (0, 88) and first["contour"].shape == (0, 264)
        body = x[1000 : 3 * HOP + 1000]
        need = s.rows_bound(len(body))
        assert need == 2 * 142
        for capacity in (0, need - 1):
            rc, _ = _raw_push(s, body, len(body), out, capacity)
            assert rc == nat.BP_ERR_INVALID_ARG
            assert b"capacity_rows" in s._lib.bp_last_error(model._handle)
        assert np.isnan(out["note"]).all() and s.rows_bound(len(body)) == need  # nothing written, nothing taken
        rc, rows = _raw_push(s, body, len(body), out, need)
        assert rc == nat.BP_OK and rows == need
        s.rows += rows
        rest = s.push(x[3 * HOP + 1000 :])
        tail = s.finish()
    got = {m: np.concatenate([out[m][:need], rest[m], tail[m]]) for m in MAPS}
    assert_same(got, ref, "after the refused pushes")


def test_argument_errors(model, nat):
    from basic_pitch_amd.inference import Model
    from basic_pitch_amd import streaming

    for bad in ((22050, 1, 99), (22050, 0, nat.BP_PCM_F32), (22050, 65, nat.BP_PCM_F32), (10, 1, nat.BP_PCM_F32),
                (10**6, 1, nat.BP_PCM_F32)):
        with pytest.raises(ValueError):
            model.open_stream(*bad)
    x = signal("noise", HOP, 1)
    with model.open_stream(22050) as s:
        s.push(x)
        s.finish()
        with pytest.raises(ValueError, match="finished"):
            s.push(x[:10])
        with pytest.raises(ValueError, match="finished"):
            s.finish()
    with Model(max_windows=2) as other, other.open_stream(22050) as foreign, model.open_stream(22050) as mine:
        with pytest.raises(ValueError, match="another handle"):
            streaming.push_streams(model, [mine, foreign], [x[:100], x[:100]])
        with pytest.raises(ValueError, match="twice"):
            streaming.push_streams(model, [mine, mine], [x[:100], x[:100]])
        assert mine.push(x)["note"].shape == (0, 88)  # the refused steps took nothing: 36164 samples complete no window
        assert mine.push(x[: WIN - LEAD - HOP])["note"].shape == (142, 88)
