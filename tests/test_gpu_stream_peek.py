"""Peek and live transcripts on the GPU (bp_stream_peek / bp_streams_peek / bp_stream_keep / bp_stream_candidates,
basic_pitch_amd/streaming.py): at any moment the rows a stream has emitted followed by the rows of a peek are bit for bit the
one-shot call's on the audio so far, a peek leaves no trace in what the stream returns later, and the live transcript is
`predict()`'s for the audio so far, event for event.  Every test does ordinary work; refusals are argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HOP, WIN, LEAD = 36164, 43844, 3840
MAPS = ("note", "onset", "contour")
WIDTH = {"note": 88, "onset": 88, "contour": 264}
DECODING = (0.5, 0.3, 127.70, None, None, False, True, 120)  # predict()'s defaults, as _output_to_notes takes them


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


@pytest.fixture(scope="module")
def clip(nat):
    """The golden clip as its file stores it: 44.1 kHz int16 mono, about 9 s."""
    from basic_pitch_amd import audio, inference

    raw, tag, bits, channels, sr = audio.wav_raw(os.path.join(GOLDEN, "vocadito_10.wav"))
    assert (sr, channels, inference._WAV_PCM[(tag, bits)]) == (44100, 1, nat.BP_PCM_S16)
    return np.frombuffer(raw, dtype=np.int16).copy()


@pytest.fixture(scope="module")
def mono22k():
    t = np.arange(120_000) / 22050.0
    rng = np.random.default_rng(77)
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 329.63 * t * (1 + 0.01 * t)) + 0.01 * rng.standard_normal(t.size)
    return x.astype(np.float32)


def sizes_for(n, head):
    """Pushes of 1 frame and of 4,099 frames over the whole signal, ONE of 50,000 frames among them, after `head`."""
    sizes, left, i = [], n, 0
    pattern = list(head) + [4099, 1, 4099, 4099, 50_000]
    while left > 0:
        k = pattern[i] if i < len(pattern) else (1 if i % 7 == 0 else 4099)
        sizes.append(min(k, left))
        left -= sizes[-1]
        i += 1
    assert sizes.count(50_000) == 1 and 1 in sizes and 4099 in sizes
    return sizes


def same(got, ref, what):
    for m in MAPS:
        assert got[m].shape == ref[m].shape, (what, m, got[m].shape, ref[m].shape)
        assert np.array_equal(got[m].view(np.uint32), ref[m].view(np.uint32)), (what, m)


def cat(parts):
    return {m: np.concatenate([p[m] for p in parts]) for m in MAPS}


# ---- 1. emitted rows + peeked rows == the one-shot call on the prefix ------------------------------------------------------
@pytest.mark.parametrize("which", ["golden clip 44.1 kHz int16", "float32 mono 22.05 kHz"])
def test_emitted_rows_followed_by_a_peek_are_the_one_shot_call_on_the_prefix(model, nat, clip, mono22k, which):
    """After EVERY push.  The prefixes include one frame, less than the 2 : 1 filter's half-length (389 taps: 194 frames;
    the prefix of 101 frames), less than one window, and lengths on both sides of every window's completion."""
    from basic_pitch_amd import streaming

    if which.startswith("golden"):
        data, fmt, sr, head = clip, nat.BP_PCM_S16, 44100, [1, 100]
    else:
        data, fmt, sr, head = mono22k, nat.BP_PCM_F32, 22050, [1]
    with model.open_stream(sr, 1, fmt) as s:
        assert s.peek()["note"].shape == (0, 88)  # nothing taken yet
        parts, at, short = [], 0, 0
        for k in sizes_for(len(data), head):
            parts.append(s.push(data[at : at + k]))
            at += k
            tail = s.peek()
            ref = model.predict_pcm_raw(data[:at], fmt, at, 1, sr)
            same(cat(parts + [tail]), ref, (which, at))
            n22 = -(-at * 22050 // sr)
            assert tail["note"].shape[0] == streaming.rows_after(n22, True) - streaming.rows_after(n22) <= 2 * 142, at
            short += s.rows == 0
        assert at == len(data) and short >= 3  # prefixes shorter than one window were among them
        parts.append(s.finish())
    same(cat(parts), model.predict_pcm_raw(data, fmt, len(data), 1, sr), (which, "finish"))


# ---- 2. a peek leaves no trace ----------------------------------------------------------------------------------------------
def test_pushes_and_finish_return_the_same_bytes_with_and_without_peeks(model, nat, clip, mono22k):
    for data, fmt, sr in ((clip, nat.BP_PCM_S16, 44100), (mono22k, nat.BP_PCM_F32, 22050)):
        runs = []
        for peeking in (True, False):
            with model.open_stream(sr, 1, fmt) as s:
                parts, at = [], 0
                for k in sizes_for(len(data), [1, 100]):
                    parts.append(s.push(data[at : at + k]))
                    at += k
                    if peeking:
                        s.peek()
                parts.append(s.finish())
            runs.append(parts)
        assert len(runs[0]) == len(runs[1])
        for i, (a, b) in enumerate(zip(*runs)):
            same(a, b, (sr, "push", i))


def test_streams_of_two_rates_through_peek_streams_and_push_streams(model, nat, clip, mono22k):
    """Both streams peeked in one step after every step of pushes: each gets the rows its own peek gives, which with its
    emitted rows are the one-shot call's; and the pushes and finishes return what they return without any peek."""
    chunks_a = [clip[a : a + 30_011] for a in range(0, 240_088, 30_011)]       # 8 chunks at 44.1 kHz
    chunks_b = [mono22k[a : a + 15_000] for a in range(0, 120_000, 15_000)]    # 8 chunks at 22.05 kHz
    kinds = ((44100, nat.BP_PCM_S16), (22050, nat.BP_PCM_F32))
    runs = []
    for peeking in (True, False):
        streams = [model.open_stream(sr, 1, fmt) for sr, fmt in kinds]
        parts = [[], []]
        for i, (ca, cb) in enumerate(zip(chunks_a, chunks_b)):
            for p, o in zip(parts, model.push_streams(streams, [ca, cb])):
                p.append(o)
            if peeking:
                tails = model.peek_streams(streams)
                if i in (1, 4, 7):
                    na, nb = 30_011 * (i + 1), 15_000 * (i + 1)
                    same(cat(parts[0] + [tails[0]]), model.predict_pcm_raw(clip[:na], nat.BP_PCM_S16, na, 1, 44100), ("a", i))
                    same(cat(parts[1] + [tails[1]]), model.predict_pcm_raw(mono22k[:nb], nat.BP_PCM_F32, nb, 1, 22050), ("b", i))
                    same(tails[0], streams[0].peek(), ("a alone", i))
        for p, s in zip(parts, streams):
            p.append(s.finish())
            s.close()
        runs.append(parts)
    for j in range(2):
        for i, (a, b) in enumerate(zip(runs[0][j], runs[1][j])):
            same(a, b, (j, i))


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def _raw_peek(s, out, capacity):
    rows = C.c_int64(-1)
    rc = s._lib.bp_stream_peek(s._s, out["note"].ctypes.data, out["onset"].ctypes.data, out["contour"].ctypes.data, capacity, 0,
                               C.byref(rows))
    return rc, int(rows.value)


def test_a_peek_that_is_refused_changes_nothing(model, nat, mono22k):
    x = mono22k
    out = {m: np.full((2 * 142, WIDTH[m]), np.nan, np.float32) for m in MAPS}
    with model.open_stream(22050) as s:
        rc, rows = _raw_peek(s, out, 0)  # an empty stream: 0 rows into no room at all
        assert (rc, rows) == (nat.BP_OK, 0)
        first = s.push(x[:50_000])
        need = s.rows_bound(0)
        assert first["note"].shape[0] == 142 and need == int(50_000 / HOP * 142) - 142
        rc, _ = _raw_peek(s, out, need - 1)
        assert rc == nat.BP_ERR_INVALID_ARG and b"capacity_rows" in s._lib.bp_last_error(model._handle)
        assert np.isnan(out["note"]).all() and np.isnan(out["contour"]).all()  # nothing written
        rc, rows = _raw_peek(s, out, need)
        assert (rc, rows) == (nat.BP_OK, need)
        ref = model.predict_track(x[:50_000])
        same({m: np.concatenate([first[m], out[m][:need]]) for m in MAPS}, ref, "after the refused peek")
        rest = s.push(x[50_000:])  # the next push is unaffected
        last = s.finish()
        same(cat([first, rest, last]), model.predict_track(x), "the stream after the refused peek")
        rc, _ = _raw_peek(s, out, 2 * 142)
        assert rc == nat.BP_ERR_INVALID_ARG and b"finished" in s._lib.bp_last_error(model._handle)
        with pytest.raises(ValueError, match="finished"):
            s.peek()


# ---- 4. the live transcript ---------------------------------------------------------------------------------------------------
def _same_events(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (what, i)
        assert np.float32(a[3]).tobytes() == np.float32(b[3]).tobytes(), (what, i)
        assert list(a[4]) == list(b[4]), (what, i)


def test_the_live_transcript_is_predicts_answer_for_the_audio_so_far(model, nat, clip):
    """0.25-second chunks of the golden clip.  Checked after 10 and 13 chunks (2.5 s and 3.25 s: both inside window 1, which
    completes at 3.45 s, one window final and the rest tail), after 24 chunks (6 s) and at the end.  The reference's golden maps
    cut at those lengths decode to 8, 11 and 18 events (host decoder, no GPU), so the prefixes are not empty."""
    from basic_pitch_amd import inference as inf
    from basic_pitch_amd.streaming import StreamingTranscriber

    chunk = 11_025
    n_chunks = -(-len(clip) // chunk)
    check_at = {10, 13, 24, n_chunks}
    non_empty_before_the_end = 0
    with StreamingTranscriber(model, 44100, 1, nat.BP_PCM_S16, live=True) as t:
        for i in range(n_chunks):
            t.push(clip[i * chunk : (i + 1) * chunk])
            if i + 1 not in check_at:
                continue
            at = min(len(clip), (i + 1) * chunk)
            midi, events = t.transcript()
            ref_midi, ref = inf._output_to_notes(model.predict_pcm_raw(clip[:at], nat.BP_PCM_S16, at, 1, 44100), *DECODING)
            _same_events(events, ref, at)
            assert [len(x.notes) for x in midi.instruments] == [len(x.notes) for x in ref_midi.instruments]
            assert [len(x.pitch_bends) for x in midi.instruments] == [len(x.pitch_bends) for x in ref_midi.instruments]
            non_empty_before_the_end += at < len(clip) and len(events) > 0
        assert non_empty_before_the_end >= 1
        # the whole clip: the reference's golden events
        g = np.load(os.path.join(GOLDEN, "vocadito_10_note_events.npz"))
        assert len(events) == len(g["pitch"]) == 28
        for i, e in enumerate(events):
            assert e[0] == g["start_s"][i] and e[1] == g["end_s"][i] and e[2] == g["pitch"][i], i
            assert abs(float(e[3]) - float(g["amplitude"][i])) <= 1e-4, i
            assert list(e[4]) == list(g["bend_values"][g["bend_offsets"][i] : g["bend_offsets"][i + 1]]), i
        assert len(midi.instruments) == 1 and len(midi.instruments[0].notes) == 28
        model_output, _, final_events = t.finish()  # unchanged in what it returns
    _same_events(final_events, events, "finish")
    same(model_output, model.predict_pcm_raw(clip, nat.BP_PCM_S16, len(clip), 1, 44100), "finish")


# ---- 5. an update sends only what is new ------------------------------------------------------------------------------------
def test_an_update_does_not_rewrite_the_final_rows_the_caller_holds(model, nat, clip):
    from basic_pitch_amd import note_creation as nc

    prm = nc._note_params(0.5, 0.3, 11, True, None, None, True, 11, True)
    cap = 1024
    note, bend, bits = np.zeros((cap, 88), np.float32), np.zeros((cap, 88), np.int8), np.zeros((cap, 12), np.uint8)
    with model.open_stream(44100, 1, nat.BP_PCM_S16) as s:
        before = s.state_bytes()
        s.keep(prm, 900)
        assert s.state_bytes() - before == (900 + 2 * 142) * 1760 + 32  # the kept maps are counted
        s.push(clip[:200_000])
        held = s.rows
        assert held == 2 * 142
        T1, status = s.candidates(note, bits, bend, 0)
        assert status == 0 and T1 == int(100_000 / HOP * 142)
        final_note, final_bend = note[:held].copy(), bend[:held].copy()
        s.push(clip[200_000:300_000])
        assert s.rows == 4 * 142
        note[:held], bend[:held] = -7.0, 99  # the sentinel over the rows the caller already holds
        T2, status = s.candidates(note, bits, bend, held)
        assert status == 0 and T2 == int(150_000 / HOP * 142)
        assert (note[:held] == -7.0).all() and (bend[:held] == 99).all()
        # everything else is what an update from row 0 gives, and the final rows are the ones held from the first update
        note0, bend0, bits0 = np.zeros_like(note), np.zeros_like(bend), np.zeros_like(bits)
        assert s.candidates(note0, bits0, bend0, 0) == (T2, 0)
        assert np.array_equal(note[held:T2].view(np.uint32), note0[held:T2].view(np.uint32))
        assert np.array_equal(bend[held:T2], bend0[held:T2]) and np.array_equal(bits[:T2], bits0[:T2])
        assert np.array_equal(final_note.view(np.uint32), note0[:held].view(np.uint32)) and np.array_equal(final_bend, bend0[:held])
        # ... and decode to the events of the one-shot call on the audio so far
        from basic_pitch_amd import inference as inf

        ref = inf._output_to_notes(model.predict_pcm_raw(clip[:300_000], nat.BP_PCM_S16, 300_000, 1, 44100), *DECODING)[1]
        _same_events(nc.decode_candidates(note0[:T2], bits0[:T2], bend0[:T2], prm), ref, "update")
        with pytest.raises(ValueError, match="first_row"):
            s.candidates(note, bits, bend, s.rows + 1)
        with pytest.raises(ValueError, match="capacity_rows"):
            s.candidates(note[: T2 - 1], bits, bend, 0)


# ---- 6. the fallback and the cap -------------------------------------------------------------------------------------------
def test_status_1_falls_back_to_the_maps_themselves(model, nat, clip):
    """An onset threshold of 0 (every cell that is not a peak qualifies) reports status 1; transcript() is then the host
    decode of the maps themselves (emitted rows + a peek), which is what the one-shot path returns for them.  The other
    cause of status 1, a NaN in the kept maps: test_a_nan_in_the_kept_maps_reports_status_1_in_the_tail_and_once_carried."""
    from basic_pitch_amd import inference as inf
    from basic_pitch_amd.streaming import StreamingTranscriber

    decoding = (0.0,) + DECODING[1:]
    with StreamingTranscriber(model, 44100, 1, nat.BP_PCM_S16, onset_threshold=0.0, live=True) as t:
        t.push(clip[:150_000])
        n, bits, bend = np.zeros((400, 88), np.float32), np.zeros((400, 12), np.uint8), np.zeros((400, 88), np.int8)
        assert t.stream.candidates(n, bits, bend, 0)[1] == 1
        _, events = t.transcript()
        ref = inf._output_to_notes(model.predict_pcm_raw(clip[:150_000], nat.BP_PCM_S16, 150_000, 1, 44100), *decoding)[1]
        _same_events(events, ref, "onset_threshold = 0")
        assert len(events) > 0


def test_a_nan_in_the_kept_maps_reports_status_1_in_the_tail_and_once_carried(tmp_path):
    """The A/B library's hook bp_ab_stream_poison makes onset cell (row 200, bin 40) of the KEPT copy a NaN whenever that row
    is written there (tools/experiments/stream_nan_ab.py, one process with that library; nothing faults: a NaN is a value).
    Updates of the golden clip: before the hook is set (status 0); with row 200 in the tail (1 final window: the NaN joins
    the update's copy of the record); and twice with row 200 among the final rows (the flag entered the carried record at
    the step that emitted the row and survives the folds after it).  Every transcript() — the three that fall back among
    them — is the host decode of the one-shot maps of the prefix, which is what push + peek hand out."""
    import json
    import subprocess
    import sys

    from basic_pitch_amd import build

    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "stream_nan_ab.py")
    out = str(tmp_path / "nan.json")
    env = dict(os.environ, BASIC_PITCH_AMD_LIB=build.build_library(ab=True))
    subprocess.run([sys.executable, tool, out], check=True, timeout=300, env=env)
    got = json.load(open(out))
    ups = got["updates"]
    assert [u["status"] for u in ups] == [0, 1, 1, 1]
    assert ups[0]["final_rows"] == 0 and ups[1]["final_rows"] == 142 <= got["row"] < ups[1]["rows"]  # in the tail
    assert got["row"] < ups[2]["final_rows"] < ups[3]["final_rows"]                                  # carried
    for u in ups:
        assert len(u["transcript"]) > 0 and u["transcript"] == u["host_decode"], u["frames"]


def test_a_frequency_band_is_applied_to_the_kept_copy_and_to_nothing_else(model, nat, clip):
    """minimum / maximum frequency: constrain_frequency runs on the kept copy (final rows as they are emitted, tail rows
    at every update), the transcript is predict()'s for the prefix with the same band, the note rows an update sends are
    zero outside the band — and the rows push and peek hand out stay the unconstrained one-shot rows."""
    from basic_pitch_amd import inference as inf
    from basic_pitch_amd import note_creation as nc
    from basic_pitch_amd.streaming import StreamingTranscriber

    decoding = DECODING[:3] + (180.0, 500.0) + DECODING[5:]
    with StreamingTranscriber(model, 44100, 1, nat.BP_PCM_S16, minimum_frequency=180.0, maximum_frequency=500.0, live=True) as t:
        parts, at, seen = [], 0, 0
        for n in (110_250, 143_325, 264_600):
            parts.append(t.push(clip[at:n]))
            at = n
            _, events = t.transcript()
            ref_maps = model.predict_pcm_raw(clip[:n], nat.BP_PCM_S16, n, 1, 44100)
            same(cat(parts + [t.stream.peek()]), ref_maps, ("unconstrained rows", n))
            constrained = {m: ref_maps[m].copy() for m in MAPS}
            ref = inf._output_to_notes(constrained, *decoding)[1]  # zeroes the bins outside the band in place
            _same_events(events, ref, n)
            T = ref_maps["note"].shape[0]
            assert np.array_equal(t._note[:T].view(np.uint32), constrained["note"].view(np.uint32)), n
            outside = ~constrained["note"].any(axis=0)
            assert 0 < outside.sum() < 88 and ref_maps["note"][:, outside].any()  # the band really cut something
            seen += len(events)
        assert seen > 0


def test_a_step_past_max_rows_is_refused_and_the_stream_stays_valid(model, nat, mono22k):
    from basic_pitch_amd import note_creation as nc

    prm = nc._note_params(0.5, 0.3, 11, True, None, None, True, 11, True)
    x = mono22k
    with model.open_stream(22050) as s:
        s.keep(prm, 142)
        first = s.push(x[:50_000])  # window 0: the 142 rows that fit
        assert first["note"].shape[0] == 142
        out = {m: np.empty((2 * 142, WIDTH[m]), np.float32) for m in MAPS}
        rows = C.c_int64(-1)
        body = x[50_000:100_000]  # completes window 1
        rc = s._lib.bp_stream_push(s._s, body.ctypes.data, len(body), 0, out["note"].ctypes.data, out["onset"].ctypes.data,
                                   out["contour"].ctypes.data, 2 * 142, 0, C.byref(rows))
        assert rc == nat.BP_ERR_OUT_OF_MEMORY and b"bp_stream_keep" in s._lib.bp_last_error(model._handle)
        # nothing was taken: the stream still peeks (the tail of the first 50,000 samples), updates, and closes
        same(cat([first, s.peek()]), model.predict_track(x[:50_000]), "peek after the refused step")
        note, bits, bend = np.zeros((512, 88), np.float32), np.zeros((512, 12), np.uint8), np.zeros((512, 88), np.int8)
        assert s.candidates(note, bits, bend, 0) == (int(50_000 / HOP * 142), 0)
        with pytest.raises(nat.NativeLibraryError, match="BP_ERR_OUT_OF_MEMORY.*bp_stream_keep"):
            s.finish()  # 196 rows in all: past the cap as well
    # closed by the context manager
