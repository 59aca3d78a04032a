"""Every entry point on the handles that are not the default one: `ext_cqt_44k` (44.1 kHz windows of 87,688 samples, hop
72,328, lead-in 7,680), `bf16_weights` and `exact_f32_mfma`.

Part A holds the ingest to 44.1 kHz to the reference: `Model.resample` on the extended handle against `oracle/soxr_oracle.py`
for the rate pairs that fall on each of the resampling kernels, and the whole extended path from a 48 kHz file against the
oracle's extended restatement under `test_gpu_parity._noise_aware`.

Part B holds every newer entry point — streams through the ingest, peeks, kept and rolling transcripts, the many-stream
steps, the clips calls, FLAC, IMA ADPCM and G.711, the file job, the window-range split — to the one-shot call
`predict_pcm_raw` of THE SAME handle, bit for bit: maps as uint32, events as the records `test_gpu_clips_events._records`
forms (frames, pitch, the amplitude's bits, times, bends) or, where the entry point returns event tuples, the same fields of
the tuples.  The one-shot calls themselves are held to the oracle by Part A, tests/test_gpu_parity.py, test_gpu_levels.py and
test_gpu_other_weights.py.

A handle's geometry is read from the handle (`sample_rate`, `audio_n_samples`); hop and lead-in are the reference's 36,164
and 3,840 samples times rate / 22,050.  Signals are `clip_files.tones` at 0.85 of full scale, at most three windows long;
every comparison of maps first asserts `note.max() > 0.3` and every comparison of events at least one event per clip that
has rows."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import adpcm_files as AF
import clip_files as CF
import container_files as K
import flac_writer as FW
from oracle import bp_oracle as O
from test_gpu_clips_events import _records
from test_gpu_parity import _noise_aware

pytestmark = pytest.mark.gpu

MODES = ("ext_cqt_44k", "bf16_weights", "exact_f32_mfma")
MAPS = ("note", "onset", "contour")
DECODING = (0.5, 0.3, 127.70, None, None, False, True, 120)  # predict()'s defaults, as _output_to_notes takes them


@pytest.fixture(scope="module")
def nat():
    from basic_pitch_amd import _native

    return _native


@pytest.fixture(scope="module")
def handles():
    """One handle per mode at max_windows = 8, made when first asked for, all closed at the end of the module."""
    from basic_pitch_amd.inference import Model

    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = Model(device=0, max_windows=8, **{mode: True})
        return made[mode]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(params=MODES)
def model(request, handles):
    return handles(request.param)


@pytest.fixture
def ext(handles):
    return handles("ext_cqt_44k")


# ---- geometry and signals --------------------------------------------------------------------------------------------------
def geometry(m):
    """(rate, window, hop, lead-in) of a handle: rate and window from the handle, hop and lead-in the reference's times
    rate / 22050."""
    rate, win = m.sample_rate, m.audio_n_samples
    assert rate % 22050 == 0
    hop, lead = 36164 * rate // 22050, 3840 * rate // 22050
    assert win == hop + 2 * lead
    return rate, win, hop, lead


def frames_for(n_model, sr, rate):
    """The most frames at `sr` that become at most `n_model` samples at `rate` (ceil(frames * rate / sr) <= n_model)."""
    return n_model * sr // rate


def music(n, channels, rate, seed, level=0.85):
    """clip_files.tones scaled so that its peak is `level` of full scale: float64 [n, channels]."""
    x = CF.tones(n, channels, rate, seed)
    return x * (level / np.abs(x).max()) if n else x


def s16(x):
    return np.clip(np.round(np.asarray(x) * 32767), -32768, 32767).astype(np.int16)


def same_maps(got, ref, what):
    for k in MAPS:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (what, k)


def loud(maps, what):
    assert maps["note"].shape[0] > 0 and maps["note"].max() > 0.3, (what, maps["note"].shape)


def tuples(events):
    """Note-event tuples (start_s, end_s, pitch, amplitude, bends) in a form that compares bit for bit."""
    return [(np.float64(e[0]).tobytes(), np.float64(e[1]).tobytes(), int(e[2]), np.float32(e[3]).tobytes(),
             None if e[4] is None else [int(b) for b in e[4]]) for e in events]


def host_events(maps):
    """The host decode of maps under predict()'s defaults: the tuples of inference._output_to_notes."""
    from basic_pitch_amd import inference as I

    return I._output_to_notes({k: np.array(maps[k]) for k in MAPS}, *DECODING)[1]


def host_records(maps, first_row=0):
    """The host decode (bp_notes_decode) of maps whose row 0 is absolute row `first_row`, as a whole track: the records of
    test_gpu_clips_events._records with absolute frames and the times of the absolute frames."""
    from basic_pitch_amd import note_creation as NC

    ev, bends, n = NC._decode(np.array(maps["note"]), np.array(maps["onset"]), np.array(maps["contour"]), 0.5, 0.3, 11, True, None,
                              None, True, NC.ENERGY_TOLERANCE, True)
    recs = _records(ev, bends, 0, n, True)
    if first_row == 0:
        return recs
    out = []
    for r in recs:
        t = NC.frames_to_time_at(np.array([r[0] + first_row, r[1] + first_row]))
        out.append((r[0] + first_row, r[1] + first_row, r[2], r[3], float(t[0]), float(t[1])) + r[6:])
    return out


def tuples_of_records(recs):
    return [(np.float64(r[4]).tobytes(), np.float64(r[5]).tobytes(), int(r[2]), r[3], list(r[8])) for r in recs]


_CENTRE = {}


def ready_samples(pushed, sr, rate):
    """Samples of the handle-rate signal that exist once `pushed` frames at `sr` have arrived: all of them at the handle's own
    rate; through the resampler sample k needs every input frame of its sum, k * down + centre <= pushed * up - 1 (DESIGN.md
    "When a row is final"), centre = the middle tap of the filter design (`audio.soxr_hq_taps`, the host copy of it)."""
    if sr == rate:
        return pushed
    from basic_pitch_amd import audio as A

    fr = Fraction(rate, sr)
    up, down = fr.numerator, fr.denominator
    if (up, down) not in _CENTRE:
        _CENTRE[(up, down)] = (len(A.soxr_hq_taps(up, down)) - 1) // 2
    t = pushed * up - 1 - _CENTRE[(up, down)]
    return 0 if t < 0 else t // down + 1


def rows_emitted(n, win, hop, lead):
    """complete windows x 142 of a stream whose handle-rate signal has n samples."""
    return 0 if n < win - lead else ((n - (win - lead)) // hop + 1) * 142


def pushes(n):
    """Uneven push sizes that sum to n: a zero-length push, a single frame, a few frames, thirds."""
    sizes = [0, 1, 4099, n // 3, 0, 12345, 1]
    rest = n - sum(sizes)
    assert rest > 2
    return sizes + [rest // 2, rest - rest // 2, 0]


def run_stream(s, data, sizes, after_push=None):
    """Push data [n, channels] in pieces of `sizes` frames, finish: (the parts, the concatenated rows)."""
    parts, at = [], 0
    for k in sizes:
        parts.append(s.push(data[at : at + k]))
        at += k
        if after_push:
            after_push(at)
    assert at == len(data)
    parts.append(s.finish())
    return parts, {k: np.concatenate([p[k] for p in parts]) for k in MAPS}


# ---- Part A 1: Model.resample to 44.1 kHz against the float64 restatement of the filter design ----------------------------
RESAMPLE_CASES = ((88200, 1, 40001), (176400, 1, 30000), (22050, 2, 30000), (11025, 2, 5000), (48000, 2, 48001), (96000, 1, 20000),
                  (8000, 1, 999), (16000, 3, 4000), (32000, 1, 1), (44101, 1, 600),
                  # 8 : 1 (the tiled kernel, taps in memory) and 16 : 1 (the one-thread-per-output kernel)
                  (352800, 1, 40000), (705600, 1, 40000))


def _noise_and_sine(sr, ch, n, seed=3):
    rng = np.random.default_rng(seed)
    pcm = rng.uniform(-1, 1, (n, ch)).astype(np.float32)
    pcm[:, 0] += 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr).astype(np.float32)
    mono = pcm.mean(axis=1, dtype=np.float32) if ch > 1 else pcm[:, 0]
    return pcm, np.ascontiguousarray(mono)


@pytest.mark.parametrize("sr,ch,n", RESAMPLE_CASES)
def test_resample_to_44100_against_the_oracle(ext, sr, ch, n):
    """max |got - oracle| <= 1e-6: float64 taps and accumulation, one rounding to fp32 — the bound test_device_audio_ingest
    holds for the 22.05 kHz target.  The same bound against the host copy of the design."""
    from basic_pitch_amd import audio as A
    from oracle import soxr_oracle as S

    assert ext.sample_rate == 44100
    pcm, mono = _noise_and_sine(sr, ch, n)
    ref = S.resample(mono, sr, 44100)
    got = ext.resample(pcm, sr)
    assert got.shape == ref.shape == (int(np.ceil(n * 44100 / sr)),), (sr, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    host = float(np.abs(got - A.resample(mono, sr, 44100)).max())
    print(f"resample {sr} Hz x{ch} n={n} -> 44100: max|got - oracle| = {err:.3e}, max|got - host copy| = {host:.3e}, "
          f"peak |oracle| = {float(np.abs(ref).max()):.3f}")
    assert err <= 1e-6, (sr, ch, n, err)
    assert host <= 1e-6, (sr, ch, n, host)


def test_input_at_44100_is_the_channel_mean_bit_for_bit(ext):
    pcm, mono = _noise_and_sine(44100, 2, 5000)
    got = ext.resample(pcm, 44100)
    assert got.shape == mono.shape and np.array_equal(got.view(np.uint32), mono.view(np.uint32))


# ---- Part A 2: the whole extended path from a 48 kHz file --------------------------------------------------------------------
def test_the_extended_path_from_48_khz_against_the_oracle(ext, nat, weights):
    """48 kHz stereo S16 of about 2.3 extended hops through predict_pcm_raw: bit for bit predict_track(resample(...)), and
    against the oracle — soxr_oracle's 44.1 kHz signal windowed on the host with hop 72,328 and lead-in 7,680, O.forward(ext)
    in fp64 and fp32, rows 15..157 un-overlapped — under test_gpu_parity._noise_aware.

    Measured on an MI355X (this test, -s), |hip - fp64| / |fp32 - fp64| / bound: note 1.7e-4 / 6.4e-4 / 1.3e-3, onset
    2.0e-4 / 8.0e-4 / 1.6e-3, contour 2.9e-4 / 1.0e-3 / 2.1e-3 (tonal input: the fp32 oracle's own distance sets the bound)."""
    from oracle import soxr_oracle as S

    rate, win, hop, lead = geometry(ext)
    assert (rate, win, hop, lead) == (44100, O.EXT_AUDIO_N_SAMPLES, 72328, 7680)
    n = frames_for(int(2.3 * hop), 48000, rate)
    pcm = s16(music(n, 2, 48000, 5))
    got = ext.predict_pcm_raw(pcm, nat.BP_PCM_S16, n, 2, 48000)
    f32 = pcm.astype(np.float32) / np.float32(32768)
    same_maps(got, ext.predict_track(ext.resample(f32, 48000)), "predict_track(resample)")
    loud(got, "48 kHz")
    mono = f32.mean(axis=1, dtype=np.float32)
    y = np.asarray(S.resample(mono, 48000, 44100), np.float32)
    L = y.shape[0]
    assert L == int(np.ceil(n * 44100 / 48000))
    n_win = -(-(L + lead) // hop)
    assert n_win == 3
    wins, _ = O.window_track(y, win=win, hop=hop, lead=lead)
    assert wins.shape == (n_win, win)
    unwrap = lambda r: {k: O.unwrap_output(np.asarray(r[k]), L, win=win, hop=hop, lead=lead) for k in MAPS}  # noqa: E731
    r64 = unwrap(O.forward(wins, weights, np.float64, ext=True))
    r32 = unwrap(O.forward(wins, weights, np.float32, ext=True))
    for k in MAPS:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        ours, orc = float(np.abs(got[k] - r64[k]).max()), float(np.abs(r32[k] - r64[k]).max())
        print(f"extended path from 48 kHz, {k}: |hip - fp64| = {ours:.3e}, |fp32 - fp64| = {orc:.3e}, bound = {max(1e-4, 2 * orc):.3e}")
    _noise_aware(got, r32, r64)


# ---- Part B 1: streams through the ingest -------------------------------------------------------------------------------------
def _stream_inputs(m, nat):
    """(name, data [n, channels], format, channels, rate) of about 2.3 hops of the handle: three windows."""
    rate, win, hop, lead = geometry(m)
    L = 2 * hop + hop // 3
    n48 = frames_for(L, 48000, rate)
    out = [("s16 stereo 48000", s16(music(n48, 2, 48000, 11)), nat.BP_PCM_S16, 2, 48000)]
    if rate == 44100:
        n22, n88 = frames_for(L, 22050, rate), frames_for(L, 88200, rate)
        out.append(("f32 mono 22050", music(n22, 1, 22050, 12).astype(np.float32), nat.BP_PCM_F32, 1, 22050))
        out.append(("s16 mono 88200", s16(music(n88, 1, 88200, 13)), nat.BP_PCM_S16, 1, 88200))
    return out


def test_streams_through_the_ingest_equal_the_one_shot_call(model, nat):
    rate, win, hop, lead = geometry(model)
    for name, data, fmt, ch, sr in _stream_inputs(model, nat):
        n = data.shape[0]
        ref = model.predict_pcm_raw(data, fmt, n, ch, sr)
        loud(ref, name)
        assert ref["note"].shape[0] > 2 * 142  # three windows
        with model.open_stream(sr, ch, fmt) as s:
            def rows_are_the_complete_windows(pushed):
                want = rows_emitted(ready_samples(pushed, sr, rate), win, hop, lead)
                assert s.rows == want, (name, pushed, s.rows, want)

            _, got = run_stream(s, data, pushes(n), rows_are_the_complete_windows)
            assert s.rows == ref["note"].shape[0]
        same_maps(got, ref, name)


# ---- Part B 2: peek -------------------------------------------------------------------------------------------------------------
def test_a_peek_inside_the_second_window_gives_the_prefix_and_changes_nothing(model, nat):
    rate, win, hop, lead = geometry(model)
    n = frames_for(2 * hop + hop // 3, 48000, rate)
    data = s16(music(n, 2, 48000, 21))
    cut = frames_for(hop + hop // 2, 48000, rate)  # window 1 covers [hop - lead, 2 * hop + lead): inside it, window 0 complete
    sizes = [cut // 2, cut - cut // 2, (n - cut) // 2, n - cut - (n - cut) // 2]
    with model.open_stream(48000, 2, nat.BP_PCM_S16) as s, model.open_stream(48000, 2, nat.BP_PCM_S16) as plain:
        parts = [s.push(data[: sizes[0]]), s.push(data[sizes[0] : cut])]
        assert s.rows == 142
        peeked = s.peek()
        prefix = model.predict_pcm_raw(data[:cut], nat.BP_PCM_S16, cut, 2, 48000)
        loud(prefix, "prefix")
        assert peeked["note"].shape[0] == prefix["note"].shape[0] - 142 > 0
        same_maps({k: np.concatenate([p[k] for p in parts] + [peeked[k]]) for k in MAPS}, prefix, "emitted + peek")
        parts += [s.push(data[cut : cut + sizes[2]]), s.push(data[cut + sizes[2] :]), s.finish()]
        never_peeked, whole = run_stream(plain, data, sizes)
    for i, (p, q) in enumerate(zip(parts, never_peeked)):
        same_maps(p, q, ("push", i))
    same_maps(whole, model.predict_pcm_raw(data, nat.BP_PCM_S16, n, 2, 48000), "whole")


# ---- Part B 3: kept and rolling streams, the many-stream steps -----------------------------------------------------------------
def test_kept_and_rolling_streams_of_two_rates_on_one_handle(model, nat):
    """A stream kept in full (22,050 Hz mono float) and a rolling one (48 kHz stereo S16, a horizon of 2 s under a signal of
    about 4 s) advance through push_streams; twins without retention advance alone.  After every step the rows and the peeks
    are the twins'; `streaming.streams_events` and `streaming.transcripts` (host and device decode) give each stream the
    events of the host decode of its own maps: the one-shot call on the prefix for the kept stream, `rolling_maps` for the
    rolling one."""
    from basic_pitch_amd import streaming
    from basic_pitch_amd.streaming import StreamingTranscriber

    rate, win, hop, lead = geometry(model)
    L = 2 * hop + hop // 3
    nk, nr = frames_for(L, 22050, rate), frames_for(L, 48000, rate)
    xk, xr = music(nk, 1, 22050, 31).astype(np.float32), s16(music(nr, 2, 48000, 32))
    cuts = (0.22, 0.61, 1.0)
    with StreamingTranscriber(model, 22050, 1, nat.BP_PCM_F32, live=True, max_rows=1024) as tk, \
            StreamingTranscriber(model, 48000, 2, nat.BP_PCM_S16, live=True, horizon_seconds=2.0) as tr, \
            model.open_stream(22050, 1, nat.BP_PCM_F32) as bk, model.open_stream(48000, 2, nat.BP_PCM_S16) as br:
        H = tr.horizon_rows
        assert H == 173
        at_k = at_r = 0
        checked = 0
        for step, frac in enumerate(cuts):
            to_k, to_r = int(nk * frac), int(nr * frac)
            together = streaming.push_streams(model, [tk.stream, tr.stream], [xk[at_k:to_k], xr[at_r:to_r]])
            alone = [bk.push(xk[at_k:to_k]), br.push(xr[at_r:to_r])]
            at_k, at_r = to_k, to_r
            for g, w in zip(together, alone):
                same_maps(g, w, ("push_streams", step))
            assert (tk.stream.rows, tr.stream.rows) == (bk.rows, br.rows)
            peeks = streaming.peek_streams(model, [tk.stream, tr.stream])
            for g, w in zip(peeks, [bk.peek(), br.peek()]):
                same_maps(g, w, ("peek_streams", step))
            if step == 0:
                continue
            # the maps each stream's events are decoded from
            prefix = model.predict_pcm_raw(xk[:at_k], nat.BP_PCM_F32, at_k, 1, 22050)
            loud(prefix, "kept prefix")
            assert prefix["note"].shape[0] == tk.stream.rows + peeks[0]["note"].shape[0]
            a, kept = tr.stream.rolling_maps()
            T = tr.stream.rows + peeks[1]["note"].shape[0]
            assert a == max(0, T - H) and kept["note"].shape[0] == T - a
            one_shot_r = model.predict_pcm_raw(xr[:at_r], nat.BP_PCM_S16, at_r, 2, 48000)
            same_maps(kept, {k: one_shot_r[k][a:T] for k in MAPS}, ("rolling_maps", step))
            loud(kept, "rolling slice")
            want = [host_records(prefix), host_records(kept, a)]
            assert all(len(w) >= 1 for w in want), [len(w) for w in want]
            tab, events, bends, offs = streaming.streams_events(model, [tk.stream, tr.stream])
            for i in range(2):
                assert tab[i].status == 0 and (tab[i].first_row, tab[i].n_rows) == ((0, prefix["note"].shape[0]), (a, T))[i]
                assert _records(events, bends, int(offs[i]), int(offs[i + 1]), True) == want[i], (step, i)
            for decode in ("host", "device"):
                res = streaming.transcripts(model, [tk, tr], decode=decode)
                for i in range(2):
                    assert tuples(res[i][1]) == tuples_of_records(want[i]), (step, decode, i)
                    assert sum(len(inst.notes) for inst in res[i][0].instruments) == len(want[i])
            assert tuples(host_events(prefix)) == tuples_of_records(want[0])  # the two host forms agree
            checked += 1
            if step == len(cuts) - 1:
                assert a > 0  # the horizon is shorter than the signal
        assert checked == 2


# ---- Part B 4: clips --------------------------------------------------------------------------------------------------------------
def _clips(m, nat):
    """Six clips at two rates, one the handle's own: [(samples, rate)].  Five are numpy arrays `transcribe_clips` takes (S16
    stereo 48 kHz; F32 mono of three windows; U8 mono of exactly hop - lead samples; an empty one; S16 mono of two windows, the
    last three at the handle's rate); the sixth is packed big-endian 24-bit stereo at 48 kHz, which has no numpy type."""
    rate, win, hop, lead = geometry(m)
    n0 = frames_for(hop + hop // 3, 48000, rate)
    x2 = music(frames_for(hop // 2, 48000, rate), 2, 48000, 43)
    return [
        (s16(music(n0, 2, 48000, 41)), 48000),
        (music(2 * hop + hop // 3, 1, rate, 42).astype(np.float32), rate),
        (K.encode(x2, K.S24_BE), 48000),
        (np.clip(np.round(music(hop - lead, 1, rate, 44) * 127) + 128, 0, 255).astype(np.uint8), rate),
        (np.zeros((0, 1), np.int16), rate),
        (s16(music(hop + hop // 5, 1, rate, 45)), rate),
    ]


def _alone(m, a, rate):
    from basic_pitch_amd import clips as CL

    a = CL.as_clip(a, 0)
    return m.predict_pcm_raw(a, CL.FORMATS[a.dtype], a.shape[0], a.shape[1], rate)


def test_transcribe_clips_gives_each_clip_the_events_of_the_one_shot_call(model, nat):
    from basic_pitch_amd import clips as CL

    rate, win, hop, lead = geometry(model)
    job = _clips(model, nat)
    ids = [0, 1, 3, 4, 5]
    clips, rates = [job[i][0] for i in ids], [job[i][1] for i in ids]
    want = []
    for c, r in zip(clips, rates):
        out = _alone(model, c, r)
        if len(c):
            loud(out, (c.dtype, r))
        want.append(host_events(out))
        assert len(want[-1]) >= 1 or len(c) == 0
    assert want[ids.index(4)] == []
    windows = lambda n: -(-(n + lead) // hop)  # noqa: E731
    assert windows(len(clips[2])) == 1 and windows(len(clips[2]) + 1) == 2 and windows(len(clips[1])) == 3
    for decode in ("host", "device"):
        got = model.transcribe_clips(clips, rates, decode=decode)
        assert len(got) == len(clips)
        for i, (g, w) in enumerate(zip(got, want)):
            assert tuples(g[1]) == tuples(w), (decode, i)
            assert sum(len(inst.notes) for inst in g[0].instruments) == len(w)
    # the row offsets on the handle are those of the handle's geometry
    for r in (48000, rate):
        arrays = [CL.as_clip(c, i) for i, (c, cr) in enumerate(zip(clips, rates)) if cr == r]
        offs = CL.clips_row_offsets(model, arrays, r)
        assert np.array_equal(offs, CL.row_offsets([a.shape[0] for a in arrays], r, model_rate=rate, hop=hop, lead=lead)), r
        assert offs[-1] > 0


def test_a_packed_big_endian_24_bit_clip_in_a_job_of_clips(model, nat):
    """Packed 24-bit PCM has no numpy type, so `transcribe_clips` cannot be handed it (clips.py FORMATS): the clip goes to the
    native calls beneath it, `bp_infer_clips_candidates` and `bp_infer_clips_events`, in one job with the S16 clip of its rate."""
    from basic_pitch_amd import clips as CL, events as EV, note_creation as NC

    job = _clips(model, nat)
    (a0, _), (raw, _) = job[0], job[2]
    a0 = CL.as_clip(a0, 0)
    n2 = raw.size // 6
    tab = (CL.bp_clip * 2)()
    tab[0] = CL.bp_clip(a0.ctypes.data, a0.shape[0], nat.BP_PCM_S16, 2)
    tab[1] = CL.bp_clip(raw.ctypes.data, n2, nat.BP_PCM_S24_BE, 2)
    outs = [_alone(model, a0, 48000), model.predict_pcm_raw(raw, nat.BP_PCM_S24_BE, n2, 2, 48000)]
    for o in outs:
        loud(o, "48 kHz clip")
    want = [host_events(o) for o in outs]
    assert all(len(w) >= 1 for w in want)
    lib = EV.bind(CL.bind(model._lib))
    prm = NC._note_params(0.5, 0.3, 11, True, None, None, True, NC.ENERGY_TOLERANCE, True)
    offs = np.zeros(3, np.int64)
    nat.check(lib, model._handle, lib.bp_clips_row_offsets(model._handle, 2, tab, 48000, offs.ctypes.data_as(C.POINTER(C.c_int64))),
              "bp_clips_row_offsets")
    assert np.diff(offs).tolist() == [o["note"].shape[0] for o in outs]
    fixed = (model._handle, 2, tab, 48000, nat.BP_MEM_HOST)
    _, note, bits, bend, status = CL._call(lib, model._handle, "bp_infer_clips_candidates", lib.bp_infer_clips_candidates, fixed, offs, prm)
    assert status.tolist() == [0, 0]
    for i in range(2):
        r0, r1 = int(offs[i]), int(offs[i + 1])
        assert tuples(NC.decode_candidates(note[r0:r1], bits[r0:r1], bend[r0:r1], prm)) == tuples(want[i]), i
    events, bends, ev_offs, status = EV._call(lib, model._handle, "bp_infer_clips_events", lib.bp_infer_clips_events,
                                              fixed + (C.addressof(prm),), 2, int(offs[-1]))
    assert status.tolist() == [0, 0]
    for i in range(2):
        assert tuples(EV.clip_events(events, bends, ev_offs, i, True)) == tuples(want[i]), i


# ---- Part B 5: FLAC ---------------------------------------------------------------------------------------------------------------
def _flac(n, channels, rate, seed, blocksize):
    pcm = np.round(music(n, channels, rate, seed) * 32767).astype(np.int64)
    return FW.encode(pcm, rate, 16, blocksize=blocksize)


def test_flac_on_the_device_equals_the_host_decoders_samples(model, nat):
    from basic_pitch_amd import flac_clips

    blobs = [_flac(40000, 2, 44100, 51, 1152), _flac(36000, 1, 48000, 52, 4096)]
    host = [flac_clips.host_decode(model._lib, b) for b in blobs]
    assert [(h[0].shape, h[1]) for h in host] == [((40000, 2), 44100), ((36000, 1), 48000)]
    for b, (pcm, sr) in zip(blobs, host):
        want = model.predict_pcm_raw(pcm, nat.BP_PCM_F32, pcm.shape[0], pcm.shape[1], sr)
        loud(want, sr)
        same_maps(model.predict_flac(b), want, sr)
    for decode in ("host", "device"):
        want = model.transcribe_clips([h[0] for h in host], [h[1] for h in host], decode=decode)
        got = model.transcribe_flac_clips(blobs, decode=decode)
        for i in range(2):
            assert len(want[i][1]) >= 1
            assert tuples(got[i][1]) == tuples(want[i][1]), (decode, i)
    assert tuples(want[0][1]) == tuples(host_events(model.predict_pcm_raw(host[0][0], nat.BP_PCM_F32, 40000, 2, 44100)))


# ---- Part B 6: IMA ADPCM and G.711 ------------------------------------------------------------------------------------------------
def test_adpcm_and_g711_equal_the_s16_route(model, nat, tmp_path):
    from basic_pitch_amd import adpcm_clips, inference as I

    rate, win, hop, lead = geometry(model)
    blobs = [AF.ima_wav(s16(music(frames_for(hop + hop // 4, 44100, rate), 2, 44100, 61)), 44100, 2048),
             AF.ima4_caf(s16(music(frames_for(hop // 2, 22050, rate), 1, 22050, 62)), 22050)]
    for b in blobs:
        pcm, lay = adpcm_clips.host_decode(model._lib, b)
        want = model.predict_pcm_raw(pcm, nat.BP_PCM_S16, lay["n_frames"], lay["channels"], lay["sample_rate"])
        loud(want, lay)
        same_maps(model.predict_adpcm(b), want, lay)
    same_rate = [blobs[0], AF.ima_wav(s16(music(frames_for(hop // 2, 44100, rate), 2, 44100, 63)), 44100, 2048)]
    dev, host = model.transcribe_adpcm_clips(same_rate, decode="device"), model.transcribe_adpcm_clips(same_rate, decode="host")
    for i, (d, h) in enumerate(zip(dev, host)):
        assert len(h[1]) >= 1 and tuples(d[1]) == tuples(h[1]), i
    pcm0, lay0 = adpcm_clips.host_decode(model._lib, blobs[0])
    assert tuples(host[0][1]) == tuples(host_events(model.predict_pcm_raw(pcm0, nat.BP_PCM_S16, lay0["n_frames"], 2, 44100)))
    # mu-law in an AU file through run_inference: the expanded samples through the S16 route
    n = frames_for(hop + hop // 4, 8000, rate)
    codes = K.encode(music(n, 1, 8000, 64), K.ULAW)
    path = tmp_path / "u.au"
    path.write_bytes(K.au_of(codes, K.ULAW, 1, 8000))
    expanded = K.ULAW_TABLE[codes].astype(np.int16)
    want = model.predict_pcm_raw(expanded, nat.BP_PCM_S16, n, 1, 8000)
    loud(want, "mu-law")
    same_maps(I.run_inference(str(path), model), want, "mu-law AU")


# ---- Part B 7: the file job -------------------------------------------------------------------------------------------------------
def test_the_file_job_writes_the_same_bytes_per_file_and_batched(model, nat, tmp_path):
    from basic_pitch_amd import inference as I, transcribe_files

    rate, win, hop, lead = geometry(model)
    d = tmp_path / "in"
    d.mkdir()
    paths = [CF.write_wav(d / "a_s16_44k.wav", music(frames_for(hop - lead, 44100, rate), 2, 44100, 71), "s16", 44100)]
    x = music(frames_for(hop // 2, 48000, rate), 2, 48000, 72)
    (d / "b_s24_48k.aiff").write_bytes(K.aiff_of(K.encode(x, K.S24_BE), K.S24_BE, 2, 48000))
    (d / "c_16_44k.flac").write_bytes(_flac(30000, 2, 44100, 73, 1152))
    (d / "d_ima_44k.wav").write_bytes(AF.ima_wav(s16(music(frames_for(hop // 2, 44100, rate), 1, 44100, 74)), 44100, 1024))
    paths += [str(d / "b_s24_48k.aiff"), str(d / "c_16_44k.flac"), str(d / "d_ima_44k.wav"),
              CF.write_wav(d / "e_f32_22k.wav", music(frames_for(2 * hop + hop // 3, 22050, rate), 1, 22050, 75), "f32", 22050)]
    want = [I.predict(p, model) for p in paths]
    for p, (mo, _, ev) in zip(paths, want):
        loud(mo, p)
        assert len(ev) >= 1, p
    assert want[4][0]["note"].shape[0] > 2 * 142
    listings = []
    for clip_batch in (0, 4):
        out = tmp_path / f"out{clip_batch}"
        out.mkdir()
        rep = transcribe_files(paths, str(out), models=[model], threads=2, clip_batch=clip_batch)
        for p, r, (mo, _, ev) in zip(paths, rep, want):
            assert r["status"] == 0 and r["message"] == "", (clip_batch, p, r)
            assert (r["n_frames"], r["n_note_events"]) == (mo["note"].shape[0], len(ev)), (clip_batch, p, r)
        listings.append({name: open(os.path.join(out, name), "rb").read() for name in sorted(os.listdir(out))})
    assert sorted(listings[0]) == sorted(listings[1]) and len(listings[0]) == 10
    for name in listings[0]:
        assert listings[0][name] == listings[1][name], name


# ---- Part B 8: window ranges -------------------------------------------------------------------------------------------------------
def test_a_file_split_by_window_range_equals_the_unsplit_file(model, nat, tmp_path):
    from basic_pitch_amd import inference as I

    rate, win, hop, lead = geometry(model)
    path = CF.write_wav(tmp_path / "three.wav", music(frames_for(2 * hop + hop // 3, 48000, rate), 2, 48000, 81), "s16", 48000)
    whole = I.run_inference(path, model)
    loud(whole, "three windows")
    parts = [I.predict_window_range(path, model, piece, 2) for piece in range(2)]
    assert parts[0]["n_windows"] == 3 and [p["range"] for p in parts] == [(0, 2), (2, 3)]
    got, midi, events = I.assemble_window_ranges(parts[::-1])
    same_maps(got, whole, "window ranges")
    want = host_events(whole)
    assert len(want) >= 1 and tuples(events) == tuples(want)
