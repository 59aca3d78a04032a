"""Rolling live transcripts on the GPU (bp_stream_keep_rolling / bp_stream_candidates_rolling / bp_stream_rolling_maps,
include/basic_pitch_amd_rolling.h; StreamingTranscriber(horizon_seconds=...)): at any moment the transcript is bit for bit the
host decoder's answer for the last H rows of the one-shot maps of the audio so far, decoded as a whole track, in absolute
frames and times; the stream is otherwise untouched, and nothing it owns grows.  H = 300 rows and a track of 1,205 rows in 9
windows: the ring of H + 284 slots wraps twice.  Every test does ordinary work; refusals are argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import note_oracle as NO

pytestmark = pytest.mark.gpu

HOP, WIN, LEAD = 36164, 43844, 3840
MAPS = ("note", "onset", "contour")
DECODING = (0.5, 0.3, 127.70, None, None, False, True, 120)  # predict()'s defaults, as _output_to_notes takes them
H, CAP = 300, 300 + 2 * 142
N = 307_000  # 13.9 s at 22.05 kHz: int(N / 36164 * 142) = 1205 rows
# irregular chunks: one sample, a few, fractions of a window, more than a window (43,844 samples)
CHUNKS = (1, 4099, 50_000, 12_345, 1, 30_011, 7, 47_000, 22_050, 4099, 36_164, 9_000, 1, 44_000, 15_000, 20_000, 13_222)
assert sum(CHUNKS) == N


def melody(n=N, seed=11):
    """Overlapping harmonic tones (three partials, 110 ... 880 Hz, 0.2 ... 1.5 s, every third or so a semitone above the one
    before, each starting before the last has ended) over 1e-3 noise.  With the CPU restatement of the model (oracle/bp_oracle.py)
    and H = 300, slices cut every 71 rows hold 5 to 12 events and 11 of the 12 with a > 0 decode differently from the whole
    prefix restricted to the slice."""
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal(n)
    at, prev = 0.0, 45
    while at < n / 22050.0:
        midi = min(81, prev + 1 if rng.random() < 0.3 else int(rng.integers(45, 82)))
        prev = midi
        f0 = 440.0 * 2 ** ((midi - 69) / 12)
        ln = float(rng.uniform(0.2, 1.5))
        a, b = int(at * 22050), min(n, int((at + ln) * 22050))
        t = np.arange(b - a) / 22050.0
        env = np.minimum(1.0, t / 0.01) * np.minimum(1.0, (t[-1] - t) / 0.03 + 1e-3)
        x[a:b] += 0.2 * env * sum(np.sin(2 * np.pi * f0 * h * t) / h for h in (1, 2, 3))
        at += ln * float(rng.uniform(0.3, 0.8))
    return x.astype(np.float32)


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
def x():
    return melody()


@pytest.fixture(scope="module")
def prm():
    from basic_pitch_amd import note_creation as nc

    return nc._note_params(0.5, 0.3, 11, True, None, None, True, 11, True)


@pytest.fixture(scope="module")
def prefixes(model, nat, x):
    """The one-shot maps of the audio after every chunk: computed once, read by every test, never written."""
    out, at = [], 0
    for k in CHUNKS:
        at += k
        maps = model.predict_pcm_raw(x[:at], nat.BP_PCM_F32, at, 1, 22050)
        for m in MAPS:
            maps[m].setflags(write=False)
        out.append((at, maps))
    return out


def slice_events(maps, a, T, onset_threshold=0.5, base=0):
    """The contract's right-hand side: bp_notes_decode on copies of rows [a, T) of maps (whose row 0 is absolute row `base`) as
    a whole track, frames shifted by a, times of the absolute frames.
    -> [(start_frame, end_frame, start_s bits, end_s bits, pitch, amplitude bits, bends)]"""
    from basic_pitch_amd import note_creation as nc

    sl = {m: np.ascontiguousarray(maps[m][a - base : T - base]).copy() for m in MAPS}
    ev, bends, n = nc._decode(sl["note"], sl["onset"], sl["contour"], onset_threshold, 0.3, 11, True, None, None, True, 11, True)
    times = nc.model_frames_to_time(T + 1)
    return [(e.start_frame + a, e.end_frame + a, times[e.start_frame + a].tobytes(), times[e.end_frame + a].tobytes(), e.pitch_midi,
             np.float32(e.amplitude).tobytes(), bends[e.bend_offset : e.bend_offset + e.n_bends].tolist()) for e in ev[:n]]


def unwrap(ring, a, T):
    return np.ascontiguousarray(ring[np.arange(a, T) % ring.shape[0]])


def rolling_events(s, note, bits, bend, held, prm):
    """One update at the C ABI and the host half: (a, T, status, events as slice_events gives them)."""
    from basic_pitch_amd import _native

    a, T, status = s.candidates_rolling(note, bits, bend, held)
    if status != 0 or T == 0:
        return a, T, status, []
    ln, lb, ld = unwrap(note, a, T), unwrap(bits, a, T), unwrap(bend, a, T)
    events = (_native.bp_note_event * 1024)()
    bends = np.empty(1 << 16, np.int32)
    n_ev, n_b = C.c_int64(0), C.c_int64(0)
    rc = s._lib.bp_notes_decode_candidates_at(ln.ctypes.data, lb.ctypes.data, ld.ctypes.data, T - a, a, C.addressof(prm),
                                              C.addressof(events), 1024, bends.ctypes.data, bends.size, C.byref(n_ev), C.byref(n_b))
    assert rc == 0, s._lib.bp_notes_last_error()
    return a, T, status, [(e.start_frame, e.end_frame, np.float64(e.start_s).tobytes(), np.float64(e.end_s).tobytes(), e.pitch_midi,
                           np.float32(e.amplitude).tobytes(), bends[e.bend_offset : e.bend_offset + e.n_bends].tolist())
                          for e in events[: n_ev.value]]


def as_tuples(events):
    """The transcriber's note events in the comparable form of slice_events, without the frames."""
    return [(np.float64(e[0]).tobytes(), np.float64(e[1]).tobytes(), int(e[2]), np.float32(e[3]).tobytes(), list(e[4])) for e in events]


def rings(rows=CAP):
    return np.zeros((rows, 88), np.float32), np.zeros((rows, 12), np.uint8), np.zeros((rows, 88), np.int8)


# ---- 1. the contract -----------------------------------------------------------------------------------------------------------
def test_a_rolling_transcript_is_the_decode_of_the_last_rows_as_a_whole_track(model, nat, x, prm, prefixes):
    """After EVERY push, at the C ABI and through StreamingTranscriber(horizon_seconds=...).  The held-rows bookkeeping is the
    transcriber's: only rows that are new since the last update are sent."""
    from basic_pitch_amd import note_creation as nc
    from basic_pitch_amd.streaming import StreamingTranscriber

    note, bits, bend = rings()
    with_a, with_events, differs, oracle_checked, at, held = 0, 0, 0, False, 0, 0
    with model.open_stream(22050) as s, StreamingTranscriber(model, 22050, live=True, horizon_seconds=3.48) as t:
        assert t.horizon_rows == H
        s.keep_rolling(prm, H)
        shapes = None
        for k, (n_at, maps) in zip(CHUNKS, prefixes):
            s.push(x[at : at + k])
            t.push(x[at : at + k])
            at += k
            assert at == n_at
            a, T, status, got = rolling_events(s, note, bits, bend, held, prm)
            held = s.rows
            assert T == maps["note"].shape[0] and a == max(0, T - H) and status == 0, at
            ref = slice_events(maps, a, T)
            print(f"update at {at}: rows [{a}, {T}), {len(got)} events, {len(ref)} in the reference")
            assert got == ref, at
            midi, events = t.transcript()
            assert as_tuples(events) == [r[2:] for r in ref], at
            assert [len(i.notes) for i in midi.instruments] == ([len(ref)] if ref else [])
            assert t.horizon_first_time == nc.model_frames_to_time(a + 1)[a]
            assert t._rows == [] and t._held == t.stream.rows
            shapes = shapes or (t._note.shape, t._bits.shape, t._bend.shape)
            assert (t._note.shape, t._bits.shape, t._bend.shape) == shapes == ((CAP, 88), (CAP, 12), (CAP, 88))
            if a == 0:
                continue
            with_a += 1
            with_events += len(ref) >= 3
            whole = [e for e in slice_events(maps, 0, T) if e[0] >= a]
            differs += sorted(whole) != sorted(ref)
            if not oracle_checked and len(ref) >= 3:  # once: the numpy restatement of the reference on the same slice
                sl = {m: np.array(maps[m][a:T]) for m in MAPS}
                o_events, o_notes = NO.model_output_to_notes(sl, 0.5, 0.3)
                times = NO.model_frames_to_time(T + 1)
                assert [(f[0] + a, f[1] + a, times[f[0] + a].tobytes(), times[f[1] + a].tobytes(), e[2]) for e, f in
                        zip(o_events, o_notes)] == [r[:5] for r in ref]
                assert [list(e[4]) for e in o_events] == [r[6] for r in ref]
                oracle_checked = True
        assert at == N and with_a >= 5 and with_events >= 3 and differs >= 1 and oracle_checked, (with_a, with_events, differs)
        # finish: the rows finish emits and the final slice, which is the last prefix's
        last = prefixes[-1][1]
        rows, midi, events = t.finish()
        T = last["note"].shape[0]
        assert rows["note"].shape[0] == T - held and np.array_equal(rows["note"].view(np.uint32), last["note"][held:].view(np.uint32))
        assert as_tuples(events) == [r[2:] for r in slice_events(last, T - H, T)]
        s.finish()
        a, T2, status, got = rolling_events(s, note, bits, bend, held, prm)  # valid after finish: no tail, the same slice
        assert (a, T2, status) == (T - H, T, 0) and got == slice_events(last, a, T)


# ---- 2. below the horizon nothing is new -------------------------------------------------------------------------------------
def test_below_the_horizon_the_transcripts_are_those_of_the_plain_live_mode(model, x):
    from basic_pitch_amd.streaming import StreamingTranscriber

    with StreamingTranscriber(model, 22050, live=True, horizon_seconds=30.0) as r, StreamingTranscriber(model, 22050, live=True) as p:
        assert r.horizon_rows > 1205
        at, seen = 0, 0
        for k in CHUNKS:
            r.push(x[at : at + k]), p.push(x[at : at + k])
            at += k
            (m1, e1), (m2, e2) = r.transcript(), p.transcript()
            assert as_tuples(e1) == as_tuples(e2), at
            assert m1.to_bytes() == m2.to_bytes(), at
            assert r.horizon_first_time == 0.0
            seen += len(e1)
        assert seen > 50
        _, m1, e1 = r.finish()
        _, m2, e2 = p.finish()
        assert as_tuples(e1) == as_tuples(e2) and m1.to_bytes() == m2.to_bytes()


# ---- 3. the stream is otherwise untouched ------------------------------------------------------------------------------------
def test_a_rolling_stream_emits_the_bytes_of_a_plain_stream(model, x, prm):
    note, bits, bend = rings()
    runs = []
    for rolling in (True, False):
        with model.open_stream(22050) as s:
            if rolling:
                s.keep_rolling(prm, H)
            parts, at = [], 0
            for i, k in enumerate(CHUNKS):
                parts.append(s.push(x[at : at + k]))
                at += k
                if rolling:
                    s.candidates_rolling(note, bits, bend, 0)
                    if i % 3 == 0:  # a peek between two updates changes no later bytes
                        s.peek()
                    a, T, _ = s.candidates_rolling(note, bits, bend, 0)
                    if i == 9:
                        a2, maps = s.rolling_maps()
                        assert a2 == a and maps["note"].shape[0] == T - a
                        assert np.array_equal(maps["note"].view(np.uint32), unwrap(note, a, T).view(np.uint32))
            parts.append(s.finish())
        runs.append(parts)
    for i, (p, q) in enumerate(zip(*runs)):
        for m in MAPS:
            assert p[m].shape == q[m].shape and np.array_equal(p[m].view(np.uint32), q[m].view(np.uint32)), (i, m)
    assert sum(p["note"].shape[0] for p in runs[0]) == 1205


def test_rows_reach_a_host_ring_of_another_size_than_the_device_ring(model, prm):
    """The note rows of an update are gathered from their slots and copied home, split wherever the host ring wraps, and the
    two rings wrap at different rows: H = 200, so 484 slots on the device, beside host rings of 484 + 37 rows.  Twelve pushes of one to two
    hops of seeded noise (at least 1,562 rows: both rings wrap twice and more); held_rows runs with the final rows.  The new
    rows [max(held_rows, a), T) of an update cross a wrap of the device ring in some updates, of the host ring in others and
    of both in at least one: counted here from the row numbers.  After every update the slice of all three rings is, byte
    for byte, that of an update into fresh rings that hold nothing (held_rows = 0)."""
    from basic_pitch_amd import note_creation as nc

    rng = np.random.default_rng(5)
    note, bits, bend = rings(484 + 37)
    with model.open_stream(22050) as s:
        s.keep_rolling(prm, 200)
        held, n_events, wraps = 0, 0, []
        for _ in range(12):
            s.push((0.1 * rng.standard_normal(int(rng.integers(HOP, 2 * HOP + 1)))).astype(np.float32))
            a, T, status = s.candidates_rolling(note, bits, bend, held)
            n0 = max(held, a)
            wraps.append((n0 // 484 != (T - 1) // 484, n0 // 521 != (T - 1) // 521))
            held = s.rows
            a2, maps = s.rolling_maps()
            assert (a2, status) == (a, 0) and a == max(0, T - 200) and maps["note"].shape[0] == T - a
            assert np.array_equal(unwrap(note, a, T).view(np.uint32), maps["note"].view(np.uint32)), T
            fresh = rings(484 + 37)
            assert s.candidates_rolling(*fresh, 0) == (a, T, 0)
            for ring, whole in zip((note, bits, bend), fresh):
                assert np.array_equal(unwrap(ring, a, T).view(np.uint8), unwrap(whole, a, T).view(np.uint8)), T
            got = nc.decode_candidates(unwrap(note, a, T), unwrap(bits, a, T), unwrap(bend, a, T), prm, first_frame=a)
            ref = slice_events(maps, a, T, base=a)
            print(f"rows [{a}, {T}): {len(got)} events, {len(ref)} in the reference")
            assert as_tuples(got) == [r[2:] for r in ref], T
            n_events += len(ref)
        assert s.rows >= 2 * (484 + 37) + 484, s.rows
        assert sum(d for d, _ in wraps) >= 2 and sum(h for _, h in wraps) >= 2 and (True, True) in wraps, wraps
        assert n_events > 0


# ---- 3b. the smallest one-stream shapes: a handle of ONE window, so a tail of two windows takes two rounds of the peek step ----
@pytest.fixture(scope="module")
def tiny():
    from basic_pitch_amd.inference import Model

    m = Model(max_windows=1)
    yield m
    m.close()


def same_bytes(got, want):
    return all(g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_a_rolling_stream_alone_on_a_handle_of_one_window(tiny, nat, x, prm):
    """horizon_rows = 3 (287 slots), nothing final at any update.  One sample: bp_track_n_frames(1) = int(1 / 36164 * 142) = 0
    rows, so the call returns before the step and writes nothing.  HOP - LEAD = 32,324 samples are the longest signal of one
    window, 32,325 the shortest of two: 126 rows either way, the slice is rows [123, 126).  Each update is held to the host
    decoder on the one-shot maps (three rows hold no note of 11 frames: the anchor that bites is the note rows, which with
    these parameters are the one-shot rows) and, without a bend ring, writes the same note rows and bitmap."""
    note, bits, bend = rings(3 + 284)
    note[:], bits[:], bend[:] = -7.0, 7, 99
    with tiny.open_stream(22050) as s:
        s.keep_rolling(prm, 3)
        s.push(x[:1])
        assert s.candidates_rolling(note, bits, bend, 0) == (0, 0, 0) and s.rows == 0
        assert (note == -7.0).all() and (bits == 7).all() and (bend == 99).all()
        at = 1
        for n, windows in ((HOP - LEAD, 1), (HOP - LEAD + 1, 2)):
            s.push(x[at:n])
            at, T = n, int(n / HOP * 142)
            assert s.rows == 0 and (n + LEAD + HOP - 1) // HOP == windows and T == 126
            a, T2, status, got = rolling_events(s, note, bits, bend, 0, prm)
            assert (a, T2, status) == (T - 3, T, 0), n
            maps = tiny.predict_pcm_raw(x[:n], nat.BP_PCM_F32, n, 1, 22050)
            assert maps["note"].shape[0] == T and got == slice_events(maps, a, T), n
            assert np.array_equal(unwrap(note, a, T).view(np.uint32), maps["note"][a:T].view(np.uint32)), n
            bare = rings(3 + 284)
            assert s.candidates_rolling(bare[0], bare[1], None, 0) == (a, T, 0)  # a null bend ring: the bends are skipped
            assert same_bytes([unwrap(r, a, T) for r in bare[:2]], [unwrap(r, a, T) for r in (note, bits)]), n
            assert (bend[a:T] != 99).all()  # the call with a bend ring wrote its bends (-25 ... 25)


def test_a_keeping_stream_alone_on_a_handle_of_one_window(tiny, nat, x, prm):
    """max_rows = 142 (426 slots).  40,004 = WIN - LEAD samples complete window 0: one window final, a tail of one window,
    T = int(40,004 / 36,164 * 142) = 157; at 72,000 samples the tail is two windows and T = 282 (window 1 completes at 76,168
    samples, which max_rows = 142 would refuse).  Each update is the host decoder's answer on the one-shot maps.  A second
    stream is finished at 36,164 samples, the 142 rows max_rows allows (two windows, none complete before the finish): there
    with_tail changes nothing, and with every final row held the note and bend arrays come back as they went in while the
    bitmap of the whole slice is written."""
    from basic_pitch_amd import note_creation as nc

    def update(s, n, held=0, **kw):
        """-> (T, the three arrays, the events as slice_events gives them without the frames)"""
        out = rings(142 + 284)
        T, status = s.candidates(out[0], out[1], out[2], held, **kw)
        assert status == 0 and T == int(n / HOP * 142), n
        return T, out, as_tuples(nc.decode_candidates(out[0][:T], out[1][:T], out[2][:T], prm))

    with tiny.open_stream(22050) as s:
        s.keep(prm, 142)
        at = 0
        for n, tail_windows, T_want in ((WIN - LEAD, 1, 157), (72_000, 2, 282)):
            s.push(x[at:n])
            at = n
            assert s.rows == 142 and (n + LEAD + HOP - 1) // HOP - 1 == tail_windows
            T, out, got = update(s, n)
            maps = tiny.predict_pcm_raw(x[:n], nat.BP_PCM_F32, n, 1, 22050)
            ref = slice_events(maps, 0, T)
            print(f"{n} samples: {T} rows, {len(got)} events, {len(ref)} in the reference")
            assert T == T_want == maps["note"].shape[0] and got == [r[2:] for r in ref], n
            assert np.array_equal(out[0][:T].view(np.uint32), maps["note"].view(np.uint32)), n
            bare = rings(142 + 284)
            assert s.candidates(bare[0], bare[1], None, 0) == (T, 0)  # a null bend ring: the bends are skipped
            assert same_bytes(bare[:2], out[:2]) and not bare[2].any() and out[2][:T].any(), n
        assert len(ref) >= 1
    with tiny.open_stream(22050) as s:
        s.keep(prm, 142)
        s.push(x[:HOP])
        assert s.rows == 0 and s.finish()["note"].shape[0] == 142 == s.rows
        T, out, got = update(s, HOP)
        maps = tiny.predict_pcm_raw(x[:HOP], nat.BP_PCM_F32, HOP, 1, 22050)
        assert T == 142 and got == [r[2:] for r in slice_events(maps, 0, T)]
        T2, final_only, _ = update(s, HOP, with_tail=False)
        assert T2 == T and same_bytes(final_only, out)
        held = rings(142 + 284)
        held[0][:], held[2][:] = -7.0, 99
        assert s.candidates(held[0], held[1], held[2], s.rows) == (T, 0)
        assert (held[0] == -7.0).all() and (held[2] == 99).all() and same_bytes(held[1:2], out[1:2])


# ---- 4. bounded ------------------------------------------------------------------------------------------------------------------
def test_the_state_of_a_rolling_stream_does_not_grow(model, x, prm):
    """bp_stream_state_bytes = 4 * (ring + 2 * hist) + cap * 1760 + 16 * ((cap + 63) / 64 + 3) (include/basic_pitch_amd_rolling.h)
    from the call on; and a horizon of 3 rows under pushes of several windows: far more rows than H, never refused."""
    with model.open_stream(22050) as s:
        plain = s.state_bytes()
        s.keep_rolling(prm, H)
        want = plain + CAP * 1760 + 16 * ((CAP + 63) // 64 + 3)
        assert s.state_bytes() == want
        at, sizes = 0, []
        for k in CHUNKS:
            s.push(x[at : at + k])
            at += k
            sizes.append((s.rows // 142, s.state_bytes()))
        assert {b for _, b in sizes} == {want} and sizes[-1][0] >= 8 and any(w == 3 for w, _ in sizes)
    note, bits, bend = rings(3 + 284)
    with model.open_stream(22050) as s:
        s.keep_rolling(prm, 3)
        for a in range(0, N, 100_000):  # three windows a push: more rows than the ring has slots
            s.push(x[a : a + 100_000])
            first, T, status = s.candidates_rolling(note, bits, bend, 0)
            assert first == T - 3 and status == 0
        assert s.rows == 8 * 142 and s.state_bytes() == plain + 287 * 1760 + 16 * (5 + 3)


# ---- 5. a second ingest format ---------------------------------------------------------------------------------------------------
def test_a_resampled_stereo_int16_stream_keeps_the_contract(model, nat, x, prm):
    """The melody as 44.1 kHz stereo int16 (each sample twice, the right channel at half the level): three updates."""
    up = np.repeat(x[:150_000], 2)
    pcm = np.stack([np.round(up * 24000), np.round(up * 12000)], axis=1).astype(np.int16)
    note, bits, bend = rings()
    with model.open_stream(44100, 2, nat.BP_PCM_S16) as s:
        s.keep_rolling(prm, H)
        at, held, with_a = 0, 0, 0
        for k in (100_001, 99_999, 100_000):
            s.push(pcm[at : at + k])
            at += k
            a, T, status, got = rolling_events(s, note, bits, bend, held, prm)
            held = s.rows
            maps = model.predict_pcm_raw(pcm[:at], nat.BP_PCM_S16, at, 2, 44100)
            assert T == maps["note"].shape[0] and status == 0
            assert got == slice_events(maps, a, T) and len(got) >= 3, at
            with_a += a > 0
        assert with_a >= 2


# ---- 6. the fallback ---------------------------------------------------------------------------------------------------------------
def test_status_1_decodes_the_slice_of_rolling_maps_on_the_host(model, nat, x):
    from basic_pitch_amd.streaming import StreamingTranscriber

    with StreamingTranscriber(model, 22050, onset_threshold=0.0, live=True, horizon_seconds=3.48) as t:
        t.push(x[:120_000])
        note, bits, bend = rings()
        a, T, status = t.stream.candidates_rolling(note, bits, bend, 0)
        assert (a, T, status) == (int(120_000 / HOP * 142) - H, int(120_000 / HOP * 142), 1)
        _, events = t.transcript()
        a2, kept = t.stream.rolling_maps()
        ref_maps = model.predict_pcm_raw(x[:120_000], nat.BP_PCM_F32, 120_000, 1, 22050)
        assert a2 == a and all(np.array_equal(kept[m].view(np.uint32), ref_maps[m][a:T].view(np.uint32)) for m in MAPS)
        ref = slice_events(kept, 0, T - a, onset_threshold=0.0)  # slice frames; the times below are those of frames + a
        assert len(events) == len(ref) > 0
        assert as_tuples(events) == [r[2:] for r in slice_events(ref_maps, a, T, onset_threshold=0.0)]
        assert t._rows == []


def test_a_nan_leaves_the_horizon_with_its_row(tmp_path):
    """The A/B library's hook makes onset cell (row 200, bin 40) of the kept copy a NaN whenever the row is written
    (tools/experiments/stream_rolling_nan_ab.py, one process with that library; a NaN is a value, nothing faults).  H = 300:
    row 200 in the tail; among the final rows, in a block the update joins from the table; and outside the horizon, twice."""
    import json
    import subprocess
    import sys

    from basic_pitch_amd import build

    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "stream_rolling_nan_ab.py")
    out = str(tmp_path / "nan.json")
    env = dict(os.environ, BASIC_PITCH_AMD_LIB=build.build_library(ab=True))
    subprocess.run([sys.executable, tool, out], check=True, timeout=300, env=env)
    got = json.load(open(out))
    ups = got["updates"]
    assert [u["status"] for u in ups] == [1, 1, 0, 0]
    assert ups[0]["final_rows"] <= got["row"] < ups[0]["rows"] and ups[0]["first_row"] == 0          # in the tail
    assert ups[1]["first_row"] + 2 <= 192 and 256 <= ups[1]["final_rows"]                            # block 3 whole, from the table
    assert got["row"] < ups[2]["first_row"] < ups[3]["first_row"]                                    # left with its row
    for u in ups:
        assert len(u["transcript"]) >= 1 and u["transcript"] == u["expected"], u["frames"]  # CPU restatement: 3, 5, 8, 10 events
        assert u["maps_equal_but_for_the_cell"] is (u["status"] == 1)


# ---- 7. refusals, with nothing changed -----------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_as_it_was(model, nat, x, prm):
    lib = model._lib
    err = lambda: lib.bp_last_error(model._handle)  # noqa: E731
    with model.open_stream(22050) as s:
        before = s.state_bytes()
        for bad in (2, 0, -5):
            assert lib.bp_stream_keep_rolling(s._s, C.addressof(prm), bad) == nat.BP_ERR_INVALID_ARG and b"horizon_rows" in err()
        assert s.state_bytes() == before
        s.keep_rolling(prm, H)
        with pytest.raises(ValueError, match="bp_stream_keep_rolling"):
            s.keep(prm, 1000)  # keep after keep_rolling
        with pytest.raises(ValueError, match="already"):
            s.keep_rolling(prm, H)
        first = s.push(x[:50_000])
        note, bits, bend = rings()
        small = rings(CAP - 1)
        note[:], small[0][:] = -7.0, -7.0
        f, T, st = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
        rc = lib.bp_stream_candidates_rolling(s._s, 1, small[0].ctypes.data, small[1].ctypes.data, small[2].ctypes.data, CAP - 1, 0,
                                              C.byref(f), C.byref(T), C.addressof(st))
        assert rc == nat.BP_ERR_INVALID_ARG and b"ring_rows" in err() and (small[0] == -7.0).all() and T.value == -1
        with pytest.raises(ValueError, match="held_rows"):
            s.candidates_rolling(note, bits, bend, s.rows + 1)
        assert (note == -7.0).all()
        with pytest.raises(ValueError, match="does not keep its maps"):
            s.candidates(note, bits, bend, 0)  # the plain call on a rolling stream
        a, T1, status = s.candidates_rolling(note, bits, bend, 0)
        assert (a, T1, status) == (0, int(50_000 / HOP * 142), 0)
        rest = s.push(x[50_000:120_000])
        ref = model.predict_pcm_raw(x[:120_000], nat.BP_PCM_F32, 120_000, 1, 22050)
        got = np.concatenate([first["note"], rest["note"], s.peek()["note"]])
        assert np.array_equal(got.view(np.uint32), ref["note"].view(np.uint32))
    with model.open_stream(22050) as s:
        s.keep(prm, 2000)
        with pytest.raises(ValueError, match="bp_stream_keep"):
            s.keep_rolling(prm, H)  # keep_rolling after keep
        with pytest.raises(ValueError, match="rolling horizon"):
            s.candidates_rolling(*rings(), 0)
    with model.open_stream(22050) as s:
        s.push(x[:50_000])
        with pytest.raises(ValueError, match="rows have left"):
            s.keep_rolling(prm, H)  # after the first row has left
        assert s.state_bytes() == before
