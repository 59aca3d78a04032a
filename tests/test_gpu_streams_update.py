"""The live transcripts of many streams in one step (bp_streams_update_layout / bp_streams_candidates,
include/basic_pitch_amd_update.h; streaming.transcripts): for every stream of the call the out fields, the new note and bend
rows and the bitmap of the slice are byte for byte what the single-stream update — bp_stream_candidates for a keeping stream,
bp_stream_candidates_rolling for a rolling one — writes with the same held_rows, for any set, order and mixture of streams,
and nothing is committed.  An update changes no counter, so the same streams serve both sides of every comparison: the
many-stream call first, the single calls after it.  The single update is the many-stream step with one stream, so the
comparison holds a step to its own n = 1 case; what holds both to the decoder is the host anchor of the first test: the
events of every update are the host decoder's on the same rows of the one-shot maps.  Every test does ordinary work; refusals
are argument errors.

Not provoked here, because no legitimate input reaches them: a broken stream (it takes a failed device call) and a tail that
does not fit the ring (tail_refused's verdict, which no supported rate produces); both are the single calls' own checks."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOP, LEAD = 36164, 3840
N = 307_000


def melody(n=N, seed=11):
    """The signal of tests/test_gpu_stream_rolling.py, restated: overlapping harmonic tones (three partials, 110 ... 880 Hz,
    0.2 ... 1.5 s, each starting before the last has ended) over 1e-3 noise."""
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


# The seven streams: (mode, horizon or max_rows, rate, parameters, input frames pushed by the end of each round, finished after
# round 0).  A stream of n model-rate samples, n = k * HOP + r, has run k windows and has a tail of one window when
# r <= HOP - LEAD = 32,324 and of two above: round 2 gives all five growing streams a tail of two (r = 34,000, 33,000, 33,500,
# 34,567, 33,000), ten windows on a handle of eight — the peek step runs two rounds.
SPECS = (
    ("roll", 150, 22050, "a", (50_001, 120_000, 142_492, N), False),       # 434 slots, 559 rows by round 2: wrapped
    ("roll", 300, 22050, "a", (10_000, 30_000, 69_164, 75_000), False),    # 294 rows at most: below its horizon
    ("roll", 3, 22050, "b", (107_328, 150_000, 178_156, 250_000), False),  # other parameters: a threshold, frequency limits
    ("keep", 1500, 22050, "c", (1, 47_000, 70_731, 200_000), False),       # no bends, no inferred onsets; no row in round 0
    ("keep", 1500, 44100, "a", (60_001, 150_000, 210_656, 290_000), False),  # 44.1 kHz stereo int16
    ("roll", 300, 22050, "a", (0, 0, 0, 0), False),                        # never fed: T == 0
    ("roll", 200, 22050, "a", (100_000,) * 4, True),                       # finished in round 0: 392 rows, a = 192, no tail
)


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


# the three parameter sets, as note_creation._note_params and note_creation._decode take them
PRM_ARGS = {"a": (0.5, 0.3, 11, True, None, None, True, 11, True),
            "b": (0.4, 0.3, 11, True, 2000.0, 100.0, True, 11, True),
            "c": (0.5, 0.3, 11, False, None, None, True, 11, False)}


@pytest.fixture(scope="module")
def prms():
    from basic_pitch_amd import note_creation as nc

    return {k: nc._note_params(*v) for k, v in PRM_ARGS.items()}


def slice_events(maps, a, T, args):
    """slice_events of tests/test_gpu_stream_rolling.py for any parameter set: bp_notes_decode on copies of rows [a, T) of the
    one-shot maps as a whole track, frames shifted by a, times of the absolute frames, in the form of as_tuples (no bends:
    None)."""
    from basic_pitch_amd import note_creation as nc

    sl = [np.ascontiguousarray(maps[m][a:T]).copy() for m in ("note", "onset", "contour")]
    ev, bends, n = nc._decode(*sl, *args)
    times = nc.model_frames_to_time(T + 1)
    return [(times[e.start_frame + a].tobytes(), times[e.end_frame + a].tobytes(), int(e.pitch_midi),
             np.float32(e.amplitude).tobytes(), bends[e.bend_offset : e.bend_offset + e.n_bends].tolist() if args[-1] else None)
            for e in ev[:n]]


class Sess:
    """A stream of SPECS with two sets of host rings: `mine`, filled from the packed rows of the many-stream call, and `ref`,
    filled by the single call; both with the held-rows bookkeeping of a transcriber."""

    def __init__(self, model, nat, spec, prms, x):
        mode, rows, rate, key, self.totals, self.finishes = spec
        self.rolling, self.prm, self.key, self.rate = mode == "roll", prms[key], key, rate
        if rate == 44100:
            up = np.repeat(x[:150_000], 2)
            self.pcm = np.stack([np.round(up * 24000), np.round(up * 12000)], axis=1).astype(np.int16)
            self.fmt, self.channels = nat.BP_PCM_S16, 2
        else:
            self.pcm = x
            self.fmt, self.channels = nat.BP_PCM_F32, 1
        self.s = model.open_stream(rate, self.channels, self.fmt)
        if self.rolling:
            self.s.keep_rolling(self.prm, rows)
            self.ring_rows = rows + 284
        else:
            self.s.keep(self.prm, rows)
            self.ring_rows = rows + 284
        self.at, self.held, self.done = 0, 0, False
        self.mine, self.ref = self.rings(), self.rings()

    def rings(self):
        return (np.zeros((self.ring_rows, 88), np.float32), np.zeros((self.ring_rows, 12), np.uint8),
                np.zeros((self.ring_rows, 88), np.int8))

    def feed(self, rnd):
        """Irregular chunks up to the round's total; returns the rows the pushes (and the finish) emitted."""
        out, delta = [], self.totals[rnd] - self.at
        for k in (1, delta // 3, delta - 1 - delta // 3) if delta > 2 else ((delta,) if delta else ()):
            out.append(self.s.push(self.pcm[self.at : self.at + k]))
            self.at += k
        if self.finishes and not self.done:
            out.append(self.s.finish())
            self.done = True
        return out

    def tail_windows(self):
        n = (self.at * 22050 + self.rate - 1) // self.rate
        return 0 if self.done or n == 0 else (n + LEAD + HOP - 1) // HOP - self.s.rows // 142

    def single(self, held, rings=None):
        """The single-stream update into `rings` (note, bits, bend): (a, T, status)."""
        note, bits, bend = rings or self.ref
        if self.rolling:
            return self.s.candidates_rolling(note, bits, bend, held)
        T, status = self.s.candidates(note, bits, bend, held)
        return 0, T, status

    def one_shot(self, model):
        """The one-shot maps of the audio fed so far, in the stream's own format, channels and rate."""
        return model.predict_pcm_raw(self.pcm[: self.at], self.fmt, self.at, self.channels, self.rate)

    def close(self):
        self.s.close()


def open_set(model, nat, prms, x, rounds, specs=SPECS):
    ss = [Sess(model, nat, spec, prms, x) for spec in specs]
    for rnd in range(rounds):
        for s in ss:
            s.feed(rnd)
    return ss


def unwrap(ring, a, T):
    return np.ascontiguousarray(ring[np.arange(a, T) % ring.shape[0]])


def many(model, ss, helds, with_tail=True):
    from basic_pitch_amd import streaming

    return streaming.streams_candidates(model, [s.s for s in ss], helds, with_tail)


def per_stream(ss, tab, note, bend, bits):
    """What the contract covers, per stream: (a, T, n0, status, note bytes, bend bytes or None, bitmap bytes)."""
    out = []
    for s, u in zip(ss, tab):
        k, b = u.n_rows - u.new_row, u.n_rows - u.first_row
        out.append((u.first_row, u.n_rows, u.new_row, u.status, note[u.note_offset : u.note_offset + k].tobytes(),
                    bend[u.note_offset : u.note_offset + k].tobytes() if s.prm.include_pitch_bends else None,
                    bits[u.bits_offset : u.bits_offset + b].tobytes()))
    return out


def singles(ss, helds):
    """The same tuples from the single calls into fresh rings."""
    out = []
    for s, held in zip(ss, helds):
        note, bits, bend = fresh = s.rings()
        a, T, status = s.single(held, fresh)
        n0 = max(held, a)
        out.append((a, T, n0, status, unwrap(note, n0, T).tobytes(),
                    unwrap(bend, n0, T).tobytes() if s.prm.include_pitch_bends else None, unwrap(bits, a, T).tobytes()))
    return out


def as_tuples(events):
    return [(np.float64(e[0]).tobytes(), np.float64(e[1]).tobytes(), int(e[2]), np.float32(e[3]).tobytes(),
             None if e[4] is None else list(e[4])) for e in events]


@pytest.fixture(scope="module")
def aged(model, nat, prms, x):
    """The seven streams after round 2 (every growing stream with a tail of two windows), for the tests that only update."""
    ss = open_set(model, nat, prms, x, 3)
    yield ss
    for s in ss:
        s.close()


# ---- 1. the contract -----------------------------------------------------------------------------------------------------------
def test_every_stream_gets_the_bytes_of_its_single_update(model, nat, prms, x):
    from basic_pitch_amd import note_creation as nc
    from basic_pitch_amd import streaming

    ss = open_set(model, nat, prms, x, 0)
    tails, n_events, wrapped, anchors = [], 0, False, {}
    try:
        for rnd in range(4):
            for s in ss:
                s.feed(rnd)
            tails.append([s.tail_windows() for s in ss])
            helds = [s.held for s in ss]
            tab, note, bend, bits = many(model, ss, helds)
            got = per_stream(ss, tab, note, bend, bits)
            for i, (s, u) in enumerate(zip(ss, tab)):
                a, T, status = s.single(s.held)
                n0 = max(s.held, a)
                print(f"round {rnd} stream {i}: rows [{a}, {T}) new from {n0}, tail {T - s.s.rows}, status {status}")
                assert (u.first_row, u.n_rows, u.new_row, u.status) == (a, T, n0, status) and status == 0, (rnd, i)
                rn, rb, rd = s.ref
                want = (a, T, n0, status, unwrap(rn, n0, T).tobytes(),
                        unwrap(rd, n0, T).tobytes() if s.prm.include_pitch_bends else None, unwrap(rb, a, T).tobytes())
                assert got[i] == want, (rnd, i)
                mn, mb, md = s.mine
                streaming.scatter_rows(mn, note[u.note_offset : u.note_offset + T - n0], n0, T)
                streaming.scatter_rows(md, bend[u.note_offset : u.note_offset + T - n0], n0, T)
                streaming.scatter_rows(mb, bits[u.bits_offset : u.bits_offset + T - a], a, T)
                s.held = s.s.rows
                wrapped = wrapped or (i == 0 and T > s.ring_rows)
                if T == 0:
                    continue
                bends = s.prm.include_pitch_bends
                ev = [nc.decode_candidates(unwrap(r[0], a, T), unwrap(r[1], a, T), unwrap(r[2], a, T) if bends else None, s.prm,
                                           first_frame=a) for r in (s.mine, s.ref)]
                assert as_tuples(ev[0]) == as_tuples(ev[1]), (rnd, i)
                # the host anchor: the host decoder on rows [a, T) of the one-shot maps of the audio fed so far
                if (i, s.at) not in anchors:
                    maps = s.one_shot(model)
                    assert maps["note"].shape[0] == T, (rnd, i)
                    anchors[i, s.at] = slice_events(maps, a, T, PRM_ARGS[s.key])
                print(f"round {rnd} stream {i}: {len(ev[0])} events, {len(anchors[i, s.at])} in the host reference")
                assert as_tuples(ev[0]) == anchors[i, s.at], (rnd, i)
                n_events += len(ev[1])
            assert (tab[5].n_rows, tab[5].note_offset, tab[5].bits_offset) == (0, tab[6].note_offset, tab[6].bits_offset)
            assert tab[6].first_row == 192 and tab[6].n_rows == 392
    finally:
        for s in ss:
            s.close()
    flat = [t for row in tails for t in row]
    assert 1 in flat and 2 in flat and tails[2][:5] == [2] * 5 and sum(tails[2]) > 8, tails
    assert wrapped and n_events > 40, (wrapped, n_events)


# ---- 2. order and grouping -----------------------------------------------------------------------------------------------------
def test_any_order_and_grouping_gives_the_same_bytes_per_stream(model, aged):
    helds = [s.s.rows // 2 for s in aged]
    base = per_stream(aged, *many(model, aged, helds))
    rev = per_stream(aged[::-1], *many(model, aged[::-1], helds[::-1]))
    assert rev[::-1] == base
    two = per_stream(aged[:3], *many(model, aged[:3], helds[:3])) + per_stream(aged[3:], *many(model, aged[3:], helds[3:]))
    assert two == base
    assert base == singles(aged, helds)
    assert sum(len(b[4]) for b in base) > 0


# ---- 3. held_rows ----------------------------------------------------------------------------------------------------------------
def test_the_rows_sent_start_at_the_held_rows_or_at_the_slice(model, aged):
    from basic_pitch_amd import streaming

    lib = streaming.bind(model._lib)
    a0 = max(0, aged[0].s.rows - 150)
    assert a0 > 5
    for name, helds in (("none held", [0] * 7), ("all final rows held", [s.s.rows for s in aged]),
                        ("below the slice", [a0 - 5] + [min(1, s.s.rows) for s in aged[1:]])):
        tab, note, bend, bits = many(model, aged, helds)
        note_at = bits_at = 0
        for s, u, held in zip(aged, tab, helds):
            assert u.new_row == max(held, u.first_row) and (u.note_offset, u.bits_offset) == (note_at, bits_at), name
            note_at, bits_at = note_at + u.n_rows - u.new_row, bits_at + u.n_rows - u.first_row
        assert (note.shape[0], bits.shape[0]) == (note_at, bits_at)
        lay = streaming.update_table([s.s for s in aged], helds)
        nr, br = C.c_int64(-1), C.c_int64(-1)
        assert lib.bp_streams_update_layout(model._handle, 7, C.addressof(lay), 1, C.byref(nr), C.byref(br)) == 0
        assert (nr.value, br.value) == (note_at, bits_at)
        fields = lambda t: [(u.first_row, u.n_rows, u.new_row, u.note_offset, u.bits_offset) for u in t[:7]]  # noqa: E731
        assert fields(lay) == fields(tab)
        assert per_stream(aged, tab, note, bend, bits) == singles(aged, helds), name
    # without the tail: the final rows only
    tab, note, bend, bits = many(model, aged, [0] * 7, with_tail=False)
    assert [u.n_rows for u in tab[:7]] == [s.s.rows for s in aged]
    for s, got in zip(aged, per_stream(aged, tab, note, bend, bits)):
        fresh = s.rings()
        if s.rolling:
            a, T, st = s.s.candidates_rolling(fresh[0], fresh[1], fresh[2], 0, with_tail=False)
        else:
            (T, st), a = s.s.candidates(fresh[0], fresh[1], fresh[2], 0, with_tail=False), 0
        assert got[:4] == (a, T, a, st) and got[4] == unwrap(fresh[0], a, T).tobytes() and got[6] == unwrap(fresh[1], a, T).tobytes()
    # no stream at all
    assert lib.bp_streams_candidates(model._handle, 0, None, 1, None, None, None, 0, 0) == 0


# ---- 4. nothing committed --------------------------------------------------------------------------------------------------------
def test_an_update_commits_nothing(model, nat, prms, x):
    specs = SPECS[:5]  # the growing streams
    A, B = open_set(model, nat, prms, x, 2, specs), open_set(model, nat, prms, x, 2, specs)
    same = lambda p, q: all(p[m].shape == q[m].shape and np.array_equal(p[m].view(np.uint32), q[m].view(np.uint32))  # noqa: E731
                            for m in ("note", "onset", "contour"))
    try:
        many(model, A, [0] * 5)
        many(model, A[::-1], [s.s.rows for s in A[::-1]])
        rows = 0
        for a, b in zip(A, B):
            assert same(a.s.peek(), b.s.peek())
        many(model, A, [0] * 5)
        for a, b in zip(A, B):
            for p, q in zip(a.feed(2), b.feed(2)):
                assert same(p, q)
                rows += p["note"].shape[0]
        many(model, A, [0] * 5)
        assert singles(A, [0] * 5) == singles(B, [0] * 5)
        for a, b in zip(A, B):
            p, q = a.s.finish(), b.s.finish()
            assert same(p, q) and p["note"].shape[0] > 0
        assert per_stream(A, *many(model, A, [0] * 5)) == singles(B, [0] * 5)  # finished streams: no tail
        assert rows > 0
    finally:
        for s in A + B:
            s.close()


# ---- 5. Python -----------------------------------------------------------------------------------------------------------------------
def test_transcripts_equals_every_transcribers_own_transcript(model, x):
    """Twins: one list through streaming.transcripts, one through transcript().  horizon_seconds=2.0 is 173 rows in host rings
    of 457: 1,205 rows wrap them twice; onset_threshold=0 is status 1 in both modes."""
    from basic_pitch_amd.streaming import StreamingTranscriber as ST

    def make():
        return [ST(model, 22050, live=True, horizon_seconds=2.0), ST(model, 22050, live=True, max_rows=1500),
                ST(model, 22050, live=True, horizon_seconds=3.48, onset_threshold=0.0),
                ST(model, 22050, live=True, max_rows=1500, onset_threshold=0.0, minimum_frequency=100.0)]

    A, B = make(), make()
    try:
        at, n_events = 0, 0
        for k in (50_001, 90_000, 100_000, 66_999):
            for t in A + B:
                t.push(x[at : at + k])
            at += k
            got, ref = model.transcripts(A), [t.transcript() for t in B]
            for i, ((m1, e1), (m2, e2)) in enumerate(zip(got, ref)):
                assert as_tuples(e1) == as_tuples(e2), (at, i)
                assert [len(j.notes) for j in m1.instruments] == [len(j.notes) for j in m2.instruments], (at, i)
                n_events += len(e2)
            for a, b in zip(A[:2], B[:2]):
                assert a._held == b._held == a.stream.rows and a._note.shape == b._note.shape
            T = A[0].stream.rows + A[0].stream.rows_bound(0)
            for name in ("_note", "_bits", "_bend"):
                assert unwrap(getattr(A[0], name), T - 173, T).tobytes() == unwrap(getattr(B[0], name), T - 173, T).tobytes(), name
        assert at == N and T > 2 * 457 and n_events > 40
    finally:
        for t in A + B:
            t.close()


# ---- 6. NaN isolation, 8. memory: one process with the A/B library ----------------------------------------------------------
@pytest.fixture(scope="module")
def ab_run(tmp_path_factory):
    from basic_pitch_amd import build

    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "streams_update_nan_ab.py")
    out = str(tmp_path_factory.mktemp("update") / "nan.json")
    env = dict(os.environ, BASIC_PITCH_AMD_LIB=build.build_library(ab=True))
    subprocess.run([sys.executable, tool, out], check=True, timeout=300, env=env)
    return json.load(open(out))


def test_a_nan_in_one_stream_changes_no_other_stream(ab_run):
    """The A/B library's hook makes onset cell (row 200, bin 40) of the middle stream's kept copy a NaN whenever the row is
    written (tools/experiments/streams_update_nan_ab.py; a NaN is a value, nothing faults): in the tail at the first update,
    among the final rows at the second."""
    for up in ab_run["updates"]:
        assert up["status"] == [0, 1, 0] and up["single_status"] == [0, 1, 0], up
        assert up["fields_equal"] == [True] * 3 and up["note_equal"] == [True] * 3, up
        assert up["bytes_equal"][0] and up["bytes_equal"][2], up
        assert up["rows"][1][0] <= 200 < up["rows"][1][1]
    assert ab_run["updates"][0]["final_rows"][1] <= 200 < ab_run["updates"][1]["final_rows"][1]


def test_updates_grow_neither_the_streams_nor_the_handle(model, aged, ab_run):
    before = [s.s.state_bytes() for s in aged]
    for _ in range(3):
        many(model, aged, [0] * 7)
    assert [s.s.state_bytes() for s in aged] == before
    live = ab_run["live_device_bytes"]  # the A/B library's count after each of 20 updates of one set
    assert len(live) == 20 and len(set(live)) == 1 and live[0] > 0, live
    assert len(set(map(tuple, ab_run["state_bytes"]))) == 1


# ---- 7. refusals, with nothing changed -----------------------------------------------------------------------------------------
def test_refusals_name_the_stream_and_leave_every_stream_as_it_was(model, nat, prms, aged):
    from basic_pitch_amd import streaming
    from basic_pitch_amd.inference import Model

    lib = streaming.bind(model._lib)
    helds = [0] * 7
    before = singles(aged, helds)
    tab, note, bend, bits = many(model, aged, helds)
    note[:], bits[:] = -7.0, 7

    def call(streams, held, note_cap=None, bits_cap=None, note_ptr=True, bits_ptr=True):
        t = (nat.bp_stream_update * len(streams))()
        for i, (s, k) in enumerate(zip(streams, held)):
            t[i].stream, t[i].held_rows = s, k
        rc = lib.bp_streams_candidates(model._handle, len(streams), C.addressof(t), 1, note.ctypes.data if note_ptr else None,
                                       bend.ctypes.data, bits.ctypes.data if bits_ptr else None,
                                       note.shape[0] if note_cap is None else note_cap, bits.shape[0] if bits_cap is None else bits_cap)
        nr, br = C.c_int64(0), C.c_int64(0)
        rc2 = lib.bp_streams_update_layout(model._handle, len(streams), C.addressof(t), 1, C.byref(nr), C.byref(br))
        return rc, rc2, lib.bp_last_error(model._handle)

    ptrs = [s.s._s.value for s in aged]
    with Model(max_windows=1) as other, other.open_stream(22050) as foreign, model.open_stream(22050) as plain:
        foreign.keep_rolling(prms["a"], 100)
        for streams, held, word in (
            (ptrs[:2] + [None], helds[:3], b"stream 2: null stream"),
            (ptrs[:1] + [foreign._s.value], helds[:2], b"stream 1: a stream of another handle"),
            (ptrs[:4] + ptrs[1:2], helds[:5], b"stream 4: the same stream twice"),
            ([plain._s.value] + ptrs[:1], helds[:2], b"stream 0: the stream retains nothing"),
            (ptrs[:3], [0, -1, 0], b"stream 1: held_rows -1"),
            (ptrs[:3], [0, 0, aged[2].s.rows + 1], b"stream 2: held_rows"),
        ):
            rc, rc2, err = call(streams, held)
            assert rc == rc2 == nat.BP_ERR_INVALID_ARG and word in err, (word, err)
    for kw, word in (({"note_cap": note.shape[0] - 1}, b"too small"), ({"bits_cap": bits.shape[0] - 1}, b"too small"),
                     ({"note_ptr": False}, b"null output"), ({"bits_ptr": False}, b"null output")):
        rc, rc2, err = call(ptrs, helds, **kw)
        assert rc == nat.BP_ERR_INVALID_ARG and rc2 == 0 and word in err, (kw, err)
    with streaming.StreamingTranscriber(model, 22050) as not_live, pytest.raises(ValueError, match="live=True"):
        streaming.transcripts(model, [not_live])
    assert (note == -7.0).all() and (bits == 7).all()
    assert singles(aged, helds) == before
    assert per_stream(aged, *many(model, aged, helds)) == before
