"""Note events of many live streams straight from the device (bp_streams_events_layout / bp_streams_events,
include/basic_pitch_amd_stream_events.h; streaming.transcripts(decode="device")): for every stream of a call with status 0 the
out fields, the events and their bends are byte for byte what the single route gives — the single update of that stream with
held_rows = 0 (bp_stream_candidates, bp_stream_candidates_rolling), then bp_notes_decode_candidates_at with first_frame =
first_row and the stream's own parameters — for any set, order and mixture of streams, and nothing is committed.  Every
comparison is of bytes: frames, pitch, the float32 amplitude's bit pattern, the times as float64, bend lists, event order.

The tracker's forms (LDS, scratch) with per-segment parameters on hand-made maps and the NaN hook need the A/B library: one child process
(tools/experiments/streams_events_ab.py) runs them and saves what it compared."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_streams_update import Sess, melody, open_set, per_stream, unwrap

pytestmark = pytest.mark.gpu

N = 307_000
# (mode, horizon or max_rows, rate, parameters, input frames pushed by the end of each round, finished after round 0)
SPECS = (
    ("roll", 500, 22050, "a", (100_001, 200_000, 250_000, N), False),      # 784 slots, 1,136 rows by round 3: wrapped, slice 500 + tail
    ("roll", 150, 22050, "a", (50_001, 120_000, 142_492, N), False),       # a slice under 432 rows
    ("roll", 3, 22050, "b", (107_328, 150_000, 178_156, 250_000), False),  # a horizon of 3 rows; a threshold, frequency limits
    ("keep", 1500, 22050, "c", (1, 47_000, 70_731, 200_000), False),       # no bends, no inferred onsets; no row in round 0
    ("keep", 1500, 44100, "a", (60_001, 150_000, 210_656, 290_000), False),  # 44.1 kHz stereo int16
    ("roll", 300, 22050, "a", (0, 0, 0, 0), False),                        # never fed: T == 0
    ("roll", 200, 22050, "a", (100_000,) * 4, True),                       # finished in round 0: 392 rows, a = 192, no tail
    ("roll", 600, 22050, "d", (80_000, 160_000, 240_000, N), False),       # melodia off
    ("keep", 1500, 22050, "d", (40_000, 130_000, 220_000, 300_000), False),
    ("roll", 450, 22050, "e", (90_000, 170_000, 260_000, N), False),       # min_note_len 0, other thresholds, frequency limits
    ("keep", 1500, 22050, "f", (70_000, 140_000, 230_000, N), False),      # min_note_len 5, a tolerance of 5, no bends
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


def note_params():
    from basic_pitch_amd import note_creation as nc

    return {"a": nc._note_params(0.5, 0.3, 11, True, None, None, True, 11, True),
            "b": nc._note_params(0.4, 0.3, 11, True, 2000.0, 100.0, True, 11, True),
            "c": nc._note_params(0.5, 0.3, 11, False, None, None, True, 11, False),
            "d": nc._note_params(0.5, 0.3, 11, True, None, None, False, 11, True),
            "e": nc._note_params(0.4, 0.25, 0, True, 1500.0, 80.0, True, 11, True),
            "f": nc._note_params(0.6, 0.35, 5, True, None, None, True, 5, False)}


@pytest.fixture(scope="module")
def prms():
    return note_params()


def records(events, bends, lo, hi, with_bends):
    """bp_note_event records lo ... hi - 1 as comparable tuples: frames, pitch, the amplitude's bits, times, bends."""
    return [(e.start_frame, e.end_frame, e.pitch_midi, np.float32(e.amplitude).tobytes(), np.float64(e.start_s).tobytes(),
             np.float64(e.end_s).tobytes(), e.n_bends, e.reserved,
             tuple(bends[e.bend_offset : e.bend_offset + e.n_bends].tolist()) if with_bends else None) for e in events[lo:hi]]


def single_route(model, s, with_tail=True):
    """The route of the contract for one Sess: its single update with held_rows = 0 into fresh rings, then
    bp_notes_decode_candidates_at: (first_row, n_rows, status, records or None)."""
    from basic_pitch_amd import note_creation as nc

    note, bits, bend = s.rings()
    if s.rolling:
        a, T, status = s.s.candidates_rolling(note, bits, bend, 0, with_tail=with_tail)
    else:
        (T, status), a = s.s.candidates(note, bits, bend, 0, with_tail=with_tail), 0
    if status or T == 0:
        return a, T, status, None if status else []
    pb = bool(s.prm.include_pitch_bends)
    ln, lb, ld = unwrap(note, a, T), unwrap(bits, a, T), unwrap(bend, a, T) if pb else None
    maps = (ln.ctypes.data, lb.ctypes.data, ld.ctypes.data if pb else None, T - a)
    events, bends, n = nc._grow_and_call(model._lib.bp_notes_decode_candidates_at, maps + (a, C.addressof(s.prm)), T - a,
                                         "bp_notes_decode_candidates_at")
    return a, T, status, records(events, bends, 0, n, pb)


def device_route(model, ss, with_tail=True, room=None):
    """One bp_streams_events call for the Sess list: [(first_row, n_rows, status, records)] per stream."""
    from basic_pitch_amd import streaming

    tab, events, bends, offs = streaming.streams_events(model, [s.s for s in ss], with_tail, room)
    assert offs[0] == 0 and (np.diff(offs) >= 0).all()
    all_ev = events[: int(offs[-1])]  # bend_offset runs through the bends of all streams in event order
    assert [e.bend_offset for e in all_ev] == np.concatenate([[0], np.cumsum([e.n_bends for e in all_ev])])[:-1].astype(int).tolist()
    out = []
    for i, s in enumerate(ss):
        u = tab[i]
        recs = records(events, bends, int(offs[i]), int(offs[i + 1]), bool(s.prm.include_pitch_bends))
        out.append((u.first_row, u.n_rows, u.status, recs if u.status == 0 else (None if not recs else "events beside a status")))
    return out


def many_bytes(model, ss):
    from basic_pitch_amd import streaming

    return per_stream(ss, *streaming.streams_candidates(model, [s.s for s in ss], [0] * len(ss)))


# ---- 1. the contract on a mixed set, over several rounds of pushes; nothing committed -----------------------------------------
def test_every_stream_gets_the_events_of_its_single_route_and_nothing_is_committed(model, nat, prms, x):
    from basic_pitch_amd import streaming

    A, B = open_set(model, nat, prms, x, 0, SPECS), open_set(model, nat, prms, x, 0, SPECS)  # B: twins that never see the call
    same = lambda p, q: all(p[m].shape == q[m].shape and np.array_equal(p[m].view(np.uint32), q[m].view(np.uint32))  # noqa: E731
                            for m in ("note", "onset", "contour"))
    n_events, long_slices, wrapped = 0, 0, False
    try:
        for rnd in range(4):
            for a, b in zip(A, B):
                for p, q in zip(a.feed(rnd), b.feed(rnd)):
                    assert same(p, q), rnd
            want = [single_route(model, s) for s in A]
            got = device_route(model, A)
            for i, (g, w) in enumerate(zip(got, want)):
                print(f"round {rnd} stream {i}: rows [{w[0]}, {w[1]}), status {w[2]}, {len(w[3])} events")
                assert w[2] == 0 and g == w, (rnd, i, g[:3], w[:3])
                n_events += len(w[3])
                long_slices += w[1] - w[0] > 432
            wrapped = wrapped or want[0][1] > A[0].ring_rows
            assert device_route(model, A[::-1])[::-1] == want, rnd  # any order
            sub = [0, 3, 4, 7, 9]
            assert device_route(model, [A[i] for i in sub]) == [want[i] for i in sub], rnd  # any subset
            # the layout: the same out fields and capacities that cover the call, from the counters alone
            lay, cap_e, cap_b = streaming.streams_events_layout(model, [s.s for s in A])
            assert [(u.first_row, u.n_rows) for u in lay[: len(A)]] == [w[:2] for w in want]
            mirror = streaming.streams_events_capacity([(w[1] - w[0], s.prm.min_note_len, bool(s.prm.include_pitch_bends))
                                                        for s, w in zip(A, want)])
            assert (cap_e, cap_b) == mirror
            assert device_route(model, A, room=(cap_e, cap_b)) == want
            assert [streaming.slice_first_row(s.s.rows, w[1] - s.s.rows, None if not s.rolling else s.ring_rows - 284)
                    for s, w in zip(A, want)] == [w[:2] for w in want]
            # without the tail: the final rows only
            assert device_route(model, A, with_tail=False) == [single_route(model, s, with_tail=False) for s in A], rnd
            # nothing committed: the many-stream update gives the twins' bytes
            assert many_bytes(model, A) == many_bytes(model, B), rnd
        assert wrapped and long_slices >= 4 and n_events > 100, (wrapped, long_slices, n_events)
        for a, b in zip(A, B):
            if not a.done:
                p, q = a.s.finish(), b.s.finish()
                assert same(p, q)
        assert many_bytes(model, A) == many_bytes(model, B)
        assert device_route(model, A) == [single_route(model, s) for s in B]  # finished streams: no tail
    finally:
        for s in A + B:
            s.close()


# ---- 2. slice lengths at the form and word boundaries ---------------------------------------------------------------------------
def test_slices_at_the_form_and_word_boundaries(model, nat, prms, x):
    from basic_pitch_amd import streaming

    lengths = (1, 2, 3, 63, 64, 65, 128, 129, 432, 433, 1000)
    specs = [("roll", 3, 22050, "a", (300,), True), ("roll", 3, 22050, "a", (600,), True)]
    specs += [("roll", h, 22050, "e" if h in (64, 433) else "a", (N,), True) for h in lengths[2:]]
    ss = [Sess(model, nat, spec, prms, x) for spec in specs]
    try:
        streaming.push_streams(model, [s.s for s in ss], [x[: s.totals[0]] for s in ss])
        for s in ss:
            s.s.finish()
            s.done = True
        want = [single_route(model, s) for s in ss]
        assert tuple(w[1] - w[0] for w in want) == lengths and all(w[2] == 0 for w in want)
        assert device_route(model, ss) == want
        for s, w in zip(ss, want):  # and each alone: the launch sized by that slice
            assert device_route(model, [s]) == [w]
        assert sum(len(w[3]) for w in want) > 30 and all(len(w[3]) > 0 for w in want[6:])  # 128 rows and more hold notes
    finally:
        for s in ss:
            s.close()


# ---- 3. statuses, buffers, edge cases (the product library) -------------------------------------------------------------------
def test_an_onset_threshold_of_zero_is_status_1_and_changes_no_other_stream(model, nat, prms, x):
    from basic_pitch_amd import note_creation as nc

    zero = dict(prms, z=nc._note_params(0.0, 0.3, 11, True, None, None, True, 11, True))
    specs = [("roll", 500, 22050, "a", (250_000,), False), ("roll", 500, 22050, "z", (250_000,), False),
             ("keep", 1500, 22050, "z", (0,), False), ("keep", 1500, 22050, "f", (250_000,), False)]
    ss = open_set(model, nat, zero, x, 1, specs)
    try:
        got = device_route(model, ss)
        want = [single_route(model, s) for s in ss]
        assert [g[2] for g in got] == [0, 1, 1, 0] == [w[2] for w in want] and got == want
        assert len(want[0][3]) > 5 and len(want[3][3]) > 5
        assert device_route(model, ss[1:3]) == want[1:3]  # no stream the device decodes: nothing queued
    finally:
        for s in ss:
            s.close()


def test_no_stream_or_no_row_is_ok_with_zero_offsets(model, nat, prms, x):
    from basic_pitch_amd import streaming

    lib = streaming.bind(model._lib)
    offs = (C.c_int64 * 3)(7, 7, 7)
    assert lib.bp_streams_events(model._handle, 0, None, 1, None, 0, None, 0, offs) == 0 and offs[0] == 0
    ss = open_set(model, nat, prms, x, 0, [SPECS[5], SPECS[3]])
    try:
        tab = streaming.events_table([s.s for s in ss])
        assert lib.bp_streams_events(model._handle, 2, C.addressof(tab), 1, None, 0, None, 0, offs) == 0
        assert list(offs) == [0, 0, 0] and [(u.first_row, u.n_rows, u.status) for u in tab] == [(0, 0, 0)] * 2
    finally:
        for s in ss:
            s.close()


def test_too_small_buffers_name_the_sizes_and_the_repeated_call_succeeds(model, nat, prms, x):
    from basic_pitch_amd import streaming

    lib = streaming.bind(model._lib)
    ss = open_set(model, nat, prms, x, 2, SPECS[:5])
    try:
        want = [single_route(model, s) for s in ss]
        n_ev, n_b = sum(len(w[3]) for w in want), sum(r[6] for w in want for r in w[3])
        assert n_ev >= 10 and n_b >= 100
        first = device_route(model, ss, room=(n_ev, n_b))
        assert first == want
        tab = streaming.events_table([s.s for s in ss])
        for room in ((n_ev - 1, n_b), (n_ev, n_b - 1), (0, 0)):
            events = (nat.bp_note_event * max(1, room[0]))()
            bends = np.zeros(max(1, room[1]), np.int32)
            offs = np.full(6, -1, np.int64)
            rc = lib.bp_streams_events(model._handle, 5, C.addressof(tab), 1, C.addressof(events), room[0], bends.ctypes.data, room[1],
                                       offs.ctypes.data_as(C.POINTER(C.c_int64)))
            msg = lib.bp_last_error(model._handle).decode()
            assert rc == nat.BP_ERR_INVALID_ARG and f"{n_ev} events and {n_b} bends are needed" in msg, msg
            assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w[3]) for w in want])]).tolist()
            assert [(u.first_row, u.n_rows, u.status) for u in tab[:5]] == [w[:3] for w in want]
        assert device_route(model, ss, room=(n_ev, n_b)) == first  # the repeat with room
        assert device_route(model, ss) == first  # and through the retry of the Python layer, from its own first guess
        for s in ss:  # the streams are not broken
            assert s.s.push(s.pcm[s.at : s.at + 1000])["note"].shape[1] == 88
    finally:
        for s in ss:
            s.close()


def test_refusals_name_the_stream_and_leave_every_stream_as_it_was(model, nat, prms, x):
    from basic_pitch_amd import note_creation as nc
    from basic_pitch_amd import streaming
    from basic_pitch_amd.inference import Model

    lib = streaming.bind(model._lib)
    bad = dict(prms, neg=nc._note_params(0.5, -0.1, 11, True, None, None, True, 11, True),
               short=nc._note_params(0.5, 0.3, -1, True, None, None, True, 11, True))
    ss = open_set(model, nat, bad, x, 1, [SPECS[0], SPECS[3], ("roll", 300, 22050, "neg", (100_000,), False),
                                          ("keep", 1500, 22050, "short", (100_000,), False)])
    events, bends, offs = (nat.bp_note_event * 4096)(), np.zeros(1 << 17, np.int32), (C.c_int64 * 8)()
    cap = C.c_int64(0)

    def call(ptrs, **kw):
        t = (nat.bp_stream_events * max(1, len(ptrs)))()
        for i, p in enumerate(ptrs):
            t[i].stream = p
        args = dict(events=C.addressof(events), max_events=4096, bends=bends.ctypes.data, max_bends=1 << 17, offs=offs)
        args.update(kw)
        rc = lib.bp_streams_events(model._handle, len(ptrs), C.addressof(t), 1, args["events"], args["max_events"], args["bends"],
                                   args["max_bends"], args["offs"])
        err = lib.bp_last_error(model._handle)
        rc2 = lib.bp_streams_events_layout(model._handle, len(ptrs), C.addressof(t), 1, C.byref(cap), C.byref(cap))
        return rc, rc2, err

    try:
        before = [single_route(model, s) for s in ss[:2]]
        ptrs = [s.s._s.value for s in ss]
        with Model(max_windows=1) as other, other.open_stream(22050) as foreign, model.open_stream(22050) as plain:
            foreign.keep_rolling(prms["a"], 100)
            for streams, word in (
                (ptrs[:2] + [None], b"stream 2: null stream"),
                (ptrs[:1] + [foreign._s.value], b"stream 1: a stream of another handle"),
                (ptrs[:2] + ptrs[:1], b"stream 2: the same stream twice"),
                ([plain._s.value] + ptrs[:1], b"stream 0: the stream retains nothing"),
                (ptrs[:3], b"stream 2: a negative frame threshold"),
                ([ptrs[3], ptrs[2]], b"stream 0: negative min_note_len"),
            ):
                rc, rc2, err = call(streams)
                assert rc == rc2 == nat.BP_ERR_INVALID_ARG and word in err and b"bp_streams_events" in err, (word, err)
        for kw, word in (({"offs": None}, b"event_offsets"), ({"max_events": -1}, b"max_events"), ({"events": None}, b"room without a buffer"),
                         ({"bends": None}, b"room without a buffer")):
            rc, rc2, err = call(ptrs[:2], **kw)
            assert rc == nat.BP_ERR_INVALID_ARG and rc2 == 0 and word in err, (kw, err)
        assert lib.bp_streams_events(model._handle, -1, None, 1, None, 0, None, 0, offs) == nat.BP_ERR_INVALID_ARG
        assert [single_route(model, s) for s in ss[:2]] == before == device_route(model, ss[:2])
    finally:
        for s in ss:
            s.close()


# ---- 4. Python: transcripts(decode="device") -------------------------------------------------------------------------------------
def as_tuples(events):
    return [(np.float64(e[0]).tobytes(), np.float64(e[1]).tobytes(), int(e[2]), np.float32(e[3]).tobytes(),
             None if e[4] is None else list(e[4])) for e in events]


def test_transcripts_on_the_device_equal_every_transcribers_own_transcript(model, x):
    """Twins: A through transcripts(decode="device"), alternating with host refreshes; B through transcript() alone."""
    from basic_pitch_amd.streaming import StreamingTranscriber as ST

    def make():
        return [ST(model, 22050, live=True, horizon_seconds=6.0), ST(model, 22050, live=True, max_rows=1500),
                ST(model, 22050, live=True, max_rows=1500, multiple_pitch_bends=True, minimum_frequency=100.0)]

    A, B = make(), make()
    try:
        at, n_events = 0, 0
        for step, k in enumerate((120_001, 90_000, 96_999)):
            for t in A + B:
                t.push(x[at : at + k])
            at += k
            ref = [t.transcript() for t in B]
            got = model.transcripts(A, decode="device") if step != 1 else model.transcripts(A)  # device, host, device
            for i, ((m1, e1), (m2, e2)) in enumerate(zip(got, ref)):
                assert as_tuples(e1) == as_tuples(e2) and m1.to_bytes() == m2.to_bytes(), (at, i)
                n_events += len(e2)
            again = model.transcripts(A, decode="device", midi=False)
            assert [m for m, _ in again] == [None] * 3 and [as_tuples(e) for _, e in again] == [as_tuples(e) for _, e in ref]
            assert [m for m, _ in model.transcripts(A, midi=False)] == [None] * 3
        assert at == N and n_events > 40
        # the device refreshes left the host rings and the held rows to the host refreshes: A's own transcript() still agrees
        for a, (m2, e2) in zip(A, [t.transcript() for t in B]):
            m1, e1 = a.transcript()
            assert as_tuples(e1) == as_tuples(e2) and m1.to_bytes() == m2.to_bytes()
    finally:
        for t in A + B:
            t.close()


def test_a_slice_over_the_limit_is_status_2_and_takes_the_host_route(model):
    """A keeping stream pushed past BP_EVENTS_MAX_ROWS rows: 96 s of 1e-3 noise and one tone."""
    from basic_pitch_amd import streaming
    from basic_pitch_amd.streaming import StreamingTranscriber as ST

    rng = np.random.default_rng(5)
    n = 96 * 22050
    sig = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    t = np.arange(3 * 22050) / 22050.0
    sig[40 * 22050 : 43 * 22050] += (0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    A, B = ST(model, 22050, live=True, max_rows=9000), ST(model, 22050, live=True, max_rows=9000)
    short = ST(model, 22050, live=True, max_rows=1500)
    try:
        for k in range(0, n, 8 * 36164):
            A.push(sig[k : k + 8 * 36164]), B.push(sig[k : k + 8 * 36164])
        short.push(sig[39 * 22050 : 45 * 22050])
        tab, events, bends, offs = streaming.streams_events(model, [short.stream, A.stream])
        assert tab[1].n_rows > 8192 and (tab[0].status, tab[1].status) == (0, 2) and offs[1] == offs[2] > 0
        (ms, es), (m1, e1) = model.transcripts([short, A], decode="device")
        m2, e2 = B.transcript()
        assert as_tuples(e1) == as_tuples(e2) and m1.to_bytes() == m2.to_bytes() and len(e2) >= 1
        assert as_tuples(es) == as_tuples(short.transcript()[1]) and len(es) >= 1
    finally:
        for s in (A, B, short):
            s.close()


# ---- 5. the tracker's forms on hand-made maps, NaN isolation: one process with the A/B library -------------------------------
@pytest.fixture(scope="module")
def ab_run(tmp_path_factory):
    from basic_pitch_amd import build

    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "streams_events_ab.py")
    out = str(tmp_path_factory.mktemp("stream_events") / "ab.json")
    env = dict(os.environ, BASIC_PITCH_AMD_LIB=build.build_library(ab=True))
    subprocess.run([sys.executable, tool, out], check=True, timeout=300, env=env)
    return json.load(open(out))


def test_every_tracker_form_gives_the_host_decoders_bytes_on_hand_made_maps(ab_run):
    """bp_ab_note_events_from_maps_forms (form 0 as the product chooses, 2 scratch; a parameter set per segment)
    against bp_note_candidates + bp_notes_decode_candidates per segment.  Every case has frame_threshold > 0, so the capacity
    bound proves status 0: none may be left out."""
    groups = {g["name"]: g for g in ab_run["forms"]}
    assert set(groups) == {"fixture cases", "edge shapes", "random maps", "two parameter sets", "frame threshold 0", "tolerance 1"}
    for name, g in groups.items():
        assert g["mismatches"] == [], (name, g["mismatches"][:5])
        assert set(g["forms"]) == {0, 2} and g["statuses"] == [0], (name, g["forms"], g["statuses"])
        assert g["events"] > 0, name
    assert groups["fixture cases"]["segments"] == 16 and groups["fixture cases"]["events"] >= 100
    assert groups["random maps"]["segments"] == 64 and groups["random maps"]["rows"][0] >= 2 and groups["random maps"]["rows"][1] <= 600
    assert groups["edge shapes"]["rows_list"] == [0, 1, 2, 3, 60, 64, 50, 142, 142, 701]
    assert {7, 8, 127, 128, 129, 131, 290} <= set(groups["edge shapes"]["lengths"])


def test_a_nan_in_one_stream_changes_no_other_stream(ab_run):
    """bp_ab_stream_poison on one stream of four: status 1 there, the other three keep the bytes of their single routes."""
    for up in ab_run["poison"]:
        assert up["status"] == [0, 1, 0, 0] == up["single_status"], up
        assert up["equal"] == [True] * 4 and up["events"][1] == 0 and up["events"][0] > 0 and up["events"][2] + up["events"][3] > 0, up
        assert up["rows"][1][0] <= ab_run["poison_row"] < up["rows"][1][1]
