"""Every sink of the job driver (csrc/clips_job.h: the candidates and events sinks of clips_api.hip, clips_sweep.hip,
clips_multipitch.hip, clips_melody.hip, clips_align.hip, clips_beat.hip) on ONE handle and ONE job, one after the other: each
sink's outputs are the same bytes whichever sinks ran before it, and the same from maps in host and in device memory.  A sink
that reads a plane another sink's call left behind, or a shared helper that serves one sink differently after another, fails
here.  The job is that of test_one_job_gives_the_same_events_by_every_route (tests/test_gpu_clips_events.py): three segments
of 142, 0 and 284 rows — the smallest with an empty segment between two that have rows — on a handle of two windows."""
import ctypes as C

import numpy as np
import pytest

import align_cases as AC
import beat_cases as BC
import melody_cases as MLC
import multipitch_cases as MC
import score_cases as SCC
from test_gpu_clips import _signal
from test_gpu_clips_events import _prm, _records

pytestmark = pytest.mark.gpu

# the note sets of a sweep: the defaults, and the second set of test_the_fixture_cases_as_one_call_of_16_segments
NOTE_SETS = ({}, {"onset_thresh": 0.6, "frame_thresh": 0.25, "min_note_len": 5, "infer_onsets": False, "min_freq": 80.0, "max_freq": 1500.0})


@pytest.fixture(scope="module")
def job():
    """The handle, the clips, their maps (made once: bp_infer_clips_candidates for the rows, then clip by clip
    bp_infer_pcm_raw_candidates + bp_track_maps), and the references the scored sinks take, derived from the job's own results."""
    import torch

    from basic_pitch_amd import _native, align as AL, clips as CL, events as EV, melody as ME
    from basic_pitch_amd.inference import Model

    rng = np.random.default_rng(31)
    frames = (2 * 36164, 0, 4 * 36164)
    arrays = [np.clip(np.round(np.stack([_signal(rng, f, 44100)] * 2, axis=1) * 32767), -32768, 32767).astype(np.int16)
              if f else np.zeros((0, 2), np.int16) for f in frames]
    prm = _prm({})
    with Model(device=0, max_windows=2) as m:
        offs = CL.infer_clips_candidates(m, arrays, 44100, prm)[0]
        assert offs.tolist() == [0, 142, 142, 426]
        maps = {k: np.zeros((426, w), np.float32) for k, w in (("note", 88), ("onset", 88), ("contour", 264))}
        for i, a in enumerate(arrays):
            r0, r1 = int(offs[i]), int(offs[i + 1])
            if r1 == r0:
                continue
            status = C.c_int(-1)
            one = [np.empty((r1 - r0, w), t) for w, t in ((88, np.float32), (12, np.uint8), (88, np.int8))]
            rc = m._lib.bp_infer_pcm_raw_candidates(m._handle, a.ctypes.data, CL.FORMATS[a.dtype], a.shape[0], 2, 44100, C.byref(prm),
                                                    one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, C.byref(status))
            _native.check(m._lib, m._handle, rc, "bp_infer_pcm_raw_candidates")
            part = {k: np.empty_like(v[r0:r1]) for k, v in maps.items()}
            rc = m._lib.bp_track_maps(m._handle, r1 - r0, part["note"].ctypes.data, part["onset"].ctypes.data,
                                      part["contour"].ctypes.data, _native.BP_MEM_HOST)
            _native.check(m._lib, m._handle, rc, "bp_track_maps")
            for k in maps:
                maps[k][r0:r1] = part[k]
        dev = {k: torch.from_numpy(v).cuda() for k, v in maps.items()}
        torch.cuda.synchronize()
        ptrs = {_native.BP_MEM_HOST: {k: v.ctypes.data for k, v in maps.items()}, _native.BP_MEM_DEVICE: {k: v.data_ptr() for k, v in dev.items()}}
        # the references: every segment's own notes (its first six, on the segment's clock) and its own melody, bent by the helper
        events, bends, ev_offs, _ = EV.note_events_from_maps(m, offs, *[maps[k].ctypes.data for k in ("note", "onset", "contour")],
                                                             _native.BP_MEM_HOST, prm)
        refs = [SCC.notes([(e.start_s, e.end_s, float(e.pitch_midi)) for e in events[int(ev_offs[i]) : int(ev_offs[i + 1])][:6]])
                for i in range(3)]
        points, _ = ME.melody_from_maps(m, offs, maps["contour"].ctypes.data, _native.BP_MEM_HOST, MLC.params())
        states = [AL.states_from_notes(np.asarray(r, np.float64).reshape(-1, 3), int(offs[i + 1] - offs[i]))[0] if offs[i + 1] > offs[i]
                  else np.zeros(0, AL.ALIGN_STATE) for i, r in enumerate(refs)]
        yield dict(model=m, arrays=arrays, offs=offs, ptrs=ptrs, keep=(maps, dev), prm=prm, refs=refs,
                   ref_pitch=MLC.ref_for(np.random.default_rng(5), points), states=np.concatenate(states),
                   state_offs=np.concatenate([[0], np.cumsum([len(s) for s in states])]).astype(np.int64))


def _fields(rec):
    """the records of a structured array but for the statuses: is any of them not zero"""
    return any(rec[name].any() for name in rec.dtype.names if name != "status")


def _sinks(job):
    """name -> (the call on maps of one memory kind -> its outputs as bytes and tuples, is the result more than nothing)"""
    from basic_pitch_amd import align as AL, beat as BT, clips as CL, events as EV, frame_score as FS, melody as ME, multipitch as MP
    from basic_pitch_amd import score as SC, sweep as SW

    m, offs, prm, refs = job["model"], job["offs"], job["prm"], job["refs"]
    sets = [_prm(a) for a in NOTE_SETS]
    mp_sets = [MC.params(), MC.params(min_bin=MC.BANDS[4][0], max_bin=MC.BANDS[4][1])]
    three = lambda p: (p["note"], p["onset"], p["contour"])

    def events_out(got):
        events, bends, ev_offs, status = got
        return (_records(events, bends, 0, int(ev_offs[-1]), True), ev_offs.tobytes(), status.tobytes()), int(ev_offs[-1]) > 0

    def candidates(p, kind):  # (its PCM entry: the product library has no other)
        o, note, bits, bend, st = CL.infer_clips_candidates(m, job["arrays"], 44100, prm)
        return (o.tobytes(), note.tobytes(), bits.tobytes(), bend.tobytes(), st.tobytes()), bool(bits.any())

    def frame_score(p, kind):
        note, frames = FS.note_events_sweep_frame_score(m, offs, *three(p), kind, sets, refs)
        return (note.tobytes(), frames.tobytes()), bool(note["matched_onset"].any() and frames["true_pos"].any())

    def score(p, kind):
        got = SC.note_events_sweep_score(m, offs, *three(p), kind, sets, refs)
        return got.tobytes(), bool(got["matched_onset"].any())

    def mp_points(p, kind):
        pts, p_offs, st = MP.multipitch_from_maps(m, offs, p["contour"], kind, mp_sets[0])
        return (pts.tobytes(), p_offs.tobytes(), st.tobytes()), len(pts) > 0

    def mp_scored(p, kind):
        got = MP.multipitch_sweep_frame_score(m, offs, p["contour"], kind, mp_sets, refs)
        return got.tobytes(), bool(got["true_pos"].any())

    def melody(p, kind):
        pts, st = ME.melody_from_maps(m, offs, p["contour"], kind, MLC.params())
        return (pts.tobytes(), st.tobytes()), bool((pts["bin"] >= 0).any())

    def melody_scored(p, kind):
        got = ME.melody_sweep_score(m, offs, p["contour"], kind, MLC.SETS[:2], job["ref_pitch"])
        return got.tobytes(), _fields(got)

    def align(p, kind):
        ff, total, st = AL.align_from_maps(m, offs, p["note"], p["onset"], kind, job["state_offs"], job["states"], AC.DEFAULT)
        return (ff.tobytes(), total.tobytes(), st.tobytes()), bool((ff >= 0).any() and (st == 0).all())

    def beats(p, kind):
        summaries, b, b_offs = BT.beats_from_maps(m, offs, p["onset"], kind, BT.beat_params(BC.PARAM_SETS["default"]))
        return (summaries.tobytes(), b.tobytes(), b_offs.tobytes()), len(b) > 0

    return {
        "candidates": candidates,
        "events": lambda p, kind: events_out(EV.note_events_from_maps(m, offs, *three(p), kind, prm)),
        "sweep": lambda p, kind: events_out(SW.note_events_sweep(m, offs, *three(p), kind, sets)),
        "score": score, "frame score": frame_score, "multi-pitch points": mp_points, "multi-pitch scored sweep": mp_scored,
        "melody records": melody, "melody scored sweep": melody_scored, "alignment": align, "beats": beats,
    }


def test_every_sink_gives_the_same_bytes_after_any_other_and_from_host_and_device_maps(job):
    sinks = _sinks(job)
    kinds = sorted(job["ptrs"])  # host, device
    first = {}
    for name, call in sinks.items():
        for kind in kinds:
            got, something = call(job["ptrs"][kind], kind)
            assert something, (name, kind, "the fixture gives this sink nothing to compare")
            first[name, kind] = got
        assert first[name, kinds[0]] == first[name, kinds[1]], (name, "host maps against device maps")
    for name, call in reversed(list(sinks.items())):
        for kind in reversed(kinds):
            got, _ = call(job["ptrs"][kind], kind)
            assert got == first[name, kind], (name, kind, "after the sinks in the reverse order")
