"""G.711 and IMA ADPCM files on the device (include/basic_pitch_amd_adpcm.h; csrc/adpcm_device.hip): the device decoder bit for
bit against the host decoder (which tests/test_adpcm_cpu.py holds to audioop) at the lane, wave and workgroup edges of the
launch; bp_infer_adpcm and bp_infer_adpcm_candidates against the BP_PCM_S16 route on the host-decoded samples;
bp_infer_adpcm_clips_events clip by clip against bp_infer_clips_events; the file job on IMA files against the job on their S16
WAV twins, per file and batched; G.711 WAV against its AU twin; and the new buffers' memory, which leaves with the handle."""
import ctypes as C
import os

import numpy as np
import pytest

import adpcm_files as A
import clip_files as CF
import container_files as K
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd.inference import Model

    with Model(device=0, max_windows=8) as m:
        yield m


def host(lib, blob):
    from basic_pitch_amd import adpcm_clips

    return adpcm_clips.host_decode(lib, blob)


def device(model, blob):
    pcm, _ = model.adpcm_decode_device(blob)
    return pcm


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def _edge_files():
    """name -> file: both containers, mono and stereo, block sizes {smallest, 256, 2048}, 1 / 63 / 64 / 65 / 257 blocks (the
    chains of a launch end inside a wave, at a wave's end, one past it, and past a workgroup of 256)."""
    files = {}
    for ch in (1, 2):
        for B in (8 * ch, 256, 2048):
            bf = A.wav_block_frames(B, ch)
            for blocks in (1, 63, 64, 65, 257):
                n = blocks * bf - (bf // 3 if blocks > 1 else 0)  # the fact chunk cuts the last block
                files[f"wav {ch}ch B{B} x{blocks}"] = A.ima_wav(A.two_tones(n, ch, 8000, seed=blocks), 8000, B)
        for packets in (1, 63, 64, 65, 257):
            files[f"caf {ch}ch x{packets}"] = A.ima4_caf(A.two_tones(packets * 64 - (17 if packets > 1 else 0), ch, 22050, seed=packets), 22050)
        blocks, B = A.random_wav_blocks(ch)
        files[f"wav {ch}ch random codes"] = A.ima_wav_of(blocks, ch, 44100, B)
        files[f"caf {ch}ch random codes"] = A.ima4_caf_of(A.random_ima4_packets(ch), ch, 44100)
    files["wav no frames"] = A.ima_wav_of(b"", 2, 8000, 256, fact=0)
    files["wav partial tail"] = A.ima_wav_of(A.wav_blocks(A.two_tones(505, 1, 8000), 256), 1, 8000, 256, fact=None, tail=bytes(99))
    return files


def test_the_device_decoder_equals_the_host_decoder(model):
    lib = model._lib
    for name, blob in _edge_files().items():
        want, lay = host(lib, blob)
        got = device(model, blob)
        assert got.shape == want.shape == (lay["n_frames"], lay["channels"]), name
        assert np.array_equal(got, want), (name, int(np.argmax((got != want).any(axis=1))))
    # the count alone; a buffer that is too small; a file that is no such file
    blob = _edge_files()["wav 2ch B256 x65"]
    n = C.c_int64()
    assert lib.bp_adpcm_decode_device(model._handle, blob, len(blob), None, 0, C.byref(n)) == 0 and n.value == host(lib, blob)[1]["n_frames"]
    small = np.zeros(8, np.int16)
    assert lib.bp_adpcm_decode_device(model._handle, blob, len(blob), small.ctypes.data, 2, C.byref(n)) == -1
    assert b"too small" in lib.bp_last_error(model._handle)
    pcm = K.wav_of(bytes(64), K.S16, 2, 44100)
    assert lib.bp_adpcm_decode_device(model._handle, pcm, len(pcm), small.ctypes.data, 2, C.byref(n)) == -7
    assert b"not an IMA ADPCM file" in lib.bp_last_error(model._handle)


# ---- the posteriorgrams -----------------------------------------------------------------------------------------------------------------
def _music(n, ch, rate, seed):
    return np.round(CF.tones(n, ch, rate, seed) * 32767 * 0.9).astype(np.int16)


def _infer_files():
    w = CF.ONE_WINDOW
    return {
        "8 kHz mono wav, one window": A.ima_wav(_music(8000, 1, 8000, 1), 8000, 256),
        "8 kHz mono wav, two windows": A.ima_wav(_music(w * 8000 // 22050 + 3000, 1, 8000, 2), 8000, 256),
        "44.1 kHz stereo wav, one window": A.ima_wav(_music(40000, 2, 44100, 3), 44100, 2048),
        "44.1 kHz stereo wav, two windows": A.ima_wav(_music(2 * w + 9000, 2, 44100, 4), 44100, 2048),
        "22.05 kHz stereo caf, one window": A.ima4_caf(_music(20000, 2, 22050, 5), 22050),
        "22.05 kHz stereo caf, two windows": A.ima4_caf(_music(w + 7000, 2, 22050, 6), 22050),
    }


def _prm(model, **kw):
    from basic_pitch_amd import _native

    prm = _native.bp_note_params()
    model._lib.bp_note_params_default(C.byref(prm))
    for k, v in kw.items():
        setattr(prm, k, v)
    return prm


def test_infer_adpcm_equals_the_s16_route(model):
    from basic_pitch_amd import _native

    lib = model._lib
    for name, blob in _infer_files().items():
        pcm, lay = host(lib, blob)
        want = model.predict_pcm_raw(pcm, _native.BP_PCM_S16, lay["n_frames"], lay["channels"], lay["sample_rate"])
        got = model.predict_adpcm(blob)
        windows = lib.bp_handle_track_n_windows(model._handle, lib.bp_handle_resampled_length(model._handle, lay["n_frames"], lay["sample_rate"]))
        assert windows == (2 if "two" in name else 1), name
        for k in ("note", "onset", "contour"):
            assert got[k].shape == want[k].shape and got[k].shape[0] > 0 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    # every output is checked before anything is queued
    blob = _infer_files()["8 kHz mono wav, one window"]
    assert lib.bp_infer_adpcm(model._handle, blob, len(blob), None, None, None, _native.BP_MEM_HOST) == -1


def test_candidates_equal_the_s16_route(model):
    from basic_pitch_amd import _native

    lib = model._lib
    prm = _prm(model)
    for name in ("44.1 kHz stereo wav, two windows", "22.05 kHz stereo caf, one window"):
        blob = _infer_files()[name]
        pcm, lay = host(lib, blob)
        T = model._pcm_frames(lay["n_frames"], lay["sample_rate"])
        outs = []
        for route in ("adpcm", "s16"):
            note, bits, bend = np.zeros((T, 88), np.float32), np.zeros((T, 12), np.uint8), np.zeros((T, 88), np.int8)
            status = C.c_int(-1)
            if route == "adpcm":
                rc = lib.bp_infer_adpcm_candidates(model._handle, blob, len(blob), C.byref(prm), note.ctypes.data, bits.ctypes.data,
                                                   bend.ctypes.data, C.byref(status))
            else:
                rc = lib.bp_infer_pcm_raw_candidates(model._handle, pcm.ctypes.data, _native.BP_PCM_S16, lay["n_frames"], lay["channels"],
                                                     lay["sample_rate"], C.byref(prm), note.ctypes.data, bits.ctypes.data, bend.ctypes.data,
                                                     C.byref(status))
            assert rc == 0 and status.value == 0, (name, route, lib.bp_last_error(model._handle))
            cap_ev, cap_b = 4096, 88 * T
            ev = (_native.bp_note_event * cap_ev)()
            bends = np.zeros(cap_b, np.int32)
            n_ev, n_b = C.c_int64(), C.c_int64()
            assert lib.bp_notes_decode_candidates(note.ctypes.data, bits.ctypes.data, bend.ctypes.data, T, C.byref(prm), C.addressof(ev), cap_ev,
                                                  bends.ctypes.data, cap_b, C.byref(n_ev), C.byref(n_b)) == 0
            outs.append((note.tobytes(), bits.tobytes(), bend.tobytes(), bytes(ev)[: n_ev.value * C.sizeof(_native.bp_note_event)],
                         bends[: n_b.value].tobytes(), n_ev.value))
        assert outs[0] == outs[1] and outs[0][5] > 0, name


# ---- many clips in one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", ["wav", "caf"])
def test_clips_events_equal_the_pcm_clips_call(model, container):
    from basic_pitch_amd import adpcm_clips, events

    lib = model._lib
    w, rate, ch = CF.ONE_WINDOW, 22050, 2
    B = 512
    frames = [w - 100, 0, 2 * w + 500, A.wav_block_frames(B, ch) if container == "wav" else 64, w + 9000]  # 1, none, 3, a single block, 2
    write = (lambda x: A.ima_wav(x, rate, B)) if container == "wav" else (lambda x: A.ima4_caf(x, rate))
    blobs = [write(_music(n, ch, rate, 10 + i) if n else np.zeros((0, ch), np.int16)) for i, n in enumerate(frames)]
    arrays = [host(lib, b)[0] for b in blobs]
    assert [a.shape[0] for a in arrays] == frames
    prm = _prm(model)
    got = adpcm_clips.infer_adpcm_clips_events(model, blobs, prm)
    want = events.infer_clips_events(model, arrays, rate, prm)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and list(want[3]) == [0] * 5
    n_ev = int(want[2][-1])
    size = C.sizeof(got[0]._type_)
    assert n_ev > 0 and bytes(got[0])[: n_ev * size] == bytes(want[0])[: n_ev * size]
    n_b = sum(e.n_bends for e in list(want[0])[:n_ev])
    assert np.array_equal(got[1][:n_b], want[1][:n_b])
    assert want[2][1] == want[2][2] and want[2][0] < want[2][1]  # the empty clip has no events, its neighbours do
    # clips of two channel counts in one call are refused before anything is queued; so is a clip that is no such file
    other = A.ima_wav(_music(5000, 1, rate, 3), rate, 256) if container == "wav" else A.ima4_caf(_music(5000, 1, rate, 3), rate)
    with pytest.raises(ValueError, match="clip 1: .*one codec, rate and channel count per call"):
        adpcm_clips.infer_adpcm_clips_events(model, [blobs[0], other], prm)
    tab, keep = adpcm_clips.clip_table([blobs[0], K.wav_of(bytes(64), K.S16, 2, rate)])
    offs, status = np.zeros(3, np.int64), np.zeros(2, np.int32)
    assert lib.bp_infer_adpcm_clips_events(model._handle, 2, tab, C.byref(prm), None, 0, None, 0, offs.ctypes.data, status.ctypes.data) == -7
    assert b"clip 1: " in lib.bp_last_error(model._handle)
    # the public entry: the same events either way
    a = model.transcribe_adpcm_clips(blobs, decode="device")
    b = model.transcribe_adpcm_clips(blobs, decode="host")
    assert [r[1] for r in a] == [r[1] for r in b] and sum(len(r[1]) for r in a) == n_ev


# ---- the file job -------------------------------------------------------------------------------------------------------------------------
def _job(model, paths, out, **kw):
    from basic_pitch_amd import transcribe_files

    os.makedirs(out)
    before = model._lib.bp_files_batched()
    rep = transcribe_files([str(p) for p in paths], str(out), models=[model], threads=2, **kw)
    batched = model._lib.bp_files_batched() - before
    listing = {name: open(os.path.join(out, name), "rb").read() for name in sorted(os.listdir(out))}
    return listing, rep, batched


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, model):
    """Six short IMA files (three WAV, three CAF ima4) and one of 16 windows, and — under the same names in a second directory
    — the S16 WAV files of the host-decoded samples."""
    lib = model._lib
    d, twin = tmp_path_factory.mktemp("ima"), tmp_path_factory.mktemp("ima_twins")
    w = CF.ONE_WINDOW
    files = [
        ("a.wav", A.ima_wav(_music(w - 50, 1, 22050, 21), 22050, 256)),
        ("b.caf", A.ima4_caf(_music(30000, 2, 44100, 22), 44100)),
        ("c.wav", A.ima_wav(_music(2 * w + 3000, 2, 44100, 23), 44100, 2048)),
        ("d.caf", A.ima4_caf(_music(w + 6000, 1, 22050, 24), 22050)),
        ("e.wav", A.ima_wav(_music(40000, 2, 44100, 25), 44100, 2048, extensible=True)),
        ("f.caf", A.ima4_caf(_music(25000, 2, 44100, 26), 44100)),
        ("g_long.wav", A.ima_wav(_music(CF.MAX_SHORT + 1, 1, 22050, 27), 22050, 1024)),
    ]
    paths, twins = [], []
    for name, blob in files:
        (d / name).write_bytes(blob)
        pcm, lay = host(lib, blob)
        stem = os.path.splitext(name)[0]
        (twin / (stem + ".wav")).write_bytes(K.wav_of(pcm.astype("<i2").tobytes(), K.S16, lay["channels"], lay["sample_rate"]))
        paths.append(d / name), twins.append(twin / (stem + ".wav"))
    return paths, twins


def test_the_file_job_writes_what_it_writes_for_the_s16_twins(model, corpus, tmp_path):
    paths, twins = corpus
    want, rep0, _ = _job(model, twins, tmp_path / "twins")
    assert all(r["status"] == 0 for r in rep0) and len(want) == 14 and sum(r["n_note_events"] for r in rep0) > 20
    rc, routes = CF.probe(model._lib, paths, CF.params(model._lib, 4), handles=[model._handle])
    assert rc == 0 and routes == [1] * 6 + [0]
    for k, (kw, n_batched) in enumerate((({"clip_batch": 0}, 0), ({"clip_batch": 4}, 6), ({"host_decode": True}, 0),
                                         ({"clip_batch": 4, "host_decode": True}, 0))):
        got, rep, batched = _job(model, paths, tmp_path / f"ima{k}", **kw)
        assert batched == n_batched, kw
        assert sorted(got) == sorted(want), kw
        for name in want:
            assert got[name] == want[name], (kw, name)
        for r, r0 in zip(rep, rep0):
            assert (r["status"], r["n_note_events"], r["n_frames"], r["message"]) == (0, r0["n_note_events"], r0["n_frames"], ""), kw


def test_g711_wav_equals_its_au_twin(model, tmp_path):
    from basic_pitch_amd import inference

    w = CF.ONE_WINDOW
    d, twin = tmp_path / "g711", tmp_path / "g711_au"
    d.mkdir(), twin.mkdir()
    paths, twins = [], []
    for i, (law, ch, rate, n, kw) in enumerate((("ulaw", 1, 8000, 9000, {}), ("alaw", 2, 8000, 12000, {"extensible": True}),
                                               ("ulaw", 2, 22050, w + 3000, {"rf64": True}), ("alaw", 1, 44100, 50000, {}))):
        code = K.ULAW if law == "ulaw" else K.ALAW
        codes = K.encode(CF.tones(n, ch, rate, 30 + i), code)
        (d / f"g{i}.wav").write_bytes(A.g711_wav(codes, law, ch, rate, **kw))
        (twin / f"g{i}.au").write_bytes(K.au_of(codes, code, ch, rate))
        paths.append(d / f"g{i}.wav"), twins.append(twin / f"g{i}.au")
    for p, q in zip(paths, twins):
        a, b = inference.run_inference(str(p), model), inference.run_inference(str(q), model)
        for k in ("note", "onset", "contour"):
            assert a[k].shape[0] > 0 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (p.name, k)
    want, rep0, n0 = _job(model, twins, tmp_path / "out_au", clip_batch=4)
    got, rep, n1 = _job(model, paths, tmp_path / "out_wav", clip_batch=4)
    assert n0 == n1 == 4 and sorted(got) == sorted(want) and len(want) == 8
    for name in want:
        assert got[name] == want[name], name
    assert all(r["status"] == 0 for r in rep) and [r["n_note_events"] for r in rep] == [r["n_note_events"] for r in rep0]


def test_run_inference_takes_ima_files_natively(model, corpus):
    from basic_pitch_amd import _native, inference

    paths, _ = corpus
    for p in paths[:4]:
        blob = p.read_bytes()
        pcm, lay = host(model._lib, blob)
        want = model.predict_pcm_raw(pcm, _native.BP_PCM_S16, lay["n_frames"], lay["channels"], lay["sample_rate"])
        got = inference.run_inference(str(p), model)
        for k in ("note", "onset", "contour"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (p.name, k)


# ---- memory ---------------------------------------------------------------------------------------------------------------------------------
def test_the_adpcm_buffers_leave_with_the_handle():
    """The form of tests/test_gpu_device_memory.py: the A/B library counts the bytes its buffers hold."""
    from basic_pitch_amd import _native as nat
    from basic_pitch_amd import build

    ab = nat.load_library(build.build_library(ab=True))
    ab.bp_ab_live_device_bytes.restype, ab.bp_ab_live_device_bytes.argtypes = C.c_int64, []
    live = ab.bp_ab_live_device_bytes
    weights = open(os.path.join(ROOT, "basic_pitch_amd", "assets", "nmp_weights.bin"), "rb").read()
    start = live()
    blob = A.ima_wav(_music(30000, 2, 44100, 40), 44100, 2048)
    clip = A.ima4_caf(_music(20000, 2, 22050, 41), 22050)
    prm = nat.bp_note_params()
    ab.bp_note_params_default(C.byref(prm))
    for cycle in range(2):
        h = C.c_void_p()
        assert ab.bp_create(weights, len(weights), 0, 0, 2, C.byref(h)) == 0, ab.bp_last_error(None)
        at_create = live()
        n = C.c_int64()
        assert ab.bp_adpcm_decode_device(h, blob, len(blob), None, 0, C.byref(n)) == 0 and n.value == 30000
        after_decode = live()
        assert after_decode >= at_create + len(blob) - 200 + 30000 * 4  # the file's blocks and its samples, at least
        T = ab.bp_handle_track_n_frames(h, ab.bp_handle_resampled_length(h, 30000, 44100))
        maps = [np.empty((T, k), np.float32) for k in (88, 88, 264)]
        assert ab.bp_infer_adpcm(h, blob, len(blob), *[m.ctypes.data for m in maps], nat.BP_MEM_HOST) == 0
        tab = (nat.bp_adpcm_clip * 2)()
        keep = [np.frombuffer(clip, np.uint8)] * 2
        for i, a in enumerate(keep):
            tab[i] = nat.bp_adpcm_clip(a.ctypes.data, a.size)
        ev = (nat.bp_note_event * 4096)()
        bends, offs, status = np.zeros(1 << 16, np.int32), np.zeros(3, np.int64), np.zeros(2, np.int32)
        assert ab.bp_infer_adpcm_clips_events(h, 2, tab, C.byref(prm), C.addressof(ev), 4096, bends.ctypes.data, bends.size, offs.ctypes.data,
                                              status.ctypes.data) == 0, ab.bp_last_error(h)
        assert live() > after_decode, cycle
        ab.bp_destroy(h)
        assert live() == start, cycle
