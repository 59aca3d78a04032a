"""AIFF / AIFF-C, CAF, AU and RF64 on the device: the eight sample formats these containers add (BP_PCM_S16_BE ... BP_PCM_ALAW)
against their plain twins — a call with a new format returns, bit for bit, what the same call returns for the plain format
on the converted bytes — through the one-shot call, the streams, the clips calls, the file job and run_inference.  Every
comparison is exact equality."""
import os
import re

import numpy as np
import pytest

import clip_files as CF
import container_files as K

pytestmark = pytest.mark.gpu

NEW_CODES = (K.S16_BE, K.S24_BE, K.S32_BE, K.F32_BE, K.F64_BE, K.S8, K.ULAW, K.ALAW)
N_ODD = 20001  # frames at 44,100 Hz: one window, 39 rows, and a tail of the four-frames-a-thread kernel


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import Model

    m = Model(max_windows=32)
    yield m
    m.close()


def _bytes_of(code, n, channels, rate, seed):
    """uint8 samples of a signal with notes in it; 8-bit formats start with all 256 codes, floats carry denormals and -0.0."""
    x = 0.9 * CF.tones(n, channels, rate, seed)
    if code in (K.F32_BE, K.F64_BE):
        x.reshape(-1)[5::97] = 1e-41 if code == K.F32_BE else 1e-310
        x.reshape(-1)[11::89] = -0.0
    raw = K.encode(x, code).copy()
    if K.WIDTH[code] == 1:
        raw[:256] = np.arange(256, dtype=np.uint8)
    if code in (K.F32_BE, K.F64_BE):
        v = raw.view(">f4" if code == K.F32_BE else ">f8")
        assert not np.isnan(v).any() and (np.abs(v[5::97]) < 1e-38).all() and np.signbit(v[11::89]).all()
    return raw


def _same_maps(a, b):
    assert set(a) == set(b) == {"note", "onset", "contour"}
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == np.float32, k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- 1. the formats against their plain twins ----------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("code", NEW_CODES)
def test_a_new_format_equals_its_plain_twin(model, code, channels):
    raw = _bytes_of(code, N_ODD, channels, 44100, code)
    got = model.predict_pcm_raw(raw, code, N_ODD, channels, 44100)
    want = model.predict_pcm_raw(K.plain_bytes(raw, code), K.PLAIN[code], N_ODD, channels, 44100)
    assert got["note"].shape == (39, 88) and got["note"].max() > 0.3  # there is music in it
    _same_maps(got, want)


def test_every_16_bit_value_once(model):
    v = np.random.default_rng(5).permutation(np.arange(-32768, 32768)).astype(">i2")
    raw = v.view(np.uint8)
    got = model.predict_pcm_raw(raw, K.S16_BE, 65536, 1, 22050)
    _same_maps(got, model.predict_pcm_raw(K.plain_bytes(raw, K.S16_BE), K.S16, 65536, 1, 22050))


@pytest.mark.parametrize("offset", [0, 2])
def test_16_bit_big_endian_stereo_from_device_memory(model, offset):
    """16-byte aligned: the one-load-one-store path with the byte permute; two bytes further on: the general path."""
    import torch

    from basic_pitch_amd import _native

    raw = _bytes_of(K.S16_BE, N_ODD, 2, 44100, 3)
    want = model.predict_pcm_raw(K.plain_bytes(raw, K.S16_BE), K.S16, N_ODD, 2, 44100)
    buf = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset : offset + raw.size]
    view.copy_(torch.from_numpy(raw))
    T = want["note"].shape[0]
    out = {k: torch.full((T, w), -1.0, dtype=torch.float32, device="cuda") for k, w in (("note", 88), ("onset", 88), ("contour", 264))}
    torch.cuda.synchronize()
    rc = model._lib.bp_infer_pcm_raw(model._handle, view.data_ptr(), K.S16_BE, N_ODD, 2, 44100, out["note"].data_ptr(),
                                     out["onset"].data_ptr(), out["contour"].data_ptr(), _native.BP_MEM_DEVICE)
    assert rc == 0, model._lib.bp_last_error(model._handle)
    torch.cuda.synchronize()
    _same_maps({k: v.cpu().numpy() for k, v in out.items()}, want)


def test_a_code_past_the_last_is_refused(model):
    out = np.zeros((4, 440), np.float32)
    rc = model._lib.bp_infer_pcm_raw(model._handle, out.ctypes.data, 14, 8, 1, 44100, out.ctypes.data, out.ctypes.data, out.ctypes.data, 0)
    assert rc == -1 and b"format" in model._lib.bp_last_error(model._handle)


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,channels,rate", [(K.S24_BE, 2, 48000), (K.ULAW, 1, 8000)])
def test_a_stream_of_a_new_format_equals_the_one_shot_call(model, code, channels, rate):
    n = int(2.6 * CF.HOP * rate / 22050)  # three windows
    raw = _bytes_of(code, n, channels, rate, 20 + code)
    want = model.predict_pcm_raw(raw, code, n, channels, rate)
    assert want["note"].shape[0] > 2 * 142
    _same_maps(want, model.predict_pcm_raw(K.plain_bytes(raw, code), K.PLAIN[code], n, channels, rate))
    frame = K.WIDTH[code] * channels
    cuts = [0, 1000, 1001, 1001 + n // 3, 1001 + n // 3 + 7777, n]  # uneven chunks, one of them a single frame
    parts = []
    with model.open_stream(rate, channels, code) as s:
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(s.push(raw[a * frame : b * frame].tobytes()))
        parts.append(s.finish())
    _same_maps({k: np.concatenate([p[k] for p in parts]) for k in want}, want)


# ---- 3. clips ------------------------------------------------------------------------------------------------------------------
def _events_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x[0], x[1], x[2]) == (y[0], y[1], y[2]) and np.float32(x[3]).tobytes() == np.float32(y[3]).tobytes()
        assert (x[4] is None and y[4] is None) or list(x[4]) == list(y[4])


@pytest.mark.parametrize("decode", ["host", "device"])
def test_clips_of_mixed_dtypes_old_and_new(model, decode):
    rate = 44100
    clips = []
    for i, t in enumerate(("<i2", ">i2", "<f4", ">f4", ">i4", ">f8", "u1", "<i4")):
        ch = 1 + i % 2
        x = 0.8 * CF.tones(15000 + 2500 * i, ch, rate, 30 + i)
        kind = np.dtype(t).kind
        if kind == "f":
            a = x.astype(t)
        elif kind == "u":
            a = (np.round(x * 127) + 128).astype(t)
        else:
            a = np.round(x * (2 ** (8 * np.dtype(t).itemsize - 1) - 1)).astype(t)
        clips.append(a)
    got = model.transcribe_clips(clips, rate, decode=decode)
    for i, c in enumerate(clips):
        alone = model.transcribe_clips([c], rate, decode=decode)[0]
        _events_equal(got[i][1], alone[1])
        assert len(alone[1]) > 0
        # ... and a big-endian clip gives what its byte-swapped form gives
        if c.dtype.byteorder == ">":
            _events_equal(got[i][1], model.transcribe_clips([c.astype(c.dtype.newbyteorder("<"))], rate, decode=decode)[0][1])


# ---- 4. the file job -------------------------------------------------------------------------------------------------------------
def _corpus(d):
    """[(file, twin WAV)] of one to three windows each, and the refused files."""
    w = CF.ONE_WINDOW
    spec = [  # name, writer, code, channels, rate, frames
        ("a_aiff_s16", K.aiff_of, K.S16_BE, 2, 44100, 2 * w),          # exactly one full window
        ("b_aiff_s24", K.aiff_of, K.S24_BE, 2, 48000, 100000),
        ("c_aiff_s8", K.aiff_of, K.S8, 1, 22050, 30000),
        ("d_aifc_sowt", K.aiff_of, K.S16, 2, 44100, 70001),
        ("e_aifc_fl32", K.aiff_of, K.F32_BE, 1, 22050, w + 9000),
        ("f_aifc_ulaw", K.aiff_of, K.ULAW, 1, 8000, 24000),
        ("g_caf_s16be", K.caf_of, K.S16_BE, 2, 44100, 50000),
        ("h_caf_f32le", K.caf_of, K.F32, 1, 48000, 60000),
        ("i_au_s16", K.au_of, K.S16_BE, 1, 22050, 2 * w + 5000),     # three windows
        ("j_au_ulaw", K.au_of, K.ULAW, 1, 8000, 16000),
        ("k_rf64_s16", K.rf64_of, K.S16, 2, 44100, 40001),
    ]
    pairs = []
    for i, (name, writer, code, ch, rate, n) in enumerate(spec):
        raw = K.encode(0.8 * CF.tones(n, ch, rate, 40 + i), code)
        ext = {K.aiff_of: ".aif", K.caf_of: ".caf", K.au_of: ".au", K.rf64_of: ".wav"}[writer]
        (d / (name + ext)).write_bytes(writer(raw, code, ch, rate))
        (d / (name + "_twin.wav")).write_bytes(K.twin_wav(raw, code, ch, rate))
        pairs.append((str(d / (name + ext)), str(d / (name + "_twin.wav"))))
    refused = []
    for name in K.REQUIRED_REFUSALS:
        (d / ("z_" + name + ".bin")).write_bytes(K.REFUSED[name][0])
        refused.append(str(d / ("z_" + name + ".bin")))
    return pairs, refused


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return _corpus(tmp_path_factory.mktemp("containers"))


@pytest.mark.parametrize("clip_batch", [0, 8])
def test_the_file_job_writes_what_it_writes_for_the_wav_twins(model, corpus, tmp_path, clip_batch):
    from basic_pitch_amd import _native, transcribe_files

    pairs, refused = corpus
    paths = [p for pair in pairs for p in pair]
    paths = paths[:6] + refused[:2] + paths[6:] + refused[2:]  # the refused files among the others
    lib = model._lib
    rc, routes = CF.probe(lib, paths, CF.params(lib, 8), handles=[model._handle])
    assert rc == 0
    assert all((r < 0) if p in refused else (r == 1) for p, r in zip(paths, routes)), routes
    before = lib.bp_files_batched()
    rep = dict(zip(paths, transcribe_files(paths, tmp_path, models=[model], threads=2, clip_batch=clip_batch)))
    assert lib.bp_files_batched() - before == (2 * len(pairs) if clip_batch else 0)
    for path, twin in pairs:
        r, r0 = rep[path], rep[twin]
        assert r["status"] == 0 and r0["status"] == 0 and r["message"] == "", (path, r, r0)
        assert (r["n_frames"], r["n_note_events"]) == (r0["n_frames"], r0["n_note_events"]) and r["n_note_events"] > 0, (path, r, r0)
        stem, stem0 = (os.path.splitext(os.path.basename(p))[0] for p in (path, twin))
        for ext in ("mid", "csv"):
            a = open(os.path.join(tmp_path, f"{stem}_basic_pitch.{ext}"), "rb").read()
            assert a == open(os.path.join(tmp_path, f"{stem0}_basic_pitch.{ext}"), "rb").read(), (path, ext)
    for path, name in zip(refused, K.REQUIRED_REFUSALS):
        r = rep[path]
        assert r["status"] == _native.BP_ERR_BAD_AUDIO and re.search(K.REFUSED[name][1], r["message"]), (name, r)
    assert len(os.listdir(tmp_path)) == 2 * 2 * len(pairs)


# ---- 5. run_inference and predict ------------------------------------------------------------------------------------------------
def test_run_inference_and_predict_on_an_aiff_and_its_wav_twin(model, corpus):
    from basic_pitch_amd import inference

    aiff, twin = corpus[0][0]
    _same_maps(inference.run_inference(aiff, model), inference.run_inference(twin, model))
    _, _, ev = inference.predict(aiff, model)
    _, _, ev0 = inference.predict(twin, model)
    assert len(ev) > 0
    _events_equal(ev, ev0)
    for path, tw in corpus[0][1:]:  # every other container too
        _same_maps(inference.run_inference(path, model), inference.run_inference(tw, model))
