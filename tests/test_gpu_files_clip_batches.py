"""Batches of short files in the native file job (`transcribe_files(clip_batch=N)`, bp_transcribe_params.clip_batch): the
short files of a claimed run go through one clips-events call per container and sample rate, and the job writes the SAME
output files, byte for byte, and the same reports as the per-file route (`clip_batch=0`) — whatever the batch size, the
number of lanes and threads, and whichever files fall back to the per-file route.  `bp_files_batched()` counts the files
whose outputs really came from a batched call: the tests hold it to the exact number the probe announces, so that a batch
route which silently fell back for every file could not pass."""
import os

import numpy as np
import pytest

import clip_files as CF
import flac_writer as FW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from basic_pitch_amd import Model

    m = Model(max_windows=32)
    yield m
    m.close()


def _flac(path, n, channels, rate, bits, seed, **kw):
    pcm = np.round(CF.tones(n, channels, rate, seed) * (1 << (bits - 1)) * 0.9).astype(np.int64)
    with open(path, "wb") as f:
        f.write(FW.encode(pcm, rate, bits, **kw))
    return str(path)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The 14 input files, in job order, and the stem whose .mid exists in every output directory before the job runs."""
    d = tmp_path_factory.mktemp("short_files")
    (d / "sub").mkdir()
    w = CF.ONE_WINDOW
    paths = [
        CF.write_wav(d / "a_s16_44k_1w.wav", CF.tones(2 * w, 2, 44100, 1), "s16", 44100),      # exactly one full window
        CF.write_wav(d / "b_f32_22k_2w.wav", CF.tones(w + 5000, 1, 22050, 2), "f32", 22050),
        _flac(d / "c_16_44k.flac", 12000, 2, 44100, 16, 3, blocksize=1152),
        CF.write_wav(d / "d_s24_48k_1w.wav", CF.tones(40000, 2, 48000, 4), "s24", 48000),
        CF.write_wav(d / "e_long_16w.wav", CF.tones(CF.MAX_SHORT + 1, 1, 22050, 5), "u8", 22050),   # 16 windows: per file
        CF.write_wav(d / "f_u8_22k_1w.wav", CF.tones(20000, 1, 22050, 6), "u8", 22050),
        _flac(d / "g_16_22k.flac", 14000, 1, 22050, 16, 7, blocksize=576),
        CF.write_wav(d / "h_zero.wav", np.zeros((0, 2)), "s16", 44100),                         # no frames: empty outputs
        CF.write_wav(d / "sub" / "a_s16_44k_1w.wav", CF.tones(9000, 1, 22050, 8), "s16", 22050),  # the stem of the first file
        CF.write_wav(d / "i_s16_48k_2w.wav", CF.tones(90000, 1, 48000, 9), "s16", 48000),
        _flac(d / "j_24_44k.flac", 9000, 2, 44100, 24, 10, blocksize=4096),
        CF.write_wav(d / "k_exists.wav", CF.tones(15000, 1, 22050, 11), "s16", 22050),           # its .mid is there already
        CF.write_wav(d / "m_f32_44k_1w.wav", CF.tones(30000, 2, 44100, 12), "f32", 44100),
    ]
    corrupt = d / "l_corrupt.wav"
    corrupt.write_bytes(open(paths[0], "rb").read()[:36])  # RIFF/WAVE with a fmt chunk and no samples
    paths.insert(11, str(corrupt))
    assert len(paths) == 14
    return {"paths": paths, "exists": "k_exists", "dup": 8}


_JOBS = []


def _run(model, corpus, base, paths=None, **kw):
    """One job into a fresh directory that already holds the pre-existing output: ({file name: bytes}, reports, batched files).
    Every job writes into the SAME path (a message names the output directory, and shortens a long path to its tail, so only
    equal paths give equal messages); once its files are read the directory is moved aside."""
    from basic_pitch_amd import transcribe_files

    out = os.path.join(str(base), "job")
    os.makedirs(out)
    with open(os.path.join(out, corpus["exists"] + "_basic_pitch.mid"), "wb") as f:
        f.write(b"was here first")
    lib = model._lib
    before = lib.bp_files_batched()
    kw.setdefault("models", [model])
    try:
        rep = transcribe_files(paths if paths is not None else corpus["paths"], out, **kw)
        delta = lib.bp_files_batched() - before
        listing = {name: open(os.path.join(out, name), "rb").read() for name in sorted(os.listdir(out))}
    finally:
        _JOBS.append(None)
        os.rename(out, os.path.join(str(base), "done%03d" % len(_JOBS)))
    return listing, rep, delta


def _same(got, want):
    listing, rep, _ = got
    listing0, rep0, _ = want
    assert sorted(listing) == sorted(listing0)
    for name in listing0:
        assert listing[name] == listing0[name], name
    assert len(rep) == len(rep0)
    for i, (r, r0) in enumerate(zip(rep, rep0)):
        for k in ("status", "n_note_events", "n_frames", "message"):
            want_k = r0[k]
            assert r[k] == want_k, (i, k, r[k], want_k)
        assert set(r["ms"]) == set(r0["ms"]) and all(v >= 0 for v in r["ms"].values())


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    return tmp_path_factory.mktemp("outputs")


@pytest.fixture(scope="module")
def per_file(model, corpus, outs):
    """The per-file route's job (clip_batch=0), run once and left unchanged: what every batched job must equal."""
    return _run(model, corpus, outs, threads=2)


@pytest.fixture(scope="module")
def announced(model, corpus):
    """What the probe announces for the corpus with the lanes' geometry, and how many of its files a job can batch."""
    lib = model._lib
    rc, routes = CF.probe(lib, corpus["paths"], CF.params(lib, 4), handles=[model._handle])
    assert rc == 0
    assert CF.probe(lib, corpus["paths"], CF.params(lib, 4)) == (0, routes)  # the default mode's geometry is the lanes'
    names = [os.path.basename(p) for p in corpus["paths"]]
    want = {"e_long_16w.wav": 0, "c_16_44k.flac": 2, "g_16_22k.flac": 2, "j_24_44k.flac": 2}
    for name, r in zip(names, routes):
        assert (r < 0) if name == "l_corrupt.wav" else r == want.get(name, 1), (name, r)
    skip = {corpus["dup"], names.index(corpus["exists"] + ".wav")}
    return sum(1 for i, r in enumerate(routes) if r > 0 and i not in skip)


def test_off_is_off_and_the_per_file_job_is_what_it_was(per_file, corpus):
    listing, rep, delta = per_file
    assert delta == 0
    names = [os.path.basename(p) for p in corpus["paths"]]
    bad = {names.index("l_corrupt.wav"): "missing fmt or data chunk", corpus["dup"]: "same file stem",
           names.index("k_exists.wav"): "already exists"}
    for i, r in enumerate(rep):
        if i in bad:
            assert r["status"] != 0 and bad[i] in r["message"], (i, r)
        else:
            assert r["status"] == 0 and r["message"] == "", (i, r)
    # 11 files written, each with both outputs, and the file that was there first untouched
    assert len(listing) == 2 * 11 + 1 and listing[corpus["exists"] + "_basic_pitch.mid"] == b"was here first"
    zero = rep[names.index("h_zero.wav")]
    assert (zero["n_frames"], zero["n_note_events"]) == (0, 0)
    assert listing["h_zero_basic_pitch.csv"] == b"start_time_s,end_time_s,pitch_midi,velocity,pitch_bend\r\n"
    short = [r for i, r in enumerate(rep) if i not in bad and names[i] not in ("h_zero.wav", "e_long_16w.wav")]
    assert all(r["n_note_events"] > 0 for r in short), [r["n_note_events"] for r in short]  # the batches have notes to get right


def test_batches_of_four_write_the_same_bytes(model, corpus, per_file, announced, outs):
    """14 files in runs of four: several batches, the last one partial, every group call with one to three clips."""
    got = _run(model, corpus, outs, threads=2, clip_batch=4)
    _same(got, per_file)
    assert announced == 10 and got[2] == announced


@pytest.mark.parametrize("direct_io", [False, True])
def test_one_batch_holds_everything_with_two_lanes_and_three_threads(model, corpus, per_file, announced, outs, direct_io):
    from basic_pitch_amd import Model

    other = Model(max_windows=32)
    try:
        got = _run(model, corpus, outs, models=[model, other], threads=3, clip_batch=64, direct_io=direct_io)
    finally:
        other.close()
    _same(got, per_file)
    assert got[2] == announced


def test_an_onset_threshold_of_zero_leaves_every_file_to_the_per_file_route(model, corpus, outs):
    """Every clip of a clips call has status 1 with such a threshold (the host decodes the maps themselves): nothing is
    batched, and the job is the per-file job."""
    want = _run(model, corpus, outs, threads=2, onset_threshold=0.0)
    got = _run(model, corpus, outs, threads=2, onset_threshold=0.0, clip_batch=4)
    _same(got, want)
    assert want[2] == 0 and got[2] == 0
    assert sum(r["status"] == 0 for r in want[1]) == 11


def test_a_file_with_a_nan_among_normal_files(model, corpus, outs, tmp_path):
    """A float32 file with one NaN sample among normal files: the same bytes and reports as the per-file route, whichever
    route the file ends on (a clip whose maps hold a NaN has status 1 and falls back alone; one whose maps hold none is
    decoded in the batch, as the per-file route's candidates call decodes it), and no file is counted twice."""
    x = CF.tones(30000, 1, 22050, 13)
    x[12345, 0] = np.nan
    nan = CF.write_wav(tmp_path / "n_nan.wav", x, "f32", 22050)
    paths = corpus["paths"][:3] + [nan] + corpus["paths"][3:]
    want = _run(model, corpus, outs, paths=paths, threads=2)
    got = _run(model, corpus, outs, paths=paths, threads=2, clip_batch=4)
    _same(got, want)
    assert want[2] == 0 and got[2] <= len(paths)


def test_a_flac_clip_the_device_decoder_fails_on_falls_back_alone(model, corpus, announced, outs, tmp_path):
    """A FLAC file with a flipped bit in its last frame: the probe announces a batched FLAC call (the headers are sound), the
    call gives the clip BP_CLIP_FLAC_FAILED (a CRC-16 mismatch) and the per-file route reports the file as it does today;
    the files batched with it come from the batched calls, all of them."""
    from basic_pitch_amd import _native

    blob = bytearray(open(corpus["paths"][2], "rb").read())
    blob[-40] ^= 0x10
    bad = tmp_path / "o_flipped.flac"
    bad.write_bytes(bytes(blob))
    paths = corpus["paths"][:2] + [str(bad)] + corpus["paths"][2:]
    lib = model._lib
    rc, routes = CF.probe(lib, paths, CF.params(lib, 4), handles=[model._handle])
    assert rc == 0 and routes[2] == 2
    want = _run(model, corpus, outs, paths=paths, threads=2)
    got = _run(model, corpus, outs, paths=paths, threads=2, clip_batch=4)
    _same(got, want)
    assert want[1][2]["status"] == _native.BP_ERR_BAD_AUDIO and "o_flipped_basic_pitch.mid" not in want[0]
    assert want[2] == 0 and got[2] == announced


def test_a_rate_the_clips_calls_refuse_sends_its_group_back(model, corpus, announced, outs, tmp_path):
    """Two files at 44,101 Hz, a ratio whose filter is not tabulated: the probe announces them (it reads headers, not filter
    tables), their call answers BP_ERR_UNSUPPORTED as a whole, and the per-file route — which evaluates such a filter in
    the kernel — writes them.  The other groups of the same runs are not concerned."""
    odd = [CF.write_wav(tmp_path / f"p_odd{i}.wav", CF.tones(30000 + 7000 * i, 1 + i, 44101, 14 + i), "s16", 44101) for i in range(2)]
    paths = corpus["paths"][:1] + odd[:1] + corpus["paths"][1:6] + odd[1:] + corpus["paths"][6:]
    lib = model._lib
    rc, routes = CF.probe(lib, paths, CF.params(lib, 4), handles=[model._handle])
    assert rc == 0 and routes[1] == 1 and routes[7] == 1
    want = _run(model, corpus, outs, paths=paths, threads=2)
    got = _run(model, corpus, outs, paths=paths, threads=2, clip_batch=4)
    _same(got, want)
    assert want[1][1]["status"] == 0 and want[1][7]["status"] == 0 and want[1][1]["n_note_events"] > 0
    assert want[2] == 0 and got[2] == announced
