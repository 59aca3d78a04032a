"""The cut of a march's frames into per-wave pieces (csrc/march_common.h: BP_MARCH_SHARES_TAKE, the text the note and the
onset march expand in their piece loops), enumerated on the host through MarchShares by tests/march_shares_enum.hip.

On the device the `aligned` branch runs only when there are exactly 8 waves per window, i.e. at a full batch on a chip whose
resident waves number 8 x the batch, so a wrong cut would show in no small GPU test.  Here every wave count is just a
number: for n_windows in {1, 2, 3, 5, 256} and total_waves in {4, 8, 12, 64, 8 n_windows, 2048}, and for both kernels'
cuts (note 68 | 133 | 151, onset 64 | 129 | 150), with 3 strips per window and 172 frames per strip:
  1. the pieces of all waves cover every (window, strip, frame) exactly once;
  2. every piece has 0 <= T0 < T1 <= 172 and lies inside one (window, strip);
  3. with 8 waves per window no wave gets more than two pieces.
The program is built once more with the host sanitizers (address, undefined) and must run clean and print the same."""
import os
import subprocess

import numpy as np
import pytest

from basic_pitch_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "march_shares_enum.hip")
FRAMES, STRIPS = 172, 3
WINDOWS = (1, 2, 3, 5, 256)


def _wave_counts(n):
    return sorted({4, 8, 12, 64, 8 * n, 2048})


def _build(out, extra):
    cmd = [build.find_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-I" + build.CSRC] + extra + [SRC, "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]  # -fno-sanitize-recover: a finding ends the sanitizer build's run
    return res.stdout


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    """rows (cuts, n_windows, total_waves, wave, ws, T0, T1) of the plain build; the sanitizer build must print the same"""
    d = tmp_path_factory.mktemp("march_shares")
    plain, san = str(d / "enum"), str(d / "enum_san")
    _build(plain, [])
    _build(san, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    syms = subprocess.run(["nm", san], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
    out = _run(plain)
    assert _run(san) == out
    return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)


def _cases():
    return [(c, n, tw) for c in (0, 1) for n in WINDOWS for tw in _wave_counts(n)]


def test_the_program_enumerates_every_case(pieces):
    seen = {tuple(r) for r in np.unique(pieces[:, :3], axis=0).tolist()}
    assert seen == set(_cases())


@pytest.mark.parametrize("cuts,n_windows,total_waves", _cases())
def test_pieces_partition_the_frames_of_every_window_and_strip(pieces, cuts, n_windows, total_waves):
    p = pieces[(pieces[:, 0] == cuts) & (pieces[:, 1] == n_windows) & (pieces[:, 2] == total_waves)]
    wave, ws, t0, t1 = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    n_ws = STRIPS * n_windows
    # 2. every piece is a non-empty frame range of one existing (window, strip), handed to an existing wave
    assert np.all((0 <= wave) & (wave < total_waves))
    assert np.all((0 <= ws) & (ws < n_ws))
    assert np.all((0 <= t0) & (t0 < t1) & (t1 <= FRAMES))
    # 1. exactly once: +1 at every piece's first frame, -1 behind its last; the running sum is the cover count
    edge = np.zeros(n_ws * FRAMES + 1, dtype=np.int64)
    np.add.at(edge, ws * FRAMES + t0, 1)
    np.add.at(edge, ws * FRAMES + t1, -1)
    cover = np.cumsum(edge)[:-1]
    assert cover.min() == 1 and cover.max() == 1, (int(cover.min()), int(cover.max()), int(np.argmax(cover != 1)))
    # 3. the aligned cut: at most two marches per wave (and every wave has work)
    if total_waves == 8 * n_windows:
        per_wave = np.bincount(wave, minlength=total_waves)
        assert per_wave.min() >= 1 and per_wave.max() <= 2, (int(per_wave.min()), int(per_wave.max()))
