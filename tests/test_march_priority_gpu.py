"""The marches' priority rule (csrc/march_common.h BP_MARCH_PRIO_*) moves no arithmetic: the posteriorgrams of the whole
path with the adopted rule and with BP_MARCH_PRIO=off (the A/B library's switch back to "no wave changes priority") are
bit-equal.  One process per setting (the switch is read once per process), through tools/experiments/march_prio_ab.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "march_prio_ab.py")


def _maps(tmp_path, n, *extra):
    """{rule: the tool's arrays} for the adopted rule and for `off`, both on the A/B library"""
    from basic_pitch_amd import build as B

    got = {}
    for rule in ("adopted", "off"):
        env = dict(os.environ)
        for k in ("BP_ONSET", "BP_NOTE", "BP_CONV1", "BP_CONV2", "BP_RIM", "BP_RESAMPLE", "BP_MARCH_PRIO"):
            env.pop(k, None)
        env["BASIC_PITCH_AMD_LIB"] = B.build_library(ab=True)
        if rule == "off":
            env["BP_MARCH_PRIO"] = "off"
        out = str(tmp_path / f"{rule}.npz")
        subprocess.run([sys.executable, TOOL, out, str(n), *extra], check=True, env=env, timeout=600)
        got[rule] = np.load(out)
    return got


def _assert_bit_equal(got, n):
    for k, width in (("note", 88), ("onset", 88), ("contour", 264)):
        a, b = got["adopted"][k], got["off"][k]
        assert a.shape == b.shape == (n, 172, width), (k, a.shape, b.shape)
        assert np.isfinite(a).all(), k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def test_one_window_most_waves_have_no_piece(tmp_path):
    """1 window: a few waves march, the others have no piece — a wave without work neither flips nor hangs."""
    _assert_bit_equal(_maps(tmp_path, 1), 1)


def test_five_windows_end_to_end_cut(tmp_path):
    """5 windows: the end-to-end cut, shares that span (window, strip) pairs, one resident half of the grid."""
    _assert_bit_equal(_maps(tmp_path, 5), 5)


def test_one_window_per_compute_unit_both_halves_resident(tmp_path):
    """n_cu windows: the smallest batch that takes the aligned cut with both halves of the grid resident — the only regime
    in which a wave changes its priority."""
    got = _maps(tmp_path, "ncu")
    n = int(got["adopted"]["n_cu"])
    assert n == int(got["off"]["n_cu"]) and n >= 8
    _assert_bit_equal(got, n)


def test_five_windows_bf16_weights(tmp_path):
    """5 windows on a bf16_weights handle: the kernels' instantiations without weight lo parts."""
    _assert_bit_equal(_maps(tmp_path, 5, "--bf16-weights"), 5)
