"""Contour conv2 inside the conv1 march (conv_contour_march.hip FUSE + conv_contour2.hip contour_conv2_finish_kernel, the
default of the 309-bin path) against the unfused pair (BP_CONV2=unfused in the A/B library: the march writes c1,
contour_conv2_proj_kernel reads it).  Both multiply the same split operands; the fused path adds the 200 products of an
output in another order (per input pixel pair and tap class on the matrix cores, then across frame taps, positions and strips),
so the maps agree to fp32 accumulation-order noise: 2e-6 on a sigmoid output, the bound of the other A/B tests
(test_gpu_parity.py).  The bound is asserted on the whole map and, separately, where the fused path has a seam of its own:
the window's first and last frames, the rows around every cut between frame chunks, the columns around every strip seam
and around the rim.  Random z through the C ABI stage hook, one process per variant (the choice is read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import AB_WEIGHTS, _ab_args, _ab_env

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "experiments", "contour_ab.py")
BOUND = 2e-6


def _run(out, args, env):
    subprocess.run([sys.executable, TOOL, out] + args, check=True, env=env, timeout=600)
    return np.load(out)


def _chunk_starts(chunks):
    return [ci * 172 // chunks for ci in range(1, chunks)]


def _regions(chunks):
    """name -> (frame index, bin index) of the places where the fused path differs in kind from the unfused one"""
    all_t, all_f = np.arange(172), np.arange(264)
    seam_rows = np.unique(np.clip(np.concatenate([np.arange(t0 - 2, t0 + 2) for t0 in _chunk_starts(chunks)]), 0, 171))
    strip_cols = np.unique(np.clip(np.concatenate([np.arange(20 + 32 * s - 2, 20 + 32 * s + 2) for s in range(8)]), 0, 263))
    return {
        "first / last frames": (np.array([0, 1, 170, 171]), all_f),
        "chunk seams": (seam_rows, all_f),
        "strip seams": (all_t, strip_cols),
        "rim": (all_t, np.concatenate([np.arange(16, 24), np.arange(240, 248)])),
    }


@AB_WEIGHTS
@pytest.mark.parametrize("bf16", [False, True], ids=["split", "bf16_weights"])
@pytest.mark.parametrize("n,chunks", [(2, 32), (74, 4)])
def test_fused_equals_unfused(tmp_path, model, bf16, n, chunks):
    from basic_pitch_amd import _native

    plan = _native.bp_launch_plan_out()
    assert _native.load_library().bp_launch_plan(n, 256, 0, plan) == 0 and plan.conv2_fused == 1
    args = _ab_args(model, tmp_path) + ["--n", str(n)] + (["--bf16"] if bf16 else [])
    fused = _run(str(tmp_path / "fused.npy"), args, _ab_env())
    unfused = _run(str(tmp_path / "unfused.npy"), args, _ab_env(BP_CONV2="unfused"))
    assert fused.shape == unfused.shape == (n, 172, 264) and np.isfinite(fused).all()
    d = np.abs(fused - unfused)
    print(f"n = {n}: whole map max |fused - unfused| = {d.max():.3e}")
    worst = {name: float(d[:, t][:, :, f].max()) for name, (t, f) in _regions(chunks).items()}
    for name, v in worst.items():
        print(f"  {name}: {v:.3e}")
    assert d.max() <= BOUND, d.max()
    for name, v in worst.items():
        assert v <= BOUND, (name, v)


def test_window_0_is_the_same_bits_at_every_chunk_count(tmp_path):
    """1, 19, 37 and 74 windows are cut into 32, 16, 8 and 4 frame chunks (the sizes on either side of the plan's thresholds
    18 | 19, 36 | 37, 73 | 74 at 256 CUs): the same input gives window 0 the same bits."""
    from basic_pitch_amd import _native

    sizes = (1, 19, 37, 74)
    lib, plan, seen = _native.load_library(), _native.bp_launch_plan_out(), []
    for n in sizes:
        assert lib.bp_launch_plan(n, 256, 0, plan) == 0
        seen.append(plan.conv1_chunks)
    assert seen == [32, 16, 8, 4]
    got = _run(str(tmp_path / "w0.npy"), ["--window0", ",".join(map(str, sizes))], _ab_env())
    assert got.shape == (4, 172, 264) and np.isfinite(got).all()
    for k in range(1, 4):
        assert np.array_equal(got[0].view(np.uint32), got[k].view(np.uint32)), (sizes[k], float(np.abs(got[0] - got[k]).max()))
