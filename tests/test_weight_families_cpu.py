"""The model families of tests/weight_families.py on the CPU: they are admitted (GPU stage tests may use them), a
single wrong tap in any of them is far outside the GPU gates (so such tests can fail), the C restatement
of the graph agrees with the torch oracle on them, and bp_create refuses weights outside the domain of its f16 operands.
No GPU: pack_weights runs before bp_create looks for a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import weight_families as WF
from conftest import ROOT
from oracle import bp_oracle as O

BOUNDED = [f"bounded{s}" for s in WF.BOUNDED_SEEDS]
BRANCH_OF = {"contour1_w": "contour", "contour2_w": "contour", "note1_w": "note", "note2_w": "note",
             "onset1_w": "onset", "onset2_w": "onset"}


@pytest.fixture(scope="module")
def x22():
    return WF.windows()


def _show(name, r):
    print(f"{name}: (a) in [0.02, 0.98] {r['a']}  (b) positive fraction min / max {r['b']}  (c) |fp32 - fp64| {r['c']}  "
          f"(d) max |.| {r['d']}")


@pytest.mark.parametrize("name", list(WF.FAMILIES))
def test_admission(x22, name):
    """Conditions (a) - (d) of weight_families.admission on the five 22.05 kHz windows, for every family the GPU tests
    use.  Measured: (a) >= 0.98, (b) every channel positive on 0.109 .. 0.897 of its positions, (c) contour <= 4.0e-7,
    note <= 1.1e-7, onset <= 1.1e-6 (half gate 2.5e-6), zpack <= 4.4e-7 (half gate 1e-6), (d) <= 16.2 (scaled: 103.4; the
    limit is 8188).  The scaled family meets (c) at factor 8."""
    r = WF.admission(WF.family(name), x22)
    _show(name, r)
    assert r["ok"], r


def test_admission_of_the_mode_family():
    """The one family of the extended-CQT and bf16 runs: admitted on the 44.1 kHz windows through the 345-bin CQT, and
    with its conv weights rounded to bf16 (the graph the bf16 mode is compared with)."""
    W = WF.family(WF.MODE_FAMILY)
    r = WF.admission(W, WF.windows_ext(), ext=True)
    _show(WF.MODE_FAMILY + " ext", r)
    assert r["ok"], r
    r = WF.admission(WF.bf16_weights(W), WF.windows())
    _show(WF.MODE_FAMILY + " bf16", r)
    assert r["ok"], r


def test_plain_draws_are_not_admitted(x22):
    """Why the conv1 layers are drawn channel by channel (which makes (b) of test_admission hold by construction, with the
    generator's margin): the shipped model itself, and a shuffle of its values within each tensor (the issue's `permuted`
    family: seeds 0 .. 3), leave hidden channels that never fire or always fire on these windows, where a dropped tap
    cannot show."""
    base = O.load_weights()
    rng = np.random.default_rng(1)
    shuffled = {k: (rng.permutation(v.ravel()).reshape(v.shape) if k.split("_")[0] in WF.CONV else v) for k, v in base.items()}
    for name, W in (("shipped", base), ("shuffled", shuffled)):
        r = WF.admission(W, x22)
        _show(name, r)
        assert not r["ok"] and min(lo for lo, _ in r["b"].values()) < 0.05


def _taps(key, w):
    """(label, index, bins) of the taps to zero: `bins` restricts where the change is measured (None: everywhere)"""
    a = np.abs(w)
    taps = [("smallest", np.unravel_index(a.argmin(), a.shape), None)]
    if key == "contour1_w":
        c0, c7 = a[:, 0, :, 0], a[:, 7, :, 38]
        # the only contributors to the folded kernel's ends: g = 0 - 19 - 36 = -55 and g = 38 - 19 + 101 = 120
        o, dt = np.unravel_index(c0.argmin(), c0.shape)
        taps.append(("fold g=-55", (o, 0, dt, 0), None))
        o, dt = np.unravel_index(c7.argmin(), c7.shape)
        taps.append(("fold g=120", (o, 7, dt, 38), None))
        # seen through the rim only: the change on the 40 bins that the position-dependent rim matrices compute
        o, c, dt, df = np.unravel_index(a.argmin(), a.shape)
        taps.append(("rim bins only", (o, c, dt, df), np.r_[0:20, 244:264]))
    return taps


@pytest.mark.parametrize("name", BOUNDED)
def test_a_single_zeroed_tap_is_far_outside_the_gpu_gate(x22, name):
    """The power the shipped model lacks: in each bounded family, for each of the six conv tensors, zeroing ONE tap — the
    smallest of the tensor; for contour1_w also the smallest of the taps that alone make up the folded kernel's ends
    g = -55 and g = 120, and the smallest tap seen on the rim bins only (f < 20, f >= 244: the position-dependent rim
    matrices) — moves the fp64 output of its branch (fed the fp32 oracle's stage input, as the GPU stage tests are) by at
    least 20 x the 5e-6 gate.  Smallest ratio measured over the three families: 215 (the smallest contour1_w tap of
    bounded4, on the rim bins; per family 244 / 215 / 363)."""
    W = WF.family(name)
    r32 = O.forward(x22, W, np.float32, intermediates=True)
    feeds = {"contour": dict(z=r32["z"]), "note": dict(contour=r32["contour"]), "onset": dict(z=r32["z"], note=r32["note"])}
    base = {b: WF.stage(b, W, np.float64, **feeds[b]) for b in feeds}
    worst = None
    for key, branch in BRANCH_OF.items():
        for label, idx, bins in _taps(key, W[key]):
            M = dict(W)
            M[key] = W[key].copy()
            M[key][idx] = 0.0
            d = np.abs(WF.stage(branch, M, np.float64, **feeds[branch]) - base[branch])
            ratio = float((d if bins is None else d[..., bins]).max()) / WF.BRANCH_GATE
            print(f"{name} {key}{list(map(int, idx))} ({label}, |w| = {abs(float(W[key][idx])):.3g}): {ratio:.0f} x gate")
            worst = ratio if worst is None else min(worst, ratio)
            assert ratio >= 20.0, (name, key, label, ratio)
    print(f"{name}: smallest ratio {worst:.0f}")


@pytest.mark.parametrize("name", list(WF.FAMILIES) + ["zero"])
def test_c_restatement_agrees_with_torch_oracle_on_the_family(x22, tmp_path, name):
    """oracle/bp_oracle.c reads the family's blob: a second, independent reference under the new weights, at the
    tolerance and on the windows (2 uniform, 1 normal; + the silent one) test_oracle_golden.py holds it to under the shipped
    ones.  Measured |C - torch fp32|: <= 4.6e-5 (onset of the scaled family; its torch fp32 is 8.7e-5 from fp64 there: the
    two CQTs differ by 2e-4 in z and these weights pass more of that on than the shipped ones).  The tonal window is left to
    test_gpu_other_weights.py::test_whole_path_on_other_weights' noise-aware bound: its z is 3.7e-3 apart between any two
    fp32 evaluations."""
    import os

    x22 = x22[[0, 1, 2, 4]]

    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    W = WF.family(name)
    r32 = O.forward(x22, W, np.float32)
    r64 = O.forward(x22, W, np.float64)
    rc = O.forward_c(x22, 4, weights_path=WF.blob_path(tmp_path, W))
    for k in ("note", "onset", "contour"):
        assert rc[k].shape == r32[k].shape
        assert np.abs(rc[k] - r32[k]).max() <= 5e-5, (name, k)
        assert np.abs(rc[k] - r64[k]).max() <= 2 * np.abs(r32[k] - r64[k]).max() + 2e-5, (name, k)


def test_zero_family_is_the_constant_map(x22):
    W = WF.zero()
    r = O.forward(x22, W, np.float64)
    for k, b in (("contour", "contour2_b"), ("note", "note2_b"), ("onset", "onset2_b")):
        assert np.abs(r[k] - 1.0 / (1.0 + np.exp(-float(W[b][0])))).max() <= 1e-12, k


# ---- bp_create's weight domain ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from basic_pitch_amd import _native, build

    build.build_library()
    return _native.load_library()


FLAGS = [0, 4, 8]  # default, BP_FLAG_BF16_WEIGHTS, BP_FLAG_EXT_CQT_44K (the 160-bin rim geometry): pack_weights' three paths


def _create(lib, tensors, flags=0):
    from basic_pitch_amd.weights import pack_blob

    blob = pack_blob(tensors)
    h = C.c_void_p()
    rc = lib.bp_create(blob, len(blob), 0, flags, 0, C.byref(h))
    msg = (lib.bp_last_error(None) or b"").decode()
    if rc == 0:
        lib.bp_destroy(h)
    return rc, msg


PAST_PACKING = (0, -3)  # BP_OK on a machine with an MI355X, BP_ERR_NO_DEVICE without: pack_weights let the blob through
BAD_WEIGHTS = -2


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("key", ["contour2_w", "note1_w", "note2_w"])
def test_create_refuses_weights_beyond_the_scaled_f16_operand(lib, key, flags):
    """The note and contour conv2 operands hold hi(w) x 2^11 in f16: |w| >= 31.98 is refused, 31.9 is packed."""
    W = WF.family(BOUNDED[0])
    W[key] = W[key].copy()
    W[key].flat[3] = 31.98
    rc, msg = _create(lib, W, flags)
    assert rc == BAD_WEIGHTS and "too large" in msg, (rc, msg)
    W[key].flat[3] = -31.9
    rc, msg = _create(lib, W, flags)
    assert rc in PAST_PACKING, (rc, msg)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("key", list(WF.CONV_W) + [c + "_b" for c in WF.CONV] + ["bn_affine"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_create_refuses_non_finite_weights(lib, key, bad, flags):
    """Without this check only the note and contour conv2 weights are looked at: a NaN or an infinity anywhere else is
    packed (f16 NaN / infinity operands, or an fp32 bias table) and every output of the branch comes back NaN."""
    W = WF.family(BOUNDED[0])
    W[key] = W[key].copy()
    W[key].flat[-1] = bad
    rc, msg = _create(lib, W, flags)
    assert rc == BAD_WEIGHTS and key in msg and "NaN or an infinity" in msg, (rc, msg)


@pytest.mark.parametrize("key", WF.CONV_W)
def test_create_refuses_a_weight_that_the_bf16_rounding_makes_infinite(lib, key):
    """3.4e38 is finite in fp32 and rounds to the bf16 infinity: refused with the tensor's name under BP_FLAG_BF16_WEIGHTS."""
    W = WF.family(BOUNDED[0])
    W[key] = W[key].copy()
    W[key].flat[0] = 3.4e38
    rc, msg = _create(lib, W, 4)
    assert rc == BAD_WEIGHTS and key in msg and "NaN or an infinity" in msg, (rc, msg)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("key,idx", [("contour1_w", (3, 2, 2, 30)), ("onset1_w", (31, 7, 4, 4)), ("onset2_w", (0, 5, 1, 1))])
def test_create_refuses_weights_whose_f16_hi_part_overflows(lib, key, idx, flags):
    """contour1_w and the onset weights are split as hi + lo / 2^11 with an unscaled hi: 65520 rounds to the f16 infinity
    (it is packed silently without the check), 65000 is representable; the message names the one tensor at fault.
    contour1_w is judged after the fold over the harmonic shifts: two taps of 40000 that meet in one z bin are refused,
    either alone is not.  onset2_w's taps of concat channel 0 (the note map) are an fp32 table: no limit there."""
    W = WF.family(BOUNDED[0])
    W[key] = W[key].copy()
    W[key][idx] = 65520.0
    rc, msg = _create(lib, W, flags)
    assert rc == BAD_WEIGHTS and key in msg and "too large" in msg, (rc, msg)
    assert sum(k in msg for k in WF.CONV_W) == 1, msg
    W[key][idx] = -65000.0
    rc, msg = _create(lib, W, flags)
    assert rc in PAST_PACKING, (rc, msg)
    if key == "contour1_w":
        W[key][idx] = 40000.0          # channel 2 (shift 36), df 30: z bin f + 47
        rc, msg = _create(lib, W, flags)
        assert rc in PAST_PACKING, (rc, msg)
        W[key][3, 3, 2, 9] = 40000.0   # channel 3 (shift 57), df 9: the same z bin
        rc, msg = _create(lib, W, flags)
        assert rc == BAD_WEIGHTS and "contour1_w" in msg, (rc, msg)
    if key == "onset2_w":
        W[key][idx] = 1.0
        W[key][0, 0, 1, 1] = 1e6       # the note-map channel
        rc, msg = _create(lib, W, flags)
        assert rc in PAST_PACKING, (rc, msg)
