"""The CNN kernels and the host weight packing (csrc/weight_pack.hip) against the oracle on OTHER weights of the same
architecture: the families of tests/weight_families.py, in which every tap is far from zero (a dropped, duplicated or
misplaced tap is >= 215 x the gate: tests/test_weight_families_cpu.py), bn_affine has either sign, activations are up to
eight times the shipped model's, or all conv weights are zero.  The stage tests feed each stage the family's fp32-oracle
input and compare with the fp64 evaluation of that stage on the same input, at the project's gates for the shipped
weights (5e-6 branches, 2e-6 zpack); the measured levels are in profiles/r07_other_weights.md.  -s prints them."""
import numpy as np
import pytest
import torch

import weight_families as WF
from oracle import bp_oracle as O

pytestmark = pytest.mark.gpu

F32 = torch.float32
KEYS = ("note", "onset", "contour")


class Fam:
    """one family (admitted by tests/test_weight_families_cpu.py::test_admission): its tensors, blob, oracles on the five windows, and an 8-window handle with a stage runner"""

    def __init__(self, name, tmp_dir, x, ext=False, **model_kw):
        from basic_pitch_amd import Model
        from stage_harness import StageRunner

        self.name, self.x, self.ext = name, x, ext
        self.W = WF.family(name)
        self.blob = WF.blob_path(tmp_dir, self.W, f"{name}.bin")
        self.r32 = O.forward(x, self.W, np.float32, intermediates=True, ext=ext)
        self.r64 = O.forward(x.astype(np.float64), self.W, np.float64, intermediates=True, ext=ext)
        self.refs = WF.stage_refs(self.W, self.r32)
        self.model = Model(self.blob, max_windows=8, ext_cqt_44k=ext, **model_kw)
        self.runner = StageRunner(self.model)

    def feed(self, stage):
        from stage_harness import ord_encode, zp_pack

        r32 = self.r32
        if stage == "zpack":
            return {"lp": r32["lp"], "mm": ord_encode(r32["minmax"])}
        if stage == "note":
            return {"contour": r32["contour"]}
        zp = zp_pack(r32["z"]).view(np.int32)  # 309 bins, or the extended mode's 345: the same row layout
        return {"zp": zp} if stage == "contour" else {"zp": zp, "note": r32["note"]}

    def run_branch(self, stage):
        n = self.x.shape[0]
        width = 264 if stage == "contour" else 88
        return self.runner.run(stage, n, self.feed(stage), {stage: ((n, 172, width), F32)})[stage]


@pytest.fixture(scope="module", params=list(WF.FAMILIES))
def fam(request, tmp_path_factory):
    f = Fam(request.param, tmp_path_factory.mktemp(request.param), WF.windows())
    yield f
    f.model.close()


def _report(tag, stage, got, f):
    hip = float(np.abs(got - f.refs["f64"][stage]).max())
    orc = float(np.abs(f.refs["f32"][stage] - f.refs["f64"][stage]).max())
    print(f"{tag} {stage}: |hip - fp64| = {hip:.2e}, |torch fp32 - fp64| = {orc:.2e} (same fp32 input)")
    return hip


@pytest.mark.parametrize("stage", ["contour", "note", "onset"])
def test_fused_branch_on_other_weights(fam, stage):
    """test_stage_fused_branch under every admitted family, against fp64 on the same fp32 input: 5e-6."""
    got = fam.run_branch(stage)
    assert np.isfinite(got).all()
    hip = _report(fam.name, stage, got, fam)
    assert hip <= WF.BRANCH_GATE, (fam.name, stage, hip)


def test_zpack_on_other_weights(fam):
    """test_stage_zpack with bn_affine of either sign: 2e-6 (|bn_a| <= 3.1: z in fp32 carries <= 2 ulp of 3.1 = 4.8e-7 of
    rounding, the split 2^-22 |z|), and the zero padding of the tensor."""
    from stage_harness import zp_unpack

    n = fam.x.shape[0]
    zp = fam.runner.run("zpack", n, fam.feed("zpack"), {"zp": ((n, 174, 448), torch.int32)})["zp"].view(np.uint32)
    pad = zp.copy()
    pad[:, 1:173, 56 : 56 + 309] = 0
    assert (pad == 0).all()
    hip = _report(fam.name, "zpack", zp_unpack(zp), fam)
    assert hip <= WF.ZPACK_GATE, (fam.name, hip)


@pytest.mark.parametrize(
    "stage,ins,outs,key,tol",
    [
        ("contour1", ("lp", "mm"), {"c1": (8, 172, 264)}, "c1", 5e-5),
        ("contour2", ("c1",), {"contour": (172, 264)}, "contour", 2e-6),
        ("note1", ("contour",), {"n1": (32, 172, 88)}, "n1", 5e-6),
        ("note2", ("n1",), {"note": (172, 88)}, "note", 2e-6),
        ("onset1", ("lp", "mm"), {"o1": (32, 172, 88)}, "o1", 2e-4),
        ("onset2", ("note", "o1"), {"onset": (172, 88)}, "onset", 2e-6),
    ],
)
def test_exact_f32_stage_chain_on_other_weights(fam, stage, ins, outs, key, tol):
    """test_stage_cnn (the exact-f32 kernels: pack_contour1, pack_onset1, pack_note1 and the plain tables) under every
    family, at its tolerances."""
    from stage_harness import ord_encode

    r32 = fam.r32
    n = fam.x.shape[0]
    feed = {k: ord_encode(r32["minmax"]) if k == "mm" else r32[k] for k in ins}
    got = fam.runner.run(stage, n, feed, {k: ((n,) + s, F32) for k, s in outs.items()})[key]
    assert np.isfinite(got).all()
    d = np.abs(got - r32[key]).max()
    scale = max(1.0, float(np.abs(r32[key]).max()))
    print(f"{fam.name} {stage}: |hip - fp32 oracle| = {d:.2e}, bound {tol * scale:.2e}")
    assert d <= tol * scale, (fam.name, stage, d)


def _silence_chain(runner, zp):
    contour = runner.run("contour", 1, {"zp": zp}, {"contour": ((1, 172, 264), F32)})["contour"]
    note = runner.run("note", 1, {"contour": contour}, {"note": ((1, 172, 88), F32)})["note"]
    onset = runner.run("onset", 1, {"zp": zp, "note": note}, {"onset": ((1, 172, 88), F32)})["onset"]
    return {"contour": contour, "note": note, "onset": onset}


def test_whole_path_on_other_weights(fam):
    """predict on the five windows against the family's fp64 / fp32 oracles with the noise-aware bound; the silent window
    bit for bit the handle's own stage chain on the constant map z = bn_b (this family's bn_b)."""
    from stage_harness import zp_pack
    from test_gpu_parity import _noise_aware

    got = fam.model.predict(fam.x)
    for k in KEYS:
        assert np.isfinite(got[k]).all()
        print(f"{fam.name} whole path {k}: |hip - fp64| = {np.abs(got[k] - fam.r64[k]).max():.2e}, "
              f"|fp32 oracle - fp64| = {np.abs(fam.r32[k] - fam.r64[k]).max():.2e}")
    _noise_aware(got, fam.r32, fam.r64)
    bn_b = np.float32(fam.W["bn_affine"][1])
    want = _silence_chain(fam.runner, zp_pack(np.full((1, 172, 309), bn_b, np.float32)).view(np.int32))
    for k in KEYS:
        assert np.array_equal(got[k][4], want[k][0]), (fam.name, k, float(np.abs(got[k][4] - want[k][0]).max()))


def test_fused_batch_equals_the_small_handle(tmp_path):
    """A handle with a window for every second CU takes the fused filterbank + normalise path, which folds bn_a / range
    (here with a negative bn_a): the same bits as the 8-window handle."""
    from basic_pitch_amd import Model

    W = WF.family(WF.MODE_FAMILY)
    blob = WF.blob_path(tmp_path, W)
    x = WF.windows()
    n = torch.cuda.get_device_properties(0).multi_processor_count // 2 + 2
    xs = np.concatenate([x] * (n // 5 + 1))[:n]
    small = Model(blob, max_windows=8)
    a = small.predict(x)
    small.close()
    big = Model(blob, max_windows=n)
    b = big.predict(xs)
    big.close()
    for k in KEYS:
        for i in range(n):
            assert np.array_equal(b[k][i], a[k][i % 5]), (k, i)


def test_bf16_mode_on_other_weights(tmp_path):
    """bf16_weights=True, stage by stage at the branch gate, against the fp64 oracle of the family with its conv weights
    rounded to bf16 by test_bf16_weights_mode's rounding."""
    f = Fam(WF.MODE_FAMILY, tmp_path, WF.windows(), bf16_weights=True)
    try:
        Wq = WF.bf16_weights(f.W)
        f.r32 = O.forward(f.x, Wq, np.float32, intermediates=True)
        f.refs = WF.stage_refs(Wq, f.r32)
        for stage in ("contour", "note", "onset"):
            got = f.run_branch(stage)
            hip = _report(f.name + " bf16", stage, got, f)
            assert hip <= WF.BRANCH_GATE, (stage, hip)
    finally:
        f.model.close()


def test_extended_mode_on_other_weights(tmp_path):
    """ext_cqt_44k=True: the contour and onset stages on a 345-bin z (the rim matrix in its 160-bin geometry, which nothing
    else reaches with non-shipped weights) against O.forward(..., ext=True), and the whole path."""
    from test_gpu_parity import _noise_aware

    f = Fam(WF.MODE_FAMILY, tmp_path, WF.windows_ext(), ext=True)
    try:
        assert f.r32["z"].shape[2] == 345
        for stage in ("contour", "onset"):
            got = f.run_branch(stage)
            hip = _report(f.name + " ext", stage, got, f)
            assert hip <= WF.BRANCH_GATE, (stage, hip)
        _noise_aware(f.model.predict(f.x), f.r32, f.r64)
    finally:
        f.model.close()


@pytest.mark.parametrize("mode", ["default", "bf16_weights", "ext_cqt_44k"])
def test_zero_family_is_sigmoid_of_the_bias_everywhere(tmp_path, mode):
    """All six conv weight tensors zero: every element of the three maps is sigmoid(b2) to 1e-6, rims and first / last
    frames included — anything read from a zero-padded K row, an unused register or uninitialised LDS shows here."""
    from basic_pitch_amd import Model

    W = WF.zero()
    ext = mode == "ext_cqt_44k"
    m = Model(WF.blob_path(tmp_path, W), max_windows=8, **({} if mode == "default" else {mode: True}))
    got = m.predict(WF.windows_ext() if ext else WF.windows())
    m.close()
    for k, b in (("contour", "contour2_b"), ("note", "note2_b"), ("onset", "onset2_b")):
        want = 1.0 / (1.0 + np.exp(-float(W[b][0])))
        d = np.abs(got[k].astype(np.float64) - want).max()
        assert d <= 1e-6, (mode, k, d)
