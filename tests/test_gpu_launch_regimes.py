"""Every launch regime of the dense path gives the small-batch bits.

Each launcher of the default path picks its kernel, grid, chunking and work cut from the number of windows of a launch and
the device's CU count (csrc/launch_plan.h).  tests/launch_regimes.py lists, for this device, the batch sizes that enter
every regime and stand on both sides of every change (tests/test_launch_plan_cpu.py holds that list to the full
enumeration); here every one of them runs, in each of the three modes, and EVERY window of every call must equal, bit for
bit, what a handle of `max_windows = 8` computes for it — the handle the suite treats as the small-batch truth, tied to the
fp64 oracle below by four probe windows under test_gpu_parity's noise-aware bound.

The handle's device buffers outlive a call, so a kernel that fails to write a window would pass any test that sends the
same batch twice: the stale value is the right one.  Every call therefore takes its windows from another offset of the
pool (a step coprime to 16), with a silent window at position 0 and a tone at position n - 1 — on the ragged conv2 group,
the one-window second launch, the last filterbank workgroup.

The stage tests run pyramid, contour, note and onset alone (bp_run_stage) at the sizes where that stage's own decisions
change, against the same stage in calls of at most 8 windows: a whole-path failure is then one kernel's, and the CNN
kernels see inputs over their whole range rather than what real posteriorgrams cover.

No number here is a measured tolerance: equality, or the existing bound for the four probes."""
import numpy as np
import pytest
import torch

import launch_regimes as L
from oracle import bp_oracle as O

pytestmark = pytest.mark.gpu

F32 = torch.float32
KEYS = ("note", "onset", "contour")
STEP = 37  # pool offset step from call to call: coprime to 16 and to every pool size used here (checked below)


def _device_cus():
    """compute units of device 0: the list of sizes is this device's (256 where nothing is visible: the cases are skipped)"""
    try:
        if torch.cuda.is_available():
            return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        pass
    return 256


N_CU = _device_cus()
WHOLE = [(mode, n) for mode in L.MODES for n in L.sizes(N_CU, mode)]
STAGES = [(stage, mode, n) for mode, stages in (("default", ("pyramid", "contour", "note", "onset")), ("ext_cqt_44k", ("pyramid", "contour")))
          for stage in stages for n in L.stage_sizes(stage, N_CU, mode)]
STAGE_WIDTH = {"contour": 264, "note": 88, "onset": 88}


def _kind(i):
    """what pool entry i holds: most are noise; every 16th a tone plus noise, every 37th silent, every 41st quiet noise"""
    return "silent" if i % 37 == 0 else "quiet" if i % 41 == 0 else "tone" if i % 16 == 0 else "noise"


def _make_pool(n, n_samples, rate, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, n_samples), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
    t = np.arange(n_samples) / rate
    for i in range(n):
        k = _kind(i)
        if k == "silent":
            x[i] = 0.0
        elif k == "quiet":
            x[i] *= np.float32(0.01)
        elif k == "tone":
            f0 = 110.0 * 2 ** (int(rng.integers(0, 48)) / 12.0)
            x[i] = (0.5 * np.sin(2 * np.pi * f0 * t) + 0.01 * x[i]).astype(np.float32)
    return x


def _call_indices(n, k, pool_n):
    """pool entries of the k-th call's n windows: a run from offset STEP k (cyclic), then a silent entry swapped to
    position 0 and a tone to position n - 1 (n = 1: one of the two)"""
    idx = (STEP * k + np.arange(n)) % pool_n
    silent = [i for i in range(pool_n) if _kind(i) == "silent"]
    tone = [i for i in range(pool_n) if _kind(i) == "tone"]
    want = [(0, silent[k % len(silent)]), (n - 1, tone[k % len(tone)])]
    if n == 1:
        want = want[k % 2 : k % 2 + 1]
    for pos, entry in want:
        at = np.flatnonzero(idx == entry)
        if at.size:
            idx[at[0]] = idx[pos]
        idx[pos] = entry
    return idx


def _first_difference(got, ref):
    """(window, frame) of the first cell whose bits differ"""
    bad = np.argwhere(got.view(np.uint32).reshape(got.shape[0], got.shape[1], -1) != ref.view(np.uint32).reshape(ref.shape[0], ref.shape[1], -1))
    return (int(bad[0][0]), int(bad[0][1]), int(len(np.unique(bad[:, 0]))))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Ctx:
    """one mode: the pool, its small-batch reference, the big handle; stage pools and references as they are first asked for"""

    def __init__(self, mode, pool=None):
        from basic_pitch_amd import Model

        self.mode = mode
        self.ext = mode == "ext_cqt_44k"
        self.n_samples = O.EXT_AUDIO_N_SAMPLES if self.ext else O.AUDIO_N_SAMPLES
        self.pool_n = L.largest(N_CU)
        assert np.gcd(STEP, 16) == 1 and np.gcd(STEP, self.pool_n) == 1
        self.pool = pool if pool is not None else _make_pool(self.pool_n, self.n_samples, 44100.0 if self.ext else 22050.0, seed=101)
        small = Model(max_windows=8, **L.MODES[mode])
        self.ref = small.predict(self.pool)
        small.close()
        self._big = self._runner = None
        self._stage = {}

    def close(self):
        if self._big is not None:
            self._big.close()
        self._big = self._runner = None

    @property
    def big(self):
        """the handle that takes every size in one launch"""
        if self._big is None:
            from basic_pitch_amd import Model

            self._big = Model(max_windows=self.pool_n, **L.MODES[self.mode])
            assert self._big.info()["compute_units"] == N_CU
        return self._big

    @property
    def runner(self):
        if self._runner is None:
            from stage_harness import StageRunner

            self._runner = StageRunner(self.big)
        return self._runner

    # ---- stages: inputs that need no oracle, the expected result from calls of at most 8 windows
    def stage_io(self, stage, idx):
        """(inputs, outputs) of bp_run_stage for the pool entries idx"""
        n = len(idx)
        if stage == "pyramid":
            stride = (O.AUDIO_N_SAMPLES + 43712) if self.ext else 43712
            return {"audio": self.pool[idx]}, {"pyr": ((n, stride), F32)}
        pools = self.stage_pools(stage)
        ins = {k: v[idx] for k, v in pools.items()}
        return ins, {stage: ((n, 172, STAGE_WIDTH[stage]), F32)}

    def stage_pools(self, stage):
        key = ("pool", stage)
        if key not in self._stage:
            from stage_harness import zp_pack

            n = max(L.stage_sizes(stage, N_CU, self.mode)) + 5
            rng = np.random.default_rng({"contour": 7, "note": 8, "onset": 9}[stage])

            def edge_cases(a):
                """windows with a single non-zero frame (the very first, the very last) or a single non-zero bin in a
                corner: what a halo row read from the neighbouring window's memory would change"""
                for i in range(a.shape[0]):
                    if i % 7 == 3:
                        a[i, 1:] = 0
                    elif i % 7 == 5:
                        a[i, :-1] = 0
                    elif i % 7 == 6:
                        first, last = a[i, 0, 0], a[i, -1, -1]
                        a[i] = 0
                        a[i, 0, 0], a[i, -1, -1] = first, last
                return a

            pools = {}
            if stage in ("contour", "onset"):
                bn_a, bn_b = (np.float32(v) for v in O.load_weights()["bn_affine"][:2])
                z = rng.random((n, 172, 345 if self.ext else 309), dtype=np.float32) * bn_a + bn_b  # BatchNorm's output range
                pools["zp"] = zp_pack(edge_cases(z)).view(np.int32)
            if stage == "note":
                pools["contour"] = edge_cases(rng.random((n, 172, 264), dtype=np.float32))
            if stage == "onset":
                pools["note"] = edge_cases(np.roll(rng.random((n, 172, 88), dtype=np.float32), 2, axis=0))
            self._stage[key] = pools
        return self._stage[key]

    def stage_pool_n(self, stage):
        if stage == "pyramid":
            return self.pool_n
        return len(next(iter(self.stage_pools(stage).values())))

    def stage_ref(self, stage, idx):
        """the stage's result for pool entries idx, each computed once in a call of at most 8 windows"""
        key = ("ref", stage)
        have = self._stage.setdefault(key, {})
        need = [int(i) for i in dict.fromkeys(idx.tolist()) if int(i) not in have]
        for i0 in range(0, len(need), 8):
            part = np.asarray(need[i0 : i0 + 8])
            ins, outs = self.stage_io(stage, part)
            (got,) = self.runner.run(stage, len(part), ins, outs).values()
            for j, i in enumerate(part):
                have[int(i)] = got[j].copy()
        return np.stack([have[int(i)] for i in idx])


@pytest.fixture(scope="module")
def contexts():
    """the modes' contexts, made when first asked for and kept for the module (pool and reference once per mode)"""
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def ctx(request, contexts):
    """the context of the mode asked for; one big handle is alive at a time"""
    mode = request.param
    for m, c in contexts.items():
        if m != mode:
            c.close()
    if mode not in contexts:
        shared = contexts["default"].pool if mode == "bf16_weights" and "default" in contexts else None
        contexts[mode] = _Ctx(mode, shared)
    return contexts[mode]


@pytest.mark.parametrize("ctx", list(L.MODES), indirect=True)
def test_small_batch_reference_is_the_oracle_s(ctx, weights):
    """noise, tone, silent and quiet probe windows of the pool's reference against the fp64 oracle (bf16_weights: the same
    graph with bf16-rounded conv weights, as test_bf16_weights_mode) under test_gpu_parity's noise-aware bound"""
    from test_gpu_parity import _noise_aware

    probes = [next(i for i in range(1, ctx.pool_n) if _kind(i) == k) for k in ("noise", "tone", "silent", "quiet")]
    w = dict(weights)
    if ctx.mode == "bf16_weights":
        for k in ("contour1_w", "contour2_w", "note1_w", "note2_w", "onset1_w", "onset2_w"):
            u = np.ascontiguousarray(weights[k], dtype=np.float32).view(np.uint32).astype(np.uint64)
            w[k] = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    x = ctx.pool[probes]
    r64 = O.forward(x, w, np.float64, ext=ctx.ext)
    r32 = O.forward(x, w, np.float32, ext=ctx.ext)
    got = {k: ctx.ref[k][probes] for k in KEYS}
    for k in KEYS:
        assert np.isfinite(got[k]).all(), (ctx.mode, k)
        print(f"{ctx.mode} {k}: |ref - fp64| = {np.abs(got[k] - r64[k]).max():.3e}, |fp32 - fp64| = {np.abs(r32[k] - r64[k]).max():.3e}")
    _noise_aware(got, r32, r64)


@pytest.mark.parametrize("ctx,n", WHOLE, indirect=["ctx"])
def test_whole_path_gives_the_small_batch_bits_at_every_regime(ctx, n):
    k = L.sizes(N_CU, ctx.mode).index(n)
    idx = _call_indices(n, k, ctx.pool_n)
    assert _kind(idx[0]) == "silent" or n == 1
    assert _kind(idx[-1]) == "tone" or n == 1
    got = ctx.big.predict(ctx.pool[idx])
    for key in KEYS:
        a, ref = got[key], ctx.ref[key][idx]
        assert a.shape == ref.shape and a.dtype == np.float32
        assert np.isfinite(a).all(), f"{ctx.mode}, n = {n}, {key}: not finite; plan: {L.describe(n, N_CU, ctx.mode)}"
        if not _same_bits(a, ref):
            w, t, n_bad = _first_difference(a, ref)
            pytest.fail(f"{ctx.mode}, n = {n}, {key}: {n_bad} of {n} windows differ from the small-batch result, the first at "
                        f"window {w} (pool entry {idx[w]}, {_kind(idx[w])}), frame {t}; plan: {L.describe(n, N_CU, ctx.mode)}")


@pytest.mark.parametrize("stage,ctx,n", STAGES, indirect=["ctx"])
def test_stage_gives_the_small_batch_bits_at_its_own_seams(stage, ctx, n):
    sizes = L.stage_sizes(stage, N_CU, ctx.mode)
    pool_n = ctx.stage_pool_n(stage)
    assert np.gcd(STEP, pool_n) == 1 or pool_n > STEP * len(sizes) + n
    idx = (STEP * (1 + sizes.index(n)) + np.arange(n)) % pool_n
    ref = ctx.stage_ref(stage, idx)
    ins, outs = ctx.stage_io(stage, idx)
    (got,) = ctx.runner.run(stage, n, ins, outs).values()  # outputs pre-filled with NaN: an unwritten cell differs
    if stage != "pyramid":  # (the pyramid's rows have gaps between the levels that nobody writes)
        assert np.isfinite(got).all(), f"{stage}, {ctx.mode}, n = {n}: not finite; plan: {L.describe(n, N_CU, ctx.mode)}"
    if not _same_bits(got, ref):
        g3, r3 = (a.reshape(n, 1, -1) if a.ndim == 2 else a for a in (got, ref))
        w, t, n_bad = _first_difference(g3, r3)
        pytest.fail(f"{stage}, {ctx.mode}, n = {n}: {n_bad} of {n} windows differ from the stage's small-batch result, the first at "
                    f"window {w} (pool entry {idx[w]}), frame {t}; plan: {L.describe(n, N_CU, ctx.mode)}")
