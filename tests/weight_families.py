"""Other weights of the same architecture: seeded model families derived from the shipped tensors, the windows the
families are run on, the per-stage oracle (torch, fp32 or fp64, fed one stage's input) and the admission conditions.

Every parity test of the shipped model runs the kernels with one set of numbers, in which 4.7 % of the contour conv1
taps are below 1e-3: a tap that the packing drops, duplicates or reads from a neighbouring channel moves the output by
less than the 5e-6 gate there.  The families below make every tap count.  `Model(path)` and `O.forward(x, tensors)`
see the same float32 values (`blob_path` writes them with basic_pitch_amd.weights.pack_blob).  The CQT tensors
(`cqt_*`, `log_*`) stay as shipped: the filterbank is specialised to their support.

  bounded(seed)   every conv weight / bias tensor = rms(shipped tensor) x random sign x U(0.5, 1.5); bn_affine from
                  BN_AFFINES (scales of both signs).  The conv1 layers are drawn channel by channel and a channel that
                  is dead or always on on the test windows is redrawn (_live_conv1)
  scaled(seed)    bounded(seed) with every conv1 tensor x SCALED_FACTOR and every conv2 weight / SCALED_FACTOR: the same
                  logits from activations SCALED_FACTOR times larger (conv2 biases are added to the logit: unscaled)
  zero()          the six conv weight tensors 0, biases bounded: every output is sigmoid(b2) at every position
"""
from __future__ import annotations

import functools
import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from conftest import make_windows
from oracle import bp_oracle as O

CONV = ("contour1", "contour2", "note1", "note2", "onset1", "onset2")
CONV_W = tuple(c + "_w" for c in CONV)
BN_AFFINES = ((3.1, -1.4), (-1.9, 1.1), (2.2, -0.6))
SCALED_FACTOR = 8.0  # admission (c) holds at 8 (tests/test_weight_families_cpu.py): no halving was needed

# the gates of the GPU stage tests (tests/test_gpu_parity.py: test_stage_fused_branch, test_stage_zpack)
BRANCH_GATE = 5e-6
ZPACK_GATE = 2e-6
F16_MAX = 65504.0


def _rms(t: np.ndarray) -> float:
    return float(np.sqrt(np.mean(np.asarray(t, np.float64) ** 2)))


@functools.lru_cache(maxsize=None)
def _probe_norm():
    """the normalised log-power (before the BatchNorm affine) of the test windows, fp32: what the generators test a
    hidden channel's liveness on.  22.05 kHz windows first, then the extended mode's."""
    with torch.no_grad():
        W = O.load_weights()
        out = []
        for x, ext in ((windows(), False), (windows_ext(), True)):
            mag = O.cqt(O._t(x, np.float32), W, np.float32, ext=ext)
            out.append(O.normalized_log(mag, W, np.float32)[0])
    return tuple(out)


LIVE_LO, LIVE_HI = 0.08, 0.92  # the generators' margin inside admission (b)'s 5 % / 95 %


def _live(pre_sets) -> np.ndarray:
    """per candidate channel: positive on LIVE_LO .. LIVE_HI of its positions, on each set of windows"""
    ok = None
    for pre in pre_sets:
        frac = (pre > 0).float().mean(dim=(0, 2, 3)).numpy()
        good = (frac >= LIVE_LO) & (frac <= LIVE_HI)
        ok = good if ok is None else ok & good
    return ok


def _draw(rng, rms: float, shape) -> np.ndarray:
    sign = rng.integers(0, 2, shape) * 2.0 - 1.0
    return (rms * sign * rng.uniform(0.5, 1.5, shape)).astype(np.float32)


def _live_conv1(rng, w_ref: np.ndarray, b_ref: np.ndarray, conv, batch: int = 64, max_batches: int = 400):
    """A conv1 layer channel by channel: candidate channels (weights + bias, each element rms x sign x U(0.5, 1.5)) are
    drawn in batches and the first that are live on the test windows are kept.  An iid draw of the whole tensor never meets
    admission (b) on these windows (nor does the shipped model: most of its n1 channels are positive everywhere on
    noise): a channel's pre-activation is dominated by sum(w) x mean(input) + b.  Conditioning on liveness leaves every
    element in the stated form, no tap near zero."""
    n_out = w_ref.shape[0]
    rw, rb = _rms(w_ref), _rms(b_ref)
    ws, bs = [], []
    for _ in range(max_batches):
        w = _draw(rng, rw, (batch,) + w_ref.shape[1:])
        b = _draw(rng, rb, (batch,))
        ok = _live(conv(torch.from_numpy(w), torch.from_numpy(b)))
        ws.extend(w[ok]), bs.extend(b[ok])
        if len(ws) >= n_out:
            return np.stack(ws[:n_out]), np.asarray(bs[:n_out], np.float32)
    raise RuntimeError("no live channels found")


def bounded(seed: int, base: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    base = O.load_weights() if base is None else base
    rng = np.random.default_rng([seed, 0xB0])
    out = {k: v.copy() for k, v in base.items()}
    bn_a, bn_b = BN_AFFINES[seed % len(BN_AFFINES)]
    out["bn_affine"] = np.asarray([bn_a, bn_b], np.float32)
    for c in ("contour2", "note2", "onset2"):
        for k in (c + "_w", c + "_b"):
            out[k] = _draw(rng, _rms(base[k]), base[k].shape)
    t = lambda k: torch.from_numpy(out[k])  # noqa: E731
    with torch.no_grad():
        stacks = [O.harmonic_stack(n * np.float32(bn_a) + np.float32(bn_b)) for n in _probe_norm()]
        out["contour1_w"], out["contour1_b"] = _live_conv1(
            rng, base["contour1_w"], base["contour1_b"], lambda w, b: [F.conv2d(s, w, b, padding=(1, 19)) for s in stacks], batch=32)
        contours = [torch.sigmoid(F.conv2d(F.relu(F.conv2d(s, t("contour1_w"), t("contour1_b"), padding=(1, 19))),
                                           t("contour2_w"), t("contour2_b"), padding=(2, 2))) for s in stacks]
        out["note1_w"], out["note1_b"] = _live_conv1(
            rng, base["note1_w"], base["note1_b"],
            lambda w, b: [F.conv2d(F.pad(c, (2, 2, 3, 3)), w, b, stride=(1, 3)) for c in contours], batch=256)
        out["onset1_w"], out["onset1_b"] = _live_conv1(
            rng, base["onset1_w"], base["onset1_b"],
            lambda w, b: [F.conv2d(F.pad(s, (1, 1, 2, 2)), w, b, stride=(1, 3)) for s in stacks])
    return out


def scaled(seed: int, base: Optional[Dict[str, np.ndarray]] = None, factor: float = SCALED_FACTOR) -> Dict[str, np.ndarray]:
    out = bounded(seed, base)
    f = np.float32(factor)  # a power of two: exact in fp32
    for c in ("contour1", "note1", "onset1"):
        out[c + "_w"] = out[c + "_w"] * f
        out[c + "_b"] = out[c + "_b"] * f
    for c in ("contour2", "note2"):
        out[c + "_w"] = out[c + "_w"] / f
    # onset2's channel 0 reads the note map (a sigmoid output, not a conv1 activation): only the o1 channels shrink
    out["onset2_w"] = out["onset2_w"].copy()
    out["onset2_w"][:, 1:] /= f
    return out


def zero(base: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    out = bounded(0, base)
    for k in CONV_W:
        out[k] = np.zeros_like(out[k])
    return out


# the families GPU tests may use: each passes the admission conditions (tests/test_weight_families_cpu.py)
BOUNDED_SEEDS = (0, 4, 5)  # of seeds 0 .. 8, those that meet (a): 1, 2, 3, 6, 8 saturate the onset map
FAMILIES = {
    **{f"bounded{s}": (lambda s=s: bounded(s)) for s in BOUNDED_SEEDS},
    "scaled": lambda: scaled(0),
}
MODE_FAMILY = "bounded4"  # the one bounded family of the bf16, extended-CQT, fused-batch and A/B runs (negative bn_a)


@functools.lru_cache(maxsize=None)
def _family(name: str) -> Dict[str, np.ndarray]:
    return zero() if name == "zero" else FAMILIES[name]()


def family(name: str) -> Dict[str, np.ndarray]:
    """the tensors of a family by name (a fresh dict of the cached arrays: replace entries, do not write into them).
    Generating one costs the CQT of the nine probe windows once per process (~5 s) and, per conv1 layer, a few batches of
    candidate convolutions on them (1 - 3 s per family)."""
    return dict(_family(name))


def blob_path(tmp_dir, tensors: Dict[str, np.ndarray], name: str = "family.bin") -> str:
    from basic_pitch_amd.weights import pack_blob

    path = os.path.join(str(tmp_dir), name)
    with open(path, "wb") as f:
        f.write(pack_blob(tensors))
    return path


def bf16_round(a: np.ndarray) -> np.ndarray:
    """round to nearest even onto bf16, as tests/test_gpu_parity.py::test_bf16_weights_mode and bp_create do"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_weights(tensors: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    out = dict(tensors)
    for k in CONV_W:
        out[k] = bf16_round(tensors[k])
    return out


def windows() -> np.ndarray:
    """the `cases` windows of tests/test_gpu_parity.py (2 uniform, 1 normal, 1 tones) + one silent window"""
    return np.concatenate([make_windows("uniform", 2, 0), make_windows("normal", 1, 1), make_windows("tones", 1, 2),
                           np.zeros((1, O.AUDIO_N_SAMPLES), np.float32)])


def windows_ext() -> np.ndarray:
    """44.1 kHz windows for the extended mode (as test_extended_cqt_44k_mode draws them) + one silent window"""
    rng = np.random.default_rng(21)
    x = rng.uniform(-1, 1, (4, O.EXT_AUDIO_N_SAMPLES)).astype(np.float32)
    t = np.arange(O.EXT_AUDIO_N_SAMPLES) / 44100.0
    x[2] = (0.4 * np.sin(2 * np.pi * 9000.0 * t) + 0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    x[3] = 0.0
    return x


# ---- one stage of the graph on a given input (oracle/bp_oracle.py cnn(), cut at the fused kernels' seams) ------------
def stage(name: str, W: Dict[str, np.ndarray], dtype, z=None, contour=None, note=None, hidden: bool = False):
    """`contour` (z -> contour), `note` (contour -> note) or `onset` (z, note -> onset) evaluated in `dtype` on the given
    arrays (any float dtype: they are converted, not recomputed).  z may hold 309 or 345 bins.  hidden=True also returns
    the stage's conv1 activations."""
    g = lambda k: O._t(W[k], dtype)  # noqa: E731
    with torch.no_grad():
        if name == "contour":
            stack = O.harmonic_stack(O._t(z, dtype))
            h = F.relu(F.conv2d(stack, g("contour1_w"), g("contour1_b"), padding=(1, 19)))
            out = torch.sigmoid(F.conv2d(h, g("contour2_w"), g("contour2_b"), padding=(2, 2)))
        elif name == "note":
            c = O._t(contour, dtype)[:, None]
            h = F.relu(F.conv2d(F.pad(c, (2, 2, 3, 3)), g("note1_w"), g("note1_b"), stride=(1, 3)))
            out = torch.sigmoid(F.conv2d(h, g("note2_w"), g("note2_b"), padding=(3, 1)))
        elif name == "onset":
            stack = O.harmonic_stack(O._t(z, dtype))
            h = F.relu(F.conv2d(F.pad(stack, (1, 1, 2, 2)), g("onset1_w"), g("onset1_b"), stride=(1, 3)))
            cat = torch.cat([O._t(note, dtype)[:, None], h], dim=1)
            out = torch.sigmoid(F.conv2d(cat, g("onset2_w"), g("onset2_b"), padding=(1, 1)))
        else:
            raise ValueError(name)
    return (out[:, 0].numpy(), h.numpy()) if hidden else out[:, 0].numpy()


def zpack_ref(lp: np.ndarray, minmax: np.ndarray, W: Dict[str, np.ndarray]) -> np.ndarray:
    """norm + BN in fp64 on the given fp32 log-power and extrema (signal.py:177-183, models.py:187-189)"""
    lp = np.asarray(lp, np.float64)
    mn, mx = (np.asarray(minmax, np.float64)[:, i][:, None, None] for i in (0, 1))
    rng = mx - mn
    nrm = np.where(rng == 0, 0.0, (lp - mn) / np.where(rng == 0, 1.0, rng))
    return nrm * float(W["bn_affine"][0]) + float(W["bn_affine"][1])


def stage_refs(W: Dict[str, np.ndarray], r32: Dict[str, np.ndarray]) -> Dict[str, Dict[str, np.ndarray]]:
    """fp64 and torch-fp32 evaluations of every fused stage on the SAME fp32 input (the fp32 oracle's tensors r32): what
    the GPU stage tests compare with, and what admission (c) bounds."""
    feeds = {"contour": dict(z=r32["z"]), "note": dict(contour=r32["contour"]), "onset": dict(z=r32["z"], note=r32["note"])}
    out = {"f64": {}, "f32": {}}
    for k, feed in feeds.items():
        out["f64"][k] = stage(k, W, np.float64, **feed)
        out["f32"][k] = stage(k, W, np.float32, **feed)
    out["f64"]["zpack"] = zpack_ref(r32["lp"], r32["minmax"], W)
    out["f32"]["zpack"] = r32["z"]
    return out


def gate(stage_name: str) -> float:
    return ZPACK_GATE if stage_name == "zpack" else BRANCH_GATE


def admission(W: Dict[str, np.ndarray], x: np.ndarray, ext: bool = False) -> Dict[str, object]:
    """The figures of the four admission conditions on the windows x, and `ok`:
      (a) >= 0.90 of each of note / onset / contour in [0.02, 0.98] (fp64 oracle);
      (b) every hidden channel of c1 / n1 / o1 positive on >= 5 % and zero on >= 5 % of its positions;
      (c) torch fp32 within half the stage's GPU gate of fp64, both fed the fp32 oracle's stage input;
      (d) |z| and the hidden activations below 1/8 of the f16 maximum."""
    r64 = O.forward(x.astype(np.float64), W, np.float64, intermediates=True, ext=ext)
    r32 = O.forward(x, W, np.float32, intermediates=True, ext=ext)
    a = {k: float(((r64[k] >= 0.02) & (r64[k] <= 0.98)).mean()) for k in ("note", "onset", "contour")}
    b = {}
    for k in ("c1", "n1", "o1"):
        pos = (r64[k] > 0).mean(axis=(0, 2, 3))
        b[k] = (float(pos.min()), float(pos.max()))
    refs = stage_refs(W, r32)
    c = {k: float(np.abs(refs["f32"][k] - refs["f64"][k]).max()) for k in ("contour", "note", "onset", "zpack")}
    d = {k: float(np.abs(r64[k]).max()) for k in ("z", "c1", "n1", "o1")}
    ok = (min(a.values()) >= 0.90 and all(lo >= 0.05 and hi <= 0.95 for lo, hi in b.values())
          and all(c[k] <= 0.5 * gate(k) for k in c) and max(d.values()) < F16_MAX / 8)
    return {"a": a, "b": b, "c": c, "d": d, "ok": ok}
