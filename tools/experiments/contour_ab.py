"""Contour stage (rim + interior conv1 + conv2) on random inputs through the C ABI test hook; saves the map (A/B of the
conv1 / conv2 kernels: run once per BP_CONV1 / BP_CONV2 / BASIC_PITCH_AMD_LIB setting and compare the files with --cmp).
  --weights PATH    the model the handle loads instead of the shipped one
  --n N             windows of the run (default 3): the batch size decides the march's frame chunks
  --bf16            a handle with bf16_weights (the kernels' WLO = false forms)
  --window0 A,B,..  one run per batch size, all on the same input: saves window 0 of each, [len][172][264]"""
import os, sys
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
if sys.argv[1] == "--cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    d = np.abs(a - b)
    print("max", d.max(), "n>1e-6", int((d > 1e-6).sum()), "of", d.size)
    sys.exit(0)


def take(flag, has_value=True):
    """removes `flag [value]` from the command line; the value, True for a bare flag, None when absent"""
    if flag not in sys.argv:
        return None
    i = sys.argv.index(flag)
    v = sys.argv[i + 1] if has_value else True
    del sys.argv[i : i + (2 if has_value else 1)]
    return v


weights = take("--weights")
n = int(take("--n") or 3)
bf16 = bool(take("--bf16", has_value=False))
window0 = take("--window0")
sizes = [int(v) for v in window0.split(",")] if window0 else [n]
n = max(sizes)
from stage_harness import StageRunner, zp_pack
import torch
from basic_pitch_amd import Model

rng = np.random.default_rng(11)
z = (rng.random((n, 172, 309), dtype=np.float32) * 2.4 - 0.8).astype(np.float32)
model = None
if weights or bf16 or n > 256:
    kw = dict(bf16_weights=bf16, max_windows=max(n, 256))
    model = Model(weights, **kw) if weights else Model(**kw)
r = StageRunner(model)
zp = zp_pack(z).view(np.int32)
maps = [r.run("contour", k, {"zp": zp[:k]}, {"contour": ((k, 172, 264), torch.float32)})["contour"] for k in sizes]
got = np.stack([m[0] for m in maps]) if window0 else maps[0]
np.save(sys.argv[1], got)
print("saved", sys.argv[1], got.shape, float(got.mean()))
