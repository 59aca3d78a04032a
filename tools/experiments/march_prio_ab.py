"""The three posteriorgrams of a seeded batch through the whole path, saved as one .npz (A/B of the marches' priority rule:
run once per BP_MARCH_PRIO / BASIC_PITCH_AMD_LIB setting and compare the files; the rule moves no arithmetic, so they are
bit-equal).

    march_prio_ab.py OUT.npz N [--bf16-weights]     N windows; N = ncu: one window per compute unit of the device, the
                                                    smallest batch whose marches run both halves of their grid at once
    march_prio_ab.py --cmp A.npz B.npz"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
if sys.argv[1] == "--cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    for k in ("note", "onset", "contour"):
        print(k, a[k].shape, "bit-equal" if np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) else "DIFFERENT")
    sys.exit(0)
bf16 = "--bf16-weights" in sys.argv
if bf16:
    sys.argv.remove("--bf16-weights")
import torch
from basic_pitch_amd import inference

n = torch.cuda.get_device_properties(0).multi_processor_count if sys.argv[2] == "ncu" else int(sys.argv[2])
rng = np.random.default_rng(21)
x = rng.uniform(-1, 1, (n, 43844)).astype(np.float32)
x[0, :2000] = 0.0  # digital silence at a window's head
m = inference.Model(max_windows=n, bf16_weights=bf16)
assert m.info()["compute_units"] == torch.cuda.get_device_properties(0).multi_processor_count
got = m.predict(x)
np.savez(sys.argv[1], note=got["note"], onset=got["onset"], contour=got["contour"], n_cu=m.info()["compute_units"])
print("saved", sys.argv[1], {k: (got[k].shape, float(got[k].mean())) for k in ("note", "onset", "contour")})
