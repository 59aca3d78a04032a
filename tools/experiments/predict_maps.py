"""Whole-path maps of given windows from whichever library BASIC_PITCH_AMD_LIB names (the A/B library beside the product):
python predict_maps.py in.npz out.npz.  in.npz: x (n, 43844) float32.  out.npz: the note / onset / contour maps."""
import os, sys
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from basic_pitch_amd import Model

m = Model(max_windows=8)
out = m.predict(np.load(sys.argv[1])["x"])
m.close()
np.savez(sys.argv[2], **out)
print("saved", sys.argv[2])
