"""The IMA ADPCM decode of a three-minute 44.1 kHz stereo file: the host decoder on one core (bp_adpcm_decode) against the
device call (bp_adpcm_decode_device with no output buffer: the copy of the file's bytes, the one launch, the wait).  Alone
for the wall times; under `rocprofv3 --kernel-trace --stats -- python tools/experiments/adpcm_time.py` for the launch itself."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adpcm_files as A  # noqa: E402
from basic_pitch_amd.inference import Model  # noqa: E402


def main():
    rate, seconds = 44100, 180
    rng = np.random.default_rng(3)
    t = np.arange(rate * seconds) / rate
    x = 0.3 * np.sin(2 * np.pi * 220 * t) * (np.sin(2 * np.pi * 1.5 * t) > 0) + 0.01 * rng.standard_normal(t.size)
    pcm = (np.clip(np.stack([x, x[::-1]], 1), -1, 1) * 32767).astype(np.int16)
    res = {}
    with Model(device=0, max_windows=16) as m:
        lib = m._lib
        for name, blob in (("wav_2048", A.ima_wav(pcm, rate, 2048)), ("wav_256", A.ima_wav(pcm, rate, 256)), ("caf_ima4", A.ima4_caf(pcm, rate))):
            lay = m.adpcm_layout(blob)
            out = np.empty((lay["n_frames"], 2), np.int16)
            n = C.c_int64()
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert lib.bp_adpcm_decode(blob, len(blob), out.ctypes.data, out.shape[0], C.byref(n)) == 0
                host.append(time.perf_counter() - t0)
            dev = []
            for _ in range(12):
                t0 = time.perf_counter()
                assert lib.bp_adpcm_decode_device(m._handle, blob, len(blob), None, 0, C.byref(n)) == 0
                dev.append(time.perf_counter() - t0)
            got, _ = m.adpcm_decode_device(blob)
            assert np.array_equal(got, out)
            res[name] = {"file_bytes": len(blob), "frames": lay["n_frames"], "chains": lay["data_bytes"] // lay["block_bytes"] * 2,
                         "host_decode_ms": round(1e3 * float(np.median(host)), 2),
                         "device_call_ms": round(1e3 * float(np.median(dev[2:])), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
