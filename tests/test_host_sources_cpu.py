"""The host sources of the file job that need no device (csrc/wav_file.cpp, note_writers.cpp, file_io.cpp, with
note_decode.cpp and flac_decode.cpp) link into a program of their own with plain g++ and no stub for any library function:
tools/sanitize/fuzz_host.cpp, the program tools/sanitize/run.sh runs for minutes, here at a twentieth of its iteration
counts.  The link is the test of the split — a device call in one of these sources is an undefined reference.  The program
is built once more with the host sanitizers (address, undefined) and must run clean and print the same two summary lines."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_pitch_amd", "csrc")
DEVICE_FREE = ("flac_decode.cpp", "note_decode.cpp", "wav_file.cpp", "note_writers.cpp", "file_io.cpp")
SCALE = "0.05"  # 300 mutated WAV headers, 15 random maps: about a second under the sanitizers


def _build(out, extra):
    """one g++ per source, side by side (the sanitizer builds of the decoders take four seconds each), then the link"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    srcs = [os.path.join(ROOT, "tools", "sanitize", "fuzz_host.cpp")] + [os.path.join(CSRC, s) for s in DEVICE_FREE]
    flags = ["-std=c++17", "-O1", "-pthread", "-w"] + extra
    cmds = [[cxx] + flags + ["-c", src, "-o", out + "." + os.path.basename(src) + ".o"] for src in srcs]
    return cmds, [cxx] + flags + [c[-1] for c in cmds] + ["-o", out]


def _check(cmd):
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def _run(exe):
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "vocadito_10.wav"), SCALE], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]  # -fno-sanitize-recover: a finding ends the sanitizer build's run
    return res.stdout


def test_the_device_free_sources_link_alone_and_run_clean_under_the_sanitizers(tmp_path):
    plain, san = str(tmp_path / "fuzz_host"), str(tmp_path / "fuzz_host_san")
    builds = [_build(plain, []), _build(san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])]
    with ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as pool:
        list(pool.map(_check, [c for compiles, _ in builds for c in compiles]))
        list(pool.map(_check, [link for _, link in builds]))
    syms = subprocess.run(["nm", san], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the sanitizer build is not instrumented"
    out = _run(plain)
    assert _run(san) == out
    lines = out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("wav ok ") and lines[1].startswith("note decode events "), out
