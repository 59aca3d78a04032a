#!/usr/bin/env python
"""Did a source change alter any kernel's device code?  Compiles every HIP source of the product library and of the A/B
library to gfx950 assembly (build.FLAGS, `-S --cuda-device-only`) at a parent revision and in the working tree, and
compares each kernel's text after taking out what depends on where the kernel stands rather than on what it does: the
directives that carry file names or line numbers, comments, and the numbering of local labels (a function's index in
its file changes when a file is split).  Whole kernel texts are hashed; no instruction is looked at.

    python tools/kernel_digest.py [--parent REV] [--out profiles/NAME.md] [--dump DIR] [--cache DIR]

--dump keeps every normalised kernel text under DIR/{parent,branch}/ (diff two of them to see what moved); --cache keeps a
revision's digests between runs.  Exit status 1 if a kernel differs, appears or disappears."""
import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "basic_pitch_amd"

_DROP = re.compile(r"^\s*(\.file|\.loc|\.ident)\b")
_LABEL = re.compile(r"\.L[A-Za-z0-9_$.]+")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_bp_build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def normalise(lines):
    """One function's lines without position-dependent directives and comments, local labels numbered by first use"""
    names, out = {}, []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or _DROP.match(line):
            continue
        out.append(_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return "\n".join(out) + "\n"


def kernel_texts(asm):
    """{kernel symbol: normalised text of its code and of its .amdhsa_kernel descriptor block}"""
    lines = [l.split(";", 1)[0].rstrip() for l in asm.splitlines()]
    kernels = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    res = {}
    for k in kernels:
        start = lines.index(k + ":")
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        d0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(k) + r"\s*$", l))
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        res[k] = normalise(lines[start:end] + lines[d0 : d1 + 1])
    return res


def tree_kernels(tree, flags, jobs):
    """{(library, kernel symbol): (source file, normalised text)} of a tree's product and A/B libraries"""
    build = load_build(tree)
    if list(build.FLAGS) != list(flags):
        raise SystemExit(f"build.FLAGS of {tree} differ from the working tree's: the comparison would not mean anything")
    csrc = os.path.join(tree, PKG, "csrc")
    work = [("product", s, []) for s in build.SOURCES if s.endswith(".hip")]
    work += [("ab", s, ["-DBP_AB_KERNELS"]) for s in build.SOURCES + build.AB_SOURCES if s.endswith(".hip")]
    hipcc = build.find_hipcc()

    def one(item):
        lib, src, extra = item
        cmd = [hipcc] + list(flags) + extra + ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, src)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src} ({lib}):\n{res.stderr}")
        return [((lib, k), (src, t)) for k, t in kernel_texts(res.stdout).items()]

    out = {}
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        for rows in pool.map(one, work):
            for key, val in rows:
                if key in out:
                    raise RuntimeError(f"kernel {key} is defined in {out[key][0]} and in {val[0]}")
                out[key] = val
    return out


def digests(kernels, dump=None):
    if dump:
        os.makedirs(dump, exist_ok=True)
        for (lib, k), (_src, text) in kernels.items():
            with open(os.path.join(dump, f"{lib}.{k}.s"), "w") as f:
                f.write(text)
    return {f"{lib} {k}": [src, hashlib.sha256(text.encode()).hexdigest()[:16]] for (lib, k), (src, text) in kernels.items()}


def parent_digests(rev, flags, jobs, dump, cache):
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", rev], capture_output=True, text=True, check=True).stdout.strip()
    cached = os.path.join(cache, sha + ".json") if cache else None
    if cached and os.path.exists(cached) and not dump:
        return sha, json.load(open(cached))
    with tempfile.TemporaryDirectory() as tmp:  # outside the repository: nothing of the parent's reaches the working tree
        tar = subprocess.run(["git", "-C", ROOT, "archive", sha, PKG, "include"], capture_output=True, check=True).stdout
        with open(os.path.join(tmp, "src.tar"), "wb") as f:
            f.write(tar)
        with tarfile.open(os.path.join(tmp, "src.tar")) as t:
            t.extractall(tmp)
        d = digests(tree_kernels(tmp, flags, jobs), dump and os.path.join(dump, "parent"))
    if cached:
        os.makedirs(cache, exist_ok=True)
        json.dump(d, open(cached, "w"))
    return sha, d


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="HEAD", help="revision to compare the working tree with (default HEAD)")
    ap.add_argument("--out", help="write the table to this markdown file")
    ap.add_argument("--dump", help="keep the normalised kernel texts under this directory")
    ap.add_argument("--cache", help="keep a revision's digests under this directory")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()

    flags = load_build(ROOT).FLAGS
    sha, parent = parent_digests(a.parent, flags, a.jobs, a.dump, a.cache)
    branch = digests(tree_kernels(ROOT, flags, a.jobs), a.dump and os.path.join(a.dump, "branch"))

    keys = sorted(set(parent) | set(branch))
    names = demangle(sorted({k.split(" ", 1)[1] for k in keys}))
    rows, n_diff = [], 0
    for key in keys:
        lib, sym = key.split(" ", 1)
        p, b = parent.get(key), branch.get(key)
        same = p is not None and b is not None and p[1] == b[1]
        n_diff += not same
        rows.append((lib, names[sym], p[0] if p else "-", b[0] if b else "-", p[1] if p else "-", b[1] if b else "-",
                     "equal" if same else "DIFFERENT"))
    head = [f"# Kernel digests: parent {sha[:12]} against the working tree", "",
            "`tools/kernel_digest.py`: sha256 (first 16 hex digits) of every kernel's gfx950 assembly and descriptor block, built",
            "with `build.FLAGS` (`-DBP_AB_KERNELS` added for the A/B library), without file / line directives and comments and",
            "with local labels renumbered per kernel.", "",
            f"{len(keys)} kernels, {n_diff} different.", "",
            "| library | kernel | parent source | branch source | parent digest | branch digest | |",
            "|---|---|---|---|---|---|---|"]
    table = "\n".join(head + ["| " + " | ".join(f"`{c}`" if i in (1, 4, 5) else c for i, c in enumerate(r)) + " |" for r in rows]) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(table)
    for r in rows:
        if r[6] != "equal" or not a.out:
            print(f"{r[6]:9s} {r[0]:7s} {r[4]:16s} {r[5]:16s} {r[1][:110]}")
    print(f"{len(keys)} kernels, {n_diff} different")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
