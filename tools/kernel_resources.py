#!/usr/bin/env python3
"""Registers, spills and scratch of every kernel instance of the library's .hip files - no GPU needed.

    python tools/kernel_resources.py rollout_h2.hip ppo_train_w8.hip ppo_train_h2.hip > profiles/<name>_resources.txt

Compiles each file with the flags of mava_amd/build.py plus -Rpass-analysis=kernel-resource-usage (objects are thrown
away) and prints one line per kernel: VGPRs, AGPRs, SGPRs, spilled VGPRs, spilled SGPRs, scratch bytes per lane,
occupancy.  A kernel whose scratch is not 0 spills or indexes a private array: look at it before it is benchmarked.
With no argument every source of the library is compiled (a few minutes).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"))


def _build_module():
    # mava_amd/build.py without importing the package (which loads the library and torch)
    import importlib.util

    spec = importlib.util.spec_from_file_location("_mava_build", os.path.join(ROOT, "mava_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _demangle(names):
    tool = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(tool):
        tool = shutil.which("c++filt")
    if not tool:
        return names
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.split("\n")[: len(names)]
    return out if r.returncode == 0 and len(out) == len(names) else names


def _short(name: str) -> str:
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)  # kernel<template arguments>, without the parameter list


def resources(src: str, extra=()):
    """[(kernel, {field: int})] of one .hip file of mava_amd/csrc, in the order the compiler reports them."""
    b = _build_module()
    path = src if os.path.exists(src) else os.path.join(b.CSRC, src)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ([b.HIPCC, "-c", path, "-o", os.path.join(tmp, "x.o")] + b.COMMON_FLAGS + b.HIP_FLAGS + b.EXTRA_FLAGS + list(extra)
               + ["-Rpass-analysis=kernel-resource-usage"])
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*Function Name: (\S+)", line)
        if m:
            cur = {}
            out.append((m.group(1), cur))
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark: (?:\S+: )?\s*" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    names = _demangle([n for n, _ in out])
    return [(_short(n), d) for n, (_, d) in zip(names, out)]


def main(argv):
    b = _build_module()
    srcs = argv or b.HIP_SOURCES
    print(f"{'kernel':<78} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'vspill':>6} {'sspill':>6} {'scratch':>7} {'occ':>3}")
    for src in srcs:
        print(f"# {os.path.basename(src)}")
        for name, d in resources(src):
            if "vgpr" not in d:
                continue
            print(f"{name:<78} {d.get('vgpr', 0):>5} {d.get('agpr', 0):>5} {d.get('sgpr', 0):>5} {d.get('vspill', 0):>6} "
                  f"{d.get('sspill', 0):>6} {d.get('scratch', 0):>7} {d.get('occ', 0):>3}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
