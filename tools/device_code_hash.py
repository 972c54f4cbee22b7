#!/usr/bin/env python3
"""sha256 of the device code of every built translation unit: does a change touch what the GPU runs?

    python tools/device_code_hash.py [--tree DIR] [--json]

For each object under DIR/mava_amd/csrc/*.o (build first: python -m mava_amd.build) it prints the sha256 of the `.text`
section of the gfx950 code object.  The fat binary and the whole code object differ between two builds of one source
(they carry build paths and identifiers); `.text`, the instructions of every kernel, is the same across rebuilds and
changes only when a kernel's code does.  Two trees with equal hashes run the same instructions; `.text` only: the kernel
descriptors (register counts, LDS size) live in `.rodata` and are not hashed.  Objects without a `.hip_fatbin` section
(api.cpp, comm.cpp) print "-".
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def text_hash(obj: str) -> str:
    with tempfile.TemporaryDirectory() as tmp:
        fat, co, text = (os.path.join(tmp, n) for n in ("fatbin", "code.o", "text"))
        sections = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", obj], check=True, capture_output=True,
                                  text=True).stdout
        if ".hip_fatbin" not in sections.split():  # host-only object
            return "-"
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj,
                        os.path.join(tmp, "copy.o")], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={fat}", f"--output={co}"], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text], check=True,
                       capture_output=True)
        with open(text, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", default=ROOT, help="repository root whose built objects are hashed")
    ap.add_argument("--json", action="store_true", help="print one JSON object instead of a table")
    a = ap.parse_args()
    objs = sorted(glob.glob(os.path.join(a.tree, "mava_amd", "csrc", "*.o")))
    if not objs:
        raise SystemExit(f"no objects under {a.tree}/mava_amd/csrc: run python -m mava_amd.build")
    table = {os.path.basename(o)[:-2]: text_hash(o) for o in objs}
    if a.json:
        print(json.dumps(table, indent=1, sort_keys=True))
    else:
        for name, h in table.items():
            print(f"{h}  {name}")


if __name__ == "__main__":
    main()
