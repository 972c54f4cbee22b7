#!/usr/bin/env python3
"""Phase shares of ff_mat's fused backward launch (csrc/mat_train.hip built with -DMAVA_STAMPS).

    python tools/mat_train_stamps.py [--lib PATH] [--envs 1024] [--out profiles/mat_train_stamps.json]

The stamped kernel adds up thread 0's cycle counter per phase and leaves the sums behind each workgroup's slab row.  Without
--lib the tool compiles the stamped kernel alone (hipcc, gfx950) into a temporary directory; the production library is not
touched.  The shape is one minibatch of ff_mat's defaults on tiny-4ag: Bm = 128 * envs / 2 samples, A = 4, O = 70, 5 actions,
D = 64, one head, one block, 256 workgroups.  Inputs are random: the kernel's control flow does not depend on the data.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PHASES = ("forward_recompute", "dW_products_on_the_slab_row", "dX_products_with_W_staging", "layernorm_gelu_backward",
          "attention_backward", "other")
STUB = "void mava_set_error(const char*, ...) {}\n"


def build(tmp: str) -> str:
    from mava_amd import build as b

    stub, out = os.path.join(tmp, "stub.cpp"), os.path.join(tmp, "libmat_train_stamps.so")
    open(stub, "w").write(STUB)
    cmd = [b.HIPCC, "-shared", "-o", out, os.path.join(b.CSRC, "mat_train.hip"), stub, "-DMAVA_STAMPS"] + b.COMMON_FLAGS + b.HIP_FLAGS
    subprocess.run(cmd + b.FILE_FLAGS["mat_train.hip"], check=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:  # (kept for as long as the library is in use)
        measure(C.CDLL(args.lib or build(tmp)), args)


def measure(L, args) -> None:
    from mava_amd import _lib
    from mava_amd.mat_learner import MATNet

    dev = torch.device("cuda", 0)
    Bm, A, O, nA, D, H, nb, blocks = 128 * args.envs // 2, 4, 70, 5, 64, 1, 1, 256
    net, TE, rows = MATNet(O, nA, A, D, H, nb), 128 * args.envs, -(-Bm * A // 32) * 32
    g = torch.Generator().manual_seed(1)
    flat, obs = net.init_flat(5).to(dev), torch.randn((TE, A, O), generator=g).to(dev)
    action = torch.randint(0, nA, (TE, A), generator=g, dtype=torch.int32).to(dev)
    idx = torch.randperm(TE, generator=g)[:Bm].to(torch.int32).to(dev)
    dl, dv = torch.randn(rows * nA, generator=g).to(dev), torch.randn(rows, generator=g).to(dev)
    P = net.num_params
    slab = torch.zeros((blocks, P + 16), device=dev)
    for name in ("mava_transformer_train_workspace_bytes", "mava_transformer_train_bwd_f32"):  # the production table's prototypes
        getattr(L, name).argtypes, getattr(L, name).restype = _lib._SIGNATURES[name], _lib._RESTYPES.get(name, C.c_int)
    ws = torch.zeros(L.mava_transformer_train_workspace_bytes(Bm, A, O, D, nb, blocks), dtype=torch.uint8, device=dev)
    run = lambda: L.mava_transformer_train_bwd_f32(flat.data_ptr(), obs.data_ptr(), TE, idx.data_ptr(), action.data_ptr(), Bm, A, O, nA,
                                                   D, H, nb, dl.data_ptr(), dv.data_ptr(), 1.0, slab.data_ptr(), P + 16, ws.data_ptr(),
                                                   ws.numel(), blocks, torch.cuda.current_stream().cuda_stream)
    assert run() == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    assert run() == 0
    b.record()
    torch.cuda.synchronize()
    cyc = slab[:, P : P + len(PHASES)].double().sum(0).cpu()
    out = {"device": torch.cuda.get_device_name(0), "shape": [Bm, A, O, nA, D, H, nb], "n_blocks": blocks,
           "stamped_launch_ms": round(a.elapsed_time(b), 3),
           "share_of_thread0_cycles": {k: round(float(c / cyc.sum()), 4) for k, c in zip(PHASES, cyc)}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
