"""Diagnostic: per-phase cycle shares of the fused PPO train kernels (needs a library built with
MAVA_HIPCC_EXTRA="-DMAVA_STAMPS").  Prints, per wave of block 0, the cycles spent in each phase.
    python tools/train_stamps.py [f16x2] [w4] [exact] [x16]
`exact`: observations exact in f16 (bits), as RobotWarehouse's are - the wide critic then runs its exact-input tile loop and
the eight-wave actor its two-product layer 1; without it the inputs are Gaussian (general loop, three products).
`x16` (with `exact`): the critic launch is handed an f16 copy of its input and a validity word of 1, as the learner does after a
fused rollout - the wide critic then stages its x tiles from the copy, and the eight-wave actor from a record of its rows laid
out as the rollout's view16 (the observation, 1.0, zeros up to a multiple of 8 halves)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from mava_amd import ops
from mava_amd._lib import Ctx, lib

dev = torch.device("cuda", 0)
MODE = 1 if (len(sys.argv) > 1 and sys.argv[1] == "f16x2") else 0
EXACT = "exact" in sys.argv[2:]
X16 = "x16" in sys.argv[2:]
TE, A, O, nA = 128 * 4096, 4, 66, 5
Rb = TE // 2
rng = np.random.default_rng(0)
names = ["P1 layer1", "P2 layer2+head", "P3 loss+dz2", "P4 dh1+sweeps", "P4b dz1 write", "P5a gW2", "P5b gW1", "barrier E",
         "commit+F", "loop top", "P2a prefetch issue", "P2b mfma loop", "P1a mfma loop", "barrier A", "x issue", "row issue"]
# note: with sub-stamps, "P1 layer1" = epilogue after P1a, "P2 layer2+head" = head part after P2b
if MODE == 1:  # phases of ppo_train_h2.hip
    names = ["P1 mfma", "P1 relu+image", "gather issue", "barrier A", "P2 mfma", "P2 image+head", "barrier B", "P3 loss",
             "B2+dz2+image", "barrier C", "P4 mfma+dz1+commit", "gW3+gW2", "barrier D", "gW1 (wide chain: gW2)", "loop top", "barrier B2"]
# phases of ppo_train_w8.hip (the eight-wave actor kernel, default for the discrete actor; `w4` as a second argument keeps
# the four-wave kernel)
names_w8 = ["P1 mfma", "P1 relu+image", "gather issue", "barrier A", "P2 mfma", "P2 image+head", "barrier B", "P3 loss | x commit",
            "barrier B2", "gW3+dz2+image", "gW2", "barrier C", "dh1+dz1 image", "gW1", "loop top", "gW1 of prev tile (P3)",
            "gathers ahead (P3)", "row loads ahead (<C)"]
# ("gW1 of prev tile": the deferred-dW1 form on the f16 record, `exact x16` - inside P3, ahead of the loss on waves 0-3 and behind
# the commit on waves 4-7; the "gW1" phase at the tile's end then reads about 0.  The last two: the gathers-ahead form of that
# loop - the staging waves' x gathers, index load and cursor update behind the commit, the loss waves' row loads, index load and
# cursor update behind gW2; "gather issue" then reads about 0.  Their sums sit behind the 8 x 16 words of the other phases.)
l = lib()
ctx = Ctx("f16x2" if MODE == 1 else "f32")
if "w4" in sys.argv[2:]:
    ctx.set(ctx.TRAIN_VARIANT, 1)
l.mava_debug_set_stamps.argtypes = [C.c_void_p]
stamps = torch.zeros(144, dtype=torch.int64, device=dev)  # waves 0-3 (chain / only group), 4-7 (loader group of wide launches)
l.mava_debug_set_stamps(stamps.data_ptr())
perm = torch.randperm(TE, device=dev).to(torch.int32)
for which in ("critic", "actor"):
    if which == "critic":
        din = A * O
        params = torch.randn(ops.mlp_param_count(din, 1), device=dev) * 0.05
        x = (torch.rand(TE, din, device=dev) < 0.2).float() if EXACT else torch.randn(TE, din, device=dev)
        ov, tg = torch.randn(TE * A, device=dev), torch.randn(TE * A, device=dev)
        slab = torch.zeros(256, params.numel() + 2, device=dev)
        x16 = x.half() if (X16 and EXACT) else None
        x16_valid = torch.ones(1, dtype=torch.int32, device=dev) if x16 is not None else None
        run = lambda: ops.ppo_critic_grad(params, x, A, ov, tg, perm, 0, Rb, A, 0.2, 0.5, slab, ctx=ctx, input16=x16,
                                          input16_valid=x16_valid)
    else:
        din = A + O
        params = torch.randn(ops.mlp_param_count(din, nA), device=dev) * 0.05
        x = (torch.rand(TE * A, din, device=dev) < 0.2).float() if EXACT else torch.randn(TE * A, din, device=dev)
        mask = (torch.rand(TE * A, nA, device=dev) > 0.2).to(torch.uint8); mask[:, 0] = 1
        act = torch.zeros(TE * A, dtype=torch.int32, device=dev)
        olp, adv = -torch.rand(TE * A, device=dev) - 1.0, torch.randn(TE * A, device=dev)
        st = ops.adv_stats(adv, perm, 0, Rb, A)
        slab = torch.zeros(256, params.numel() + 2, device=dev)
        v16 = v16_valid = None
        if X16 and EXACT:
            v16 = torch.zeros(TE * A, 8 * ((din + 8) // 8), dtype=torch.float16, device=dev)
            v16[:, :din] = x.half(); v16[:, din] = 1.0
            v16_valid = torch.ones(1, dtype=torch.int32, device=dev)
        run = lambda: ops.ppo_actor_grad(params, x, mask, act, olp, adv, st, perm, 0, Rb, A, nA, 0.2, 0.01, slab, ctx=ctx,
                                         input16=v16, input16_valid=v16_valid)
    w8_before = ctx.get(ctx.W8_LAUNCHES)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); run(); b.record(); torch.cuda.synchronize()
    s8 = stamps.cpu().numpy()[:128].reshape(8, 16)
    if which == "critic" and MODE == 1:
        print(f"   (exact-loop tiles of the three launches: {ctx.get(ctx.EXACT_TILES)} of {3 * -(-Rb // 32)}; "
              f"launches on the f16 copy: {ctx.get(ctx.X16_LAUNCHES)})")
    if ctx.get(ctx.W8_LAUNCHES) > w8_before:  # eight equal waves: print waves 0-3 and wave 4 (the SIMD partner of wave 0)
        s8 = np.concatenate([s8, stamps.cpu().numpy()[128:].reshape(8, 2)], axis=1)  # (the eight-wave kernel's two extra phases)
        tot = s8.sum(1)
        ntile = -(-(Rb * A) // 32 // 256)
        print(f"   (eight-wave launches on the f16 record so far: {ctx.get(ctx.X16_W8_LAUNCHES)})")
        print(f"== {which} (eight-wave kernel): launch {a.elapsed_time(b):.3f} ms, block 0 cycles per wave {tot.tolist()}, {ntile} tiles per block")
        for i, n in enumerate(names_w8):
            print(f"   {n:24s} " + "  ".join(f"{s8[w, i] / ntile:8.0f}" for w in (0, 1, 4, 5)) + f"   ({100 * s8[0, i] / tot[0]:5.1f} %)")
        stamps.zero_()
        continue
    s = s8[:4]
    tot = s.sum(1)
    # row tiles per block: agent rows for the actor; (t,e) rows for the critic when the agents of a row are aggregated
    rows = Rb * A if which == "actor" else Rb
    ntile = -(-rows // 32 // 256)
    print(f"== {which}: launch {a.elapsed_time(b):.3f} ms, block 0 cycles per wave {tot.tolist()}, {ntile} tiles per block")
    for i, n in enumerate(names):
        print(f"   {n:24s} " + "  ".join(f"{s[w, i] / ntile:8.0f}" for w in range(4)) + f"   ({100 * s[0, i] / tot[0]:5.1f} %)"
              + (f"   loader wave 4: {s8[4, i] / ntile:8.0f}" if s8[4].sum() > 0 else ""))
    stamps.zero_()
