"""Per-phase cycle stamps of the Robot Warehouse step kernel (block 0, thread 0) from a -DMAVA_STAMPS build:

    tools/build_stamps.sh && MAVA_LIB_PATH=tools/libmavahip_stamps.so python tools/rware_stamps.py [--real] [--overlap]

4096 envs x tiny-4ag, random actions, mid-episode states; cycles per launch by phase, summed over 200 launches."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mava_amd._lib import lib
from mava_amd.envs import RobotWarehouse
dev = torch.device("cuda", 0)
L = lib()
L.mava_debug_set_rware_stamps.argtypes = [C.c_void_p]
real, mode = "--real" in sys.argv, "overlap" if "--overlap" in sys.argv else "terminate"
E, A, N = 4096, 4, 200
env = RobotWarehouse(E, 8, 1, 3, A, 1, 4, 500, mode, add_global_state=True, device=dev)
st, obs = env.alloc_state(), env.alloc_obs()
env.step_into(st, 0, obs, is_reset=True)
tr = (torch.empty((E, A), device=dev), torch.empty((E, A), dtype=torch.uint8, device=dev), torch.empty(E, device=dev),
      torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.uint8, device=dev))
kw = dict(real_obs={"agents_view": torch.empty_like(obs["agents_view"]), "action_mask": torch.empty_like(obs["action_mask"])},
          terminated=torch.empty(E, dtype=torch.uint8, device=dev)) if real else {}
acts = [torch.randint(0, 5, (E, A), dtype=torch.int32, device=dev) for _ in range(8)]
for t in range(1, 31):
    env.step_into(st, t, obs, *tr, action=acts[t % 8], **kw)
torch.cuda.synchronize()
stamps = torch.zeros(8, dtype=torch.int64, device=dev)
L.mava_debug_set_rware_stamps(stamps.data_ptr())
ends = 0
for t in range(31, 31 + N):
    env.step_into(st, t, obs, *tr, action=acts[t % 8], **kw)
    ends += int(tr[4][:16].sum())
torch.cuda.synchronize()
L.mava_debug_set_rware_stamps(None)
s = stamps.cpu().numpy()
print(f"collision_mode={mode} real_next={real}: cycles per launch by phase (block 0; {ends / N:.2f} of its 16 envs reset per launch):")
names = ["layout + state load", "ground tables", "rule phase (plain: + reset draws)", "real_next: pre-reset view + reset draws",
         "reset fill", "row bytes (header, mask bit, view cells)", "output: view, state, mask", "output: advanced state"]
for n, v in zip(names, s):
    print(f"  {n:42s} {v / N:8.0f}  ({100 * v / s.sum():5.1f} %)")
print(f"  {'total':42s} {s.sum() / N:8.0f}")
