"""Generates tests/golden/smax_2s3z.npz from the NumPy rules of tests/smax_model.py: the reset of four environments of
2s3z at a fixed seed and 120 steps of the tests' fixed action mix (smax_model.mixed_actions: env 0 and 3 random, env 1
attack-else-east, env 2 always west) - state, transition, mask and flags after every step, and the float observations
(agents_view, global_state, the pre-reset view) after every OBS_EVERY-th step and after the first END_KEPT steps that
ended an episode, which keeps the file small.  PARITY UNPINNED with respect to JaxMARL's SMAX: the file pins this
repository's statement of the rules, so that a later edit of the model cannot move the model and the kernel together
(tests/test_smax.py holds the model to it, tests/test_gpu_smax.py the kernel).
Run:  python tests/golden/make_smax_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import smax_model as m  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smax_2s3z.npz")
SCENARIO, E, STEPS, SEED, ENV_OFFSET, OBS_EVERY, END_KEPT = "2s3z", 4, 120, 0x5AC5EED, 1000, 30, 3
SMALL = ("action_mask", "step_count")  # observation parts kept for every step
FLOATS = ("agents_view", "global_state")  # kept for the steps of `obs_steps`
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")


def main() -> None:
    p = m.scenario(SCENARIO)
    st, obs = m.reset(p, E, SEED, ENV_OFFSET, 0)
    rec = {f"reset_{k}": st[k].copy() for k in m.STATE_FIELDS}
    rec.update({f"reset_obs_{k}": obs[k] for k in SMALL + FLOATS})
    rng = np.random.default_rng(5)
    names = m.STATE_FIELDS + tuple(f"obs_{k}" for k in SMALL) + TRANSITION + ("action", "won", "terminated", "real_mask")
    steps = {k: [] for k in names}
    kept = {k: [] for k in ("obs_steps", "real_view") + tuple(f"obs_{k}" for k in FLOATS)}
    mask = obs["action_mask"]
    for t in range(1, STEPS + 1):
        a = m.mixed_actions(rng, mask)
        out = m.step(p, st, a, SEED, ENV_OFFSET, t)
        mask = out[0]["action_mask"]
        steps["action"].append(a)
        for k in m.STATE_FIELDS:
            steps[k].append(st[k].copy())
        for k in SMALL:
            steps[f"obs_{k}"].append(out[0][k])
        for k, v in zip(TRANSITION, out[1:6]):
            steps[k].append(v)
        for k in ("won", "terminated", "real_mask"):
            steps[k].append(out[6][k])
        ends_kept = sum(1 for n in kept["obs_steps"] if (n + 1) % OBS_EVERY)
        if t % OBS_EVERY == 0 or (out[5].any() and ends_kept < END_KEPT):
            kept["obs_steps"].append(t - 1)
            kept["real_view"].append(out[6]["real_view"])
            for k in FLOATS:
                kept[f"obs_{k}"].append(out[0][k])
    rec.update({k: np.stack(v) for k, v in steps.items()})
    rec.update({k: np.stack(v) for k, v in kept.items()})
    rec["params"] = np.array([E, STEPS, SEED, ENV_OFFSET], np.int64)
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes;", int(rec["info_terminal"].sum()), "episode ends,", int(rec["won"].sum()), "won,",
          len(kept["obs_steps"]), "steps with float observations")


if __name__ == "__main__":
    main()
