"""Generates tests/golden/cleaner_5x5x5a.npz from the NumPy rules of tests/cleaner_model.py: the reset of six
environments of clean-5x5x5a at a fixed seed and 20 steps with recorded masked-random actions (one agent in ten draws
without the mask, so episodes end on invalid actions too, and the time limit of 8 truncates the rest) - state,
observation and transition after every step.  PARITY UNPINNED with respect to Jumanji's Cleaner: the file pins this
repository's statement of the rules, so that a later edit of the model cannot move the model and the kernel together
(tests/test_cleaner.py holds the model to it, tests/test_gpu_cleaner.py the kernel).
Run:  python tests/golden/make_cleaner_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import cleaner_model as m  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cleaner_5x5x5a.npz")
R, C, A, TIME_LIMIT, E, STEPS, SEED, ENV_OFFSET = 5, 5, 5, 8, 6, 20, 0xC1EA9E5, 1000
OBS = ("agents_view", "global_state", "action_mask", "step_count")
TRANSITION = ("reward", "done", "info_return", "info_length", "info_terminal")


def main() -> None:
    p = m.Params(R, C, A, TIME_LIMIT)
    st, obs = m.reset(p, E, SEED, ENV_OFFSET, 0)
    rec = {f"reset_{k}": st[k].copy() for k in m.STATE_FIELDS}
    rec.update({f"reset_obs_{k}": obs[k] for k in OBS})
    rng = np.random.default_rng(5)
    steps = {k: [] for k in m.STATE_FIELDS + tuple(f"obs_{k}" for k in OBS) + TRANSITION + ("action", "won", "terminated", "real_view", "real_mask")}
    mask = obs["action_mask"]
    for t in range(1, STEPS + 1):
        u = rng.random(mask.shape) * np.where(rng.random(mask.shape[:2] + (1,)) < 0.1, 1.0, mask)
        a = u.argmax(-1).astype(np.int32)
        out = m.step(p, st, a, SEED, ENV_OFFSET, t)
        mask = out[0]["action_mask"]
        steps["action"].append(a)
        for k in m.STATE_FIELDS:
            steps[k].append(st[k].copy())
        for k in OBS:
            steps[f"obs_{k}"].append(out[0][k])
        for k, v in zip(TRANSITION, out[1:6]):
            steps[k].append(v)
        for k in ("won", "terminated", "real_view", "real_mask"):
            steps[k].append(out[6][k])
    rec.update({k: np.stack(v) for k, v in steps.items()})
    rec["params"] = np.array([R, C, A, TIME_LIMIT, E, STEPS, SEED, ENV_OFFSET], np.int64)
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes;", int(rec["info_terminal"].sum()), "episode ends,", int(rec["won"].sum()), "won")


if __name__ == "__main__":
    main()
