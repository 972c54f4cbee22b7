"""ff_mat: the Multi-Agent Transformer (Wen et al. 2022; upstream entry points ff_mat / mava.systems.mat).

An encoder attends over all agents' observations and emits one value per agent; a decoder emits the actions agent by
agent, each conditioned on the actions already chosen.  `learner_setup(env, keys, config)` and `run_experiment(config)`
as the other PPO systems; the learner is mava_amd/mat_learner.py.
"""
from __future__ import annotations

from ... import envs as environments
from ... import mat_learner as _learner
from . import anakin


def learner_setup(env, keys, config, device=None):
    return _learner.learner_setup(env, keys, config, device)


def run_experiment(config, log=None) -> float:
    return anakin.run_experiment(config, learner_setup, environments.make, add_global_state=False, log=log)


if __name__ == "__main__":
    import sys

    from ...config import compose

    print(run_experiment(compose("default_ff_mat", sys.argv[1:])))
