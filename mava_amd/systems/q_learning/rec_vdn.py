"""rec_vdn: recurrent value-decomposition networks (Sunehag et al. 2017) - rec_iql's per-agent recurrent Q networks with
Q_tot = sum_j Q_j regressed on the team reward (mava_amd/qmix_learner.py with system.mixer=vdn: no mixer parameters).

`learner_setup(env, keys, config)` and `run_experiment(config, log=None)` as rec_iql.py; runs on the environments rec_iql
runs on (env=lbf, the default, env=rware_native, env=connector, env=cleaner, env=smax_native) with the same refusals.

    python -m mava_amd.systems.q_learning.rec_vdn env=smax_native system.total_timesteps=200000
"""
from __future__ import annotations

from .. import off_policy
from . import _mixer_runner as _runner

MIXER = "vdn"


def learner_setup(env, keys, config, device=None):
    return _runner.learner_setup(env, keys, config, MIXER, device)


def _check_config(config) -> None:
    _runner.check_config(config, MIXER)


def run_experiment(config, log=None) -> float:
    return off_policy.run_experiment(config, _runner.spec(MIXER), log)


if __name__ == "__main__":
    import sys

    from ...config import compose

    print(run_experiment(compose("default_rec_vdn", sys.argv[1:])))
