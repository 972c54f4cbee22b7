"""rec_iql: recurrent independent (double) Q-learning, mava/systems/q_learning/rec_iql.py.

`learner_setup(env, keys, config)` (init + make_update_fns, :62-530) and `run_experiment(config, log=None)` (:533-659):
train for the updates of one evaluation interval, log MISC {timestep, epsilon}, ACT episode metrics when an episode
completed, TRAIN losses (skipped while the buffer is below the train gate), EVAL with the greedy (eps = 0) policy,
checkpoint, and finally ABSOLUTE with the best parameters.  Runs on env=lbf (the default here; the reference's default is
smax, here env=smax_native), env=rware_native, env=connector and env=cleaner; environments without a pre-reset
observation (the synthetic stand-ins) are refused.

    python -m mava_amd.systems.q_learning.rec_iql env/scenario=10x10-3p-3f system.total_timesteps=200000
"""
from __future__ import annotations

import copy
import time
from typing import Any, Callable, Dict, Optional

import torch

from ... import envs as environments
from ... import iql_learner as _learner
from ...config import Config, check_total_timesteps
from ...learner import get_final_step_metrics
from ..ppo.anakin import _tree_clone, _tree_to, _unreplicate_n_dims
from .types import QNetParams


def learner_setup(env, keys, config, device=None):
    return _learner.learner_setup(env, keys, config, device)


def _check_config(config: Config) -> None:
    """Refusals that need no environment or device (the learner repeats them with its own context)."""
    import torch.distributed as dist

    s = config.system
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("rec_iql runs on one device (multi-GPU is not implemented)")
    if int(s.update_batch_size) != 1:
        raise NotImplementedError("rec_iql supports update_batch_size == 1 only")
    if int(config.network.get("hidden_state_dim", 128)) != 128:
        raise ValueError("rec_iql needs network.hidden_state_dim == 128 (the fused acting step and the scans)")
    qn = config.network.get("q_network", None)
    if qn is None or not (_learner._default_torso(qn.get("pre_torso")) and _learner._default_torso(qn.get("post_torso"))):
        raise NotImplementedError("rec_iql runs network/rnn.yaml's q_network torsos only (MLPTorso [128] relu)")
    native = config.env.get("env_name", None) in ("RobotWarehouse", "Smax") and bool(config.env.get("native", False))
    if config.env.get("env_name", None) not in ("LevelBasedForaging", "MaConnector", "Cleaner") and not native:
        raise ValueError(f"rec_iql needs an environment that returns its pre-reset observation (env=lbf, "
                         f"env=rware_native, env=connector, env=cleaner, env=smax_native); "
                         f"{config.env.get('env_name', None)} runs on the synthetic stand-in, which does not")


def run_experiment(_config: Config, log: Optional[Callable[[Dict[str, Any]], None]] = None) -> float:
    config = copy.deepcopy(_config)
    _check_config(config)
    config.arch.n_devices = 1
    config = check_total_timesteps(config, 1)
    s = config.system
    # rec_iql.py:535-543: env steps per evaluation interval and the updates that take them
    steps_per_rollout = int(s.total_timesteps // config.arch.num_evaluation)
    act_steps = int(config.arch.num_envs) * int(s.rollout_length)
    s.num_updates_per_eval = max(1, steps_per_rollout // act_steps)

    env, eval_env = environments.make(config)
    seed = int(s.seed)
    key, q_key, key_e = seed, seed + 1, seed + 2  # stands in for the reference's key splits
    learn, q_network, learner_state = learner_setup(env, (key, q_key), config)

    from ...evaluator import get_eval_fn, make_rec_eval_act_fn
    from ...utils.logger import LogEvent, MavaLogger

    # eval_act_fn (:563-578): the epsilon-greedy distribution at eps = 0 (q_network.apply's default): greedy either way
    act_fn = make_rec_eval_act_fn(q_network.apply, config)
    init_act_state = {"hidden_state": torch.zeros((eval_env.num_envs, eval_env.num_agents, 128), device=eval_env.device)}
    evaluator = get_eval_fn(eval_env, act_fn, config, absolute_metric=False)

    ck = config.logger.checkpointing
    checkpointer = None
    if bool(ck.save_model):
        from ...utils.checkpointing import Checkpointer

        checkpointer = Checkpointer(metadata=config.to_container(), model_name=str(config.logger.system_name),
                                    **{k: (v if v != "" else None) for k, v in dict(ck.save_args).items()})
    if bool(ck.load_model):
        from ...utils.checkpointing import Checkpointer

        loaded = Checkpointer(model_name=str(config.logger.system_name), **{k: v for k, v in dict(ck.load_args).items()})
        restored, _ = loaded.restore_params(input_params=learner_state.params)
        learner_state = learner_state._replace(params=_tree_to(restored, eval_env.device))  # learn() adopts online + target

    logger = MavaLogger(config) if log is None else None

    def emit(event: str, rec: Dict[str, Any], t: int, idx: int) -> None:
        if logger is not None:
            logger.log(rec, t, idx, getattr(LogEvent, event))
        else:
            out = {k: (float(v.float().mean()) if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}
            if "won_episode" in out:  # what MavaLogger.calc_winrate makes of it
                out["win_rate"] = 100.0 * out.pop("won_episode")
            log({"event": event, "timestep": t, **out})

    eval_return, max_return, best_params, t = 0.0, -float("inf"), None, 0
    n_evals = int(config.arch.num_evaluation)
    for eval_idx in range(n_evals):
        torch.cuda.synchronize()
        start = time.time()
        out = learn(learner_state)
        torch.cuda.synchronize()
        elapsed = time.time() - start
        learner_state = out.learner_state
        t = steps_per_rollout * (eval_idx + 1)
        eps = _learner.epsilon(t, s.eps_min, s.eps_decay)  # :604-606, at the interval's end
        ep_metrics, ep_completed = get_final_step_metrics(out.episode_metrics)
        ep_metrics = dict(ep_metrics)
        ep_metrics["steps_per_second"] = steps_per_rollout / elapsed
        emit("MISC", {"timestep": t, "epsilon": eps}, t, eval_idx)
        if ep_completed:
            emit("ACT", ep_metrics, t, eval_idx)
        if out.train_metrics:
            emit("TRAIN", out.train_metrics, t, eval_idx)
        eval_params = _tree_clone(learner_state.params.online)
        eval_metrics = evaluator(eval_params, key_e + eval_idx, init_act_state)
        emit("EVAL", eval_metrics, t, eval_idx)
        eval_return = float(eval_metrics["episode_return"].float().mean())
        if bool(config.arch.absolute_metric) and max_return <= eval_return:
            best_params, max_return = eval_params, eval_return
        if checkpointer is not None:  # online + target (QNetParams); the replay buffer is not checkpointed
            p = _unreplicate_n_dims(learner_state.params)
            checkpointer.save(timestep=t, unreplicated_learner_state={"params": QNetParams(p.online, p.target)._asdict()},
                              episode_return=eval_return)
    if bool(config.arch.absolute_metric) and best_params is not None:
        abs_metrics = get_eval_fn(eval_env, act_fn, config, absolute_metric=True)(best_params, key, init_act_state)
        emit("ABSOLUTE", abs_metrics, t, n_evals - 1)
    if logger is not None:
        logger.stop()
    return eval_return


if __name__ == "__main__":
    import sys

    from ...config import compose

    print(run_experiment(compose("default_rec_iql", sys.argv[1:])))
