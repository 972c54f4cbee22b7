"""Experiment driver shared by the replay-buffer systems (rec_iql, rec_qmix, rec_vdn, ff_isac, ff_masac): the host loop of
mava/systems/q_learning/rec_iql.py:533-659 and mava/systems/sac/ff_isac.py:491-602.  (SAC only: explore with random
actions first.)  Then per evaluation interval: train for the interval's updates, log MISC, ACT episode metrics when an
episode completed, TRAIN (skipped while the learner reports no train metrics), EVAL with the evaluation policy,
checkpoint, and finally ABSOLUTE with the best parameters.  What differs between the systems is their `Spec`.
"""
from __future__ import annotations

import copy
import time
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from .. import envs as environments
from ..config import Config, check_total_timesteps
from ..learner import get_final_step_metrics
from ..utils.tree import tree_clone, unreplicate_n_dims


class Spec(NamedTuple):
    name: str
    check_config: Callable[[Config], None]  # refusals that need no environment or device
    add_global_state: bool  # how the environments are made
    # (env, config) -> (learn, network, initial learner state, (key of the absolute metric, first evaluation key))
    setup: Callable[[Any, Config], Tuple[Callable, Any, Any, Tuple[int, int]]]
    eval_act: Callable[[Any, Config, Any], Tuple[Callable, Any]]  # (network, config, eval_env) -> (act_fn, init_act_state)
    eval_params: Callable[[Any], Any]  # the branch of the learner state's params that the evaluator reads
    misc: Callable[[Config, int], Dict[str, Any]]  # what MISC carries next to the timestep
    train_extra: Callable[[Any], Dict[str, Any]]  # what TRAIN carries next to the losses, from the learner state
    checkpoint_payload: Callable[[Any], Dict[str, Any]]  # unreplicated params -> the "params" item of a checkpoint
    explore_steps: Callable[[Config], int] = lambda config: 0  # env steps taken before the first interval


def eval_schedule(total_timesteps: int, num_evaluation: int, num_envs: int, rollout_length: int,
                  explore_steps: int = 0) -> Tuple[int, int, List[int]]:
    """rec_iql.py:535-543 / ff_isac.py:496-503, :542-547: the env steps of one evaluation interval, the updates that take
    them (at least one), and the timestep every interval is logged at."""
    steps_per_rollout = int(total_timesteps) // int(num_evaluation)
    num_updates_per_eval = max(1, steps_per_rollout // (int(num_envs) * int(rollout_length)))
    timesteps = [int(explore_steps) + steps_per_rollout * (i + 1) for i in range(int(num_evaluation))]
    return steps_per_rollout, num_updates_per_eval, timesteps


def run_experiment(_config: Config, spec: Spec, log: Optional[Callable[[Dict[str, Any]], None]] = None) -> float:
    config = copy.deepcopy(_config)
    spec.check_config(config)
    config.arch.n_devices = 1
    config = check_total_timesteps(config, 1)
    s = config.system
    steps_per_rollout, s.num_updates_per_eval, timesteps = eval_schedule(
        s.total_timesteps, config.arch.num_evaluation, config.arch.num_envs, s.rollout_length, spec.explore_steps(config))

    env, eval_env = environments.make(config, add_global_state=spec.add_global_state)
    learn, network, learner_state, (key, key_e) = spec.setup(env, config)

    from ..evaluator import get_eval_fn
    from ..utils.checkpointing import open_checkpoints
    from ..utils.logger import LogEvent, MavaLogger

    act_fn, init_act_state = spec.eval_act(network, config, eval_env)
    evaluator = get_eval_fn(eval_env, act_fn, config, absolute_metric=False)
    checkpointer, restored = open_checkpoints(config, learner_state.params, eval_env.device)
    learner_state = learner_state._replace(params=restored)  # learn() adopts trees that do not alias its buffers

    logger = MavaLogger(config) if log is None else None

    def emit(event: str, rec: Dict[str, Any], t: int, idx: int) -> None:
        if logger is not None:
            logger.log(rec, t, idx, getattr(LogEvent, event))
        else:
            out = {k: (float(v.float().mean()) if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}
            if "won_episode" in out:  # what MavaLogger.calc_winrate makes of it
                out["win_rate"] = 100.0 * out.pop("won_episode")
            log({"event": event, "timestep": t, **out})

    t = 0
    if hasattr(learn, "explore"):  # ff_isac.py:526-537: fill the buffer with random actions
        torch.cuda.synchronize()
        start = time.time()
        metrics = learn.explore()
        torch.cuda.synchronize()
        t = learn.learner.t
        emit("MISC", {"step": t}, t, 0)
        final_metrics, _ = get_final_step_metrics(metrics)
        final_metrics = dict(final_metrics)
        final_metrics["steps_per_second"] = t / max(time.time() - start, 1e-9)
        emit("ACT", final_metrics, spec.explore_steps(config), 0)

    eval_return, max_return, best_params = 0.0, -float("inf"), None
    for eval_idx, t in enumerate(timesteps):
        torch.cuda.synchronize()
        start = time.time()
        out = learn(learner_state)
        torch.cuda.synchronize()
        elapsed = time.time() - start
        learner_state = out.learner_state
        ep_metrics, ep_completed = get_final_step_metrics(out.episode_metrics)
        ep_metrics = dict(ep_metrics)
        ep_metrics["steps_per_second"] = steps_per_rollout / elapsed
        emit("MISC", {"timestep": t, **spec.misc(config, t)}, t, eval_idx)
        if ep_completed:
            emit("ACT", ep_metrics, t, eval_idx)
        if out.train_metrics:
            emit("TRAIN", {**out.train_metrics, **spec.train_extra(learner_state)}, t, eval_idx)
        eval_params = tree_clone(spec.eval_params(learner_state.params))
        eval_metrics = evaluator(eval_params, key_e + eval_idx, init_act_state)
        emit("EVAL", eval_metrics, t, eval_idx)
        eval_return = float(eval_metrics["episode_return"].float().mean())
        if bool(config.arch.absolute_metric) and max_return <= eval_return:
            best_params, max_return = eval_params, eval_return
        if checkpointer is not None:  # the parameters alone: the replay buffer is not checkpointed
            payload = spec.checkpoint_payload(unreplicate_n_dims(learner_state.params))
            checkpointer.save(timestep=t, unreplicated_learner_state={"params": payload}, episode_return=eval_return)
    if bool(config.arch.absolute_metric) and best_params is not None:
        abs_metrics = get_eval_fn(eval_env, act_fn, config, absolute_metric=True)(best_params, key, init_act_state)
        emit("ABSOLUTE", abs_metrics, t, len(timesteps) - 1)
    if logger is not None:
        logger.stop()
    return eval_return
