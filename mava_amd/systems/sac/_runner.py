"""What ff_isac and ff_masac share: mava/systems/sac/ff_isac.py:491-602 (run_experiment), which ff_masac.py repeats with
add_global_state=True and the centralised Q network."""
from __future__ import annotations

import copy
import time
from typing import Any, Callable, Dict, Optional

import torch

from ... import envs as environments
from ... import sac_learner as _learner
from ...config import Config, check_total_timesteps
from ...learner import get_final_step_metrics
from ..ppo.anakin import _tree_clone, _tree_to, _unreplicate_n_dims


def check_config(config: Config, name: str) -> None:
    """Refusals that need no environment or device (the learner repeats them with its own context)."""
    import torch.distributed as dist

    from ...generic_networks import CNNTorso, torso_from_config

    s = config.system
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{name} runs on one device (multi-GPU is not implemented)")
    if int(s.update_batch_size) != 1:
        raise NotImplementedError(f"{name} supports update_batch_size == 1 only")
    head = str((config.network.get("action_head", None) or {}).get("_target_", "DiscreteActionHead"))
    if not head.endswith("ContinuousActionHead"):
        raise ValueError(f"{name} needs a ContinuousActionHead (network=continuous_mlp), got {head}")
    if isinstance(torso_from_config(config.network.critic_network.pre_torso), CNNTorso):
        raise NotImplementedError(f"{name}: a CNN critic torso cannot read [state | action] rows (use an MLPTorso)")
    if config.env.get("env_name", None) != "Spread":
        raise ValueError(f"{name} needs an environment with continuous actions that returns its pre-reset observation "
                         f"(env=spread); {config.env.get('env_name', None)} is not one")


def run_experiment(_config: Config, centralised: bool, log: Optional[Callable[[Dict[str, Any]], None]] = None) -> float:
    name = "ff_masac" if centralised else "ff_isac"
    config = copy.deepcopy(_config)
    check_config(config, name)
    config.arch.n_devices = 1
    config = check_total_timesteps(config, 1)
    s = config.system
    # :496-503: env steps per evaluation interval and the update steps that take them
    steps_per_rollout = int(s.total_timesteps // config.arch.num_evaluation)
    anakin_act_steps = int(config.arch.num_envs) * int(s.rollout_length)
    s.scan_steps = s.num_updates_per_eval = max(1, int(steps_per_rollout / anakin_act_steps))

    env, eval_env = environments.make(config, add_global_state=centralised)
    seed = int(s.seed)
    keys = [seed + i for i in range(7)]  # stands in for the reference's key splits (:104, :185, :512)
    learn, actor_network, learner_state = _learner.learner_setup(env, keys[:6], config, centralised)

    from ...evaluator import get_eval_fn, make_ff_eval_act_fn
    from ...utils.logger import LogEvent, MavaLogger

    act_fn = make_ff_eval_act_fn(actor_network.apply, config)
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
        learner_state = learner_state._replace(params=_tree_to(restored, eval_env.device))  # learn() adopts them

    logger = MavaLogger(config) if log is None else None

    def emit(event: str, rec: Dict[str, Any], t: int, idx: int) -> None:
        if logger is not None:
            logger.log(rec, t, idx, getattr(LogEvent, event))
        else:
            out = {k: (float(v.float().mean()) if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}
            log({"event": event, "timestep": t, **out})

    # :526-537: fill the buffer with random actions
    torch.cuda.synchronize()
    start = time.time()
    metrics = learn.explore()
    torch.cuda.synchronize()
    t = learn.learner.t
    emit("MISC", {"step": t}, t, 0)
    final_metrics, _ = get_final_step_metrics(metrics)
    final_metrics = dict(final_metrics)
    final_metrics["steps_per_second"] = t / max(time.time() - start, 1e-9)
    emit("ACT", final_metrics, int(s.explore_steps), 0)

    eval_return, max_return, best_params = 0.0, -float("inf"), None
    n_evals = int(config.arch.num_evaluation)
    for eval_idx in range(n_evals):
        torch.cuda.synchronize()
        start = time.time()
        out = learn(learner_state)
        torch.cuda.synchronize()
        elapsed = time.time() - start
        learner_state = out.learner_state
        t = int(s.explore_steps) + steps_per_rollout * (eval_idx + 1)  # :542-547
        ep_metrics, ep_completed = get_final_step_metrics(out.episode_metrics)
        ep_metrics = dict(ep_metrics)
        ep_metrics["steps_per_second"] = steps_per_rollout / elapsed
        emit("MISC", {"timestep": t}, t, eval_idx)
        if ep_completed:
            emit("ACT", ep_metrics, t, eval_idx)
        emit("TRAIN", {**out.train_metrics, "log_alpha": learner_state.params.log_alpha}, t, eval_idx)  # :556-561
        eval_params = _tree_clone(learner_state.params.actor)
        eval_metrics = evaluator(eval_params, keys[6] + eval_idx, {})
        emit("EVAL", eval_metrics, t, eval_idx)
        eval_return = float(eval_metrics["episode_return"].float().mean())
        if bool(config.arch.absolute_metric) and max_return <= eval_return:
            best_params, max_return = eval_params, eval_return
        if checkpointer is not None:  # SacParams; the replay buffer is not checkpointed
            p = _unreplicate_n_dims(learner_state.params)
            checkpointer.save(timestep=t, unreplicated_learner_state={"params": {"actor": p.actor, "q": {
                "online": p.q.online._asdict(), "targets": p.q.targets._asdict()}, "log_alpha": p.log_alpha}},
                episode_return=eval_return)
    if bool(config.arch.absolute_metric) and best_params is not None:
        abs_metrics = get_eval_fn(eval_env, act_fn, config, absolute_metric=True)(best_params, keys[0], {})
        emit("ABSOLUTE", abs_metrics, t, n_evals - 1)
    if logger is not None:
        logger.stop()
    return eval_return
