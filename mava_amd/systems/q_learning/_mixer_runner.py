"""What rec_qmix and rec_vdn share: the refusals and the experiment loop.  The loop is rec_iql's (rec_iql.py here, itself
mava/systems/q_learning/rec_iql.py:533-659) with the value-decomposition learner: MISC {timestep, epsilon}, ACT, TRAIN
(q_loss, mean_q, mean_target of Q_tot), EVAL with the greedy per-agent policy (the mixer takes no part in acting),
checkpoints of online / target, each {"q_network", "mixer"}, and ABSOLUTE with the best parameters."""
from __future__ import annotations

import copy
import time
from typing import Any, Callable, Dict, Optional

import torch

from ... import envs as environments
from ... import iql_learner as _iql
from ... import qmix_learner as _learner
from ...config import Config, check_total_timesteps
from ...learner import get_final_step_metrics
from ..ppo.anakin import _tree_clone, _tree_to, _unreplicate_n_dims
from . import rec_iql
from .types import QNetParams


def learner_setup(env, keys, config, mixer: str, device=None):
    config.system.mixer = mixer
    return _learner.learner_setup(env, keys, config, device)


def check_config(config: Config, mixer: str) -> None:
    """rec_iql's refusals (one device, update_batch_size == 1, the default Q-network torsos, an environment with a
    pre-reset observation), then the mixer's own keys."""
    rec_iql._check_config(config)
    s = config.system
    got = str(s.get("mixer", mixer))
    if got != mixer:
        raise ValueError(f"rec_{mixer} runs system.mixer={mixer}, got {got!r} (the other system is rec_{got})")
    if mixer == "qmix":
        em, hh = int(s.get("mixer_embed_dim", 32)), int(s.get("hypernet_hidden_dim", 64))
        if not 1 <= em <= _learner.MAX_EMBED or hh < 1:
            raise ValueError(f"system.mixer_embed_dim must be in [1, {_learner.MAX_EMBED}] and system.hypernet_hidden_dim >= 1, "
                             f"got {em} and {hh}")


def run_experiment(_config: Config, mixer: str, log: Optional[Callable[[Dict[str, Any]], None]] = None) -> float:
    config = copy.deepcopy(_config)
    check_config(config, mixer)
    config.arch.n_devices = 1
    config = check_total_timesteps(config, 1)
    s = config.system
    steps_per_rollout = int(s.total_timesteps // config.arch.num_evaluation)
    act_steps = int(config.arch.num_envs) * int(s.rollout_length)
    s.num_updates_per_eval = max(1, steps_per_rollout // act_steps)

    env, eval_env = environments.make(config)
    seed = int(s.seed)
    key, q_key, key_e = seed, seed + 1, seed + 2
    learn, q_network, learner_state = learner_setup(env, (key, q_key), config, mixer)

    from ...evaluator import get_eval_fn, make_rec_eval_act_fn
    from ...utils.logger import LogEvent, MavaLogger

    act_fn = make_rec_eval_act_fn(q_network.apply, config)  # reads params["q_network"]: greedy per-agent actions
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
        ep_metrics, ep_completed = get_final_step_metrics(out.episode_metrics)
        ep_metrics = dict(ep_metrics)
        ep_metrics["steps_per_second"] = steps_per_rollout / elapsed
        emit("MISC", {"timestep": t, "epsilon": _iql.epsilon(t, s.eps_min, s.eps_decay)}, t, eval_idx)
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
        if checkpointer is not None:  # online + target, each {"q_network", "mixer"}; the replay buffer is not checkpointed
            p = _unreplicate_n_dims(learner_state.params)
            checkpointer.save(timestep=t, unreplicated_learner_state={"params": QNetParams(p.online, p.target)._asdict()},
                              episode_return=eval_return)
    if bool(config.arch.absolute_metric) and best_params is not None:
        abs_metrics = get_eval_fn(eval_env, act_fn, config, absolute_metric=True)(best_params, key, init_act_state)
        emit("ABSOLUTE", abs_metrics, t, n_evals - 1)
    if logger is not None:
        logger.stop()
    return eval_return
