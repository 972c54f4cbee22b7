"""What ff_isac and ff_masac share: the refusals and their spec for the experiment loop of mava_amd/systems/off_policy.py
(mava/systems/sac/ff_isac.py:491-602, which ff_masac.py repeats with add_global_state=True and the centralised Q network)."""
from __future__ import annotations

from ... import sac_learner as _learner
from ...config import Config
from .. import off_policy


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


def _eval_act(actor_network, config: Config, eval_env):
    from ...evaluator import make_ff_eval_act_fn

    return make_ff_eval_act_fn(actor_network.apply, config), {}


def spec(centralised: bool) -> off_policy.Spec:
    name = "ff_masac" if centralised else "ff_isac"

    def setup(env, config: Config):
        s = config.system
        s.scan_steps = s.num_updates_per_eval  # :496-503: the update steps of one evaluation interval
        # seed .. seed + 5 | evaluations from seed + 6: stands in for the reference's key splits (:104, :185, :512)
        keys = [int(s.seed) + i for i in range(7)]
        return (*_learner.learner_setup(env, keys[:6], config, centralised), (keys[0], keys[6]))

    return off_policy.Spec(
        name=name, check_config=lambda config: check_config(config, name), add_global_state=centralised, setup=setup,
        eval_act=_eval_act, eval_params=lambda params: params.actor, misc=lambda config, t: {},
        train_extra=lambda state: {"log_alpha": state.params.log_alpha},  # :556-561
        checkpoint_payload=lambda p: {"actor": p.actor, "q": {"online": p.q.online._asdict(), "targets": p.q.targets._asdict()},
                                      "log_alpha": p.log_alpha},  # SacParams
        explore_steps=lambda config: int(config.system.explore_steps))
