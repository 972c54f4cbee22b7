"""Minibatch time of rec_mappo on env=spread with a ContinuousActionHead, the actor's output path fused
(MAVA_REC_FUSED_OUT_CONTINUOUS=1: mava_rec_out_continuous_f32) against layer-wise, both in ONE process on the same rollout
shape, alternating blocks.  The two learners differ in nothing else, so the difference of the minibatch times is the
difference of the actor's output path.  The critic runs on the same stream here (MAVA_REC_OVERLAP=0) so that it cannot hide it.
    python tools/rec_out_continuous_timing.py [--envs 2048] [--rollout 32] [--out profiles/rec_out_continuous_timing.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--rollout", type=int, default=32)
    ap.add_argument("--scenario", default="spread-3a")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import rec_mappo

    dev = torch.device("cuda:0")
    os.environ["MAVA_MATMUL"], os.environ["MAVA_REC_OVERLAP"] = "f16x2", "0"
    learners = {}
    for name, switch in (("layerwise", "0"), ("fused", "1")):
        os.environ["MAVA_REC_FUSED_OUT_CONTINUOUS"] = switch
        cfg = compose("default_rec_mappo", ["env=spread", f"env/scenario={a.scenario}", "network=rnn", f"arch.num_envs={a.envs}",
                                            f"system.rollout_length={a.rollout}", "system.num_minibatches=2",
                                            "network.action_head._target_=mava.networks.ContinuousActionHead"])
        env, _ = envs.make(cfg, add_global_state=True, device=dev)
        L = rec_mappo.learner_setup(env, (42, 43, 44), cfg, device=dev)[0].learner
        assert L.fused_out_continuous == (switch == "1")
        L._rollout(0)
        L._bootstrap_and_gae()
        learners[name] = L
    perm = torch.arange(a.envs, device=dev, dtype=torch.int32)

    def block(L, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(n):
            L._minibatch(0, 0, i % 2, perm)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    times = {k: [] for k in learners}
    for r in range(a.rounds + 1):  # round 0 warms both up
        for k, L in learners.items():
            t = block(L, a.per_round)
            if r:
                times[k].append(t)
    L = learners["fused"]
    res = {"what": "ms per minibatch (actor + critic + Adam), rec_mappo env=spread continuous head, f16x2",
           "scenario": a.scenario, "envs": a.envs, "rollout": a.rollout, "rows_per_minibatch": L.T * L.Rm, "action_dim": L.nA,
           "blocks": times, "median_ms": {k: statistics.median(v) for k, v in times.items()}}
    res["fused_minus_layerwise_ms"] = res["median_ms"]["fused"] - res["median_ms"]["layerwise"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
