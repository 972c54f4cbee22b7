"""GPU: the continuous actor's fused output path (mava_rec_out_continuous_f32, csrc/rec_out_h2.hip) against float64
(seq_model.out_path around continuous_loss) at six tiles, both instances and their edges, 1 | 4 | 6 slabs; its refusals; one RecLearner
minibatch on env=spread, switched on against layer-wise.  Bounds: 1e-4 gradients, 1e-5 loss sums; a case whose float32 NumPy loss head
(seq_model.cont_f32_error) lies beyond a quarter of 1e-4 takes four times that floor: 8.3e-7 at 1 dimension, which keeps 1e-4; 3.28e-5 |
2.82e-5 | 3.65e-5 at 8 | 9 | 16 dimensions (either row offset), which take 1.31e-4 | 1.13e-4 | 1.46e-4.  Whole tiles only (Rm % 32 == 0): no rows to pad."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import tanh_normal as tn
from tests import seq_model as sm
from tests.conftest import assert_close
from tests.test_gpu_seq_kernels import SENT, H, _bits, _d, _L, _out, _take

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def case(dim, row_offset):
    c = dict(sm.cont_case(dim, False, row_offset))
    rows = lambda x: sm.gather_rows(x, c["idx"], c["A"], c["Rm"]).reshape(-1)
    for draw in range(64):  # as seq_model.out_case: the first draw clear of relu's kink and of the clip boundaries
        rng = np.random.default_rng([7000 + dim, draw])
        p, hs = sm.out_params(rng, dim, 0.1), sm.f32(rng.standard_normal((c["R"], H)) * 0.5)
        mean = sm.out_forward(hs, p)
        lp = tn.log_prob_terms(c["action_rows"], mean, np.broadcast_to(tn.scale_of(sm.f64(c["raw"])), mean.shape))[0].sum(-1)
        old = np.zeros_like(c["old_lp"])
        old.reshape(c["T"], -1)[:, sm.ext_index(c["idx"], c["E"], c["A"], c["Rm"])] = (lp + rng.standard_normal(c["R"]) * 0.25).reshape(c["T"], -1)
        edge = np.abs(np.abs(np.exp(lp - sm.f64(rows(old))) - 1.0) - sm.CLIP).min()
        if np.abs(sm.out_pre(hs, p)).min() >= sm.RELU_CLEAR and edge >= sm.CLIP_CLEAR:
            break
    assert draw < 63, "no draw clear of the kinks"
    c.update(params=p, hs=hs, mean=mean, old_lp=old, old_lp_rows=rows(old))
    def loss_fn(y):
        la, ent, c["dmean"], c["draw"] = sm.continuous_loss(y, c["raw"], c["action_rows"], c["old_lp_rows"], c["adv_rows"], c["eps"])
        return (la, ent), c["dmean"]
    c["losses"], c["grads"] = sm.out_path(hs, p, loss_fn)
    c["bound"] = max(1e-4, 4.0 * sm.cont_f32_error(c))  # from the reference alone
    return c


def launch(dev, c, n_slab, dim=None, short=0):
    """(rc, dh, slabs (n_slab, needed)); the slab tails and the guard tiles behind both buffers must keep their sentinel."""
    L, check, ptr, s = _L()
    dim = c["dim"] if dim is None else dim
    need = H * H + H + H * dim + dim + 2 + dim
    stats = sm.adv_stats(c["adv_rows"])
    t = [_d(a, dev) for a in (c["idx"], sm.to_t32(c["hs"]), sm.out_flat(c["params"]), c["raw"], c["action"], c["old_lp"], c["adv"], stats)]
    dh, slab = _out(c["R"] * H, H, dev), _out(n_slab * (need + 8), 1, dev)
    rc = L.mava_rec_out_continuous_f32(c["T"], c["Rm"], c["E"], c["A"], dim, tn.MIN_SCALE, *(ptr(x) for x in t), stats.shape[0], sm.CLIP,
                                       sm.ENT_COEF, sm.SEED, c["ent_step"], c["row_offset"], sm.GRAD_SCALES[1], ptr(dh), ptr(slab), need + 8 - short * 9, n_slab, s)
    slab_ = _take(slab, n_slab * (need + 8), "slab").reshape(n_slab, need + 8)
    assert (slab_[:, need:] == np.float32(SENT)).all(), "the tail of every slab row must stay untouched"
    return rc, _take(dh, c["R"] * H, "dh"), slab_[:, :need]


@pytest.mark.parametrize("row_offset", sm.ROW_OFFSETS)
@pytest.mark.parametrize("dim", sm.CONT_DIMS)
def test_kernel_matches_float64(dev, dim, row_offset):
    c = case(dim, row_offset)
    g = dict(c["grads"], losses=np.array(c["losses"]), dlog_std=c["draw"])
    for n_slab in sm.OUT_SLABS:
        rc, dh, slab = launch(dev, c, n_slab)
        assert rc == 0
        if n_slab == 4:  # the same launch again: bit for bit
            [_bits(a, b, "second launch") for a, b in zip(launch(dev, c, n_slab)[1:], (dh, slab))]
        tot, o = slab.astype(np.float64).sum(0), 0
        assert_close(sm.from_t32(dh, c["R"], H) / sm.GRAD_SCALES[1], g["dh"], c["bound"], f"dh ({n_slab} slabs)")
        for name, k in (("dWpost", H * H), ("dbpost", H), ("dWhead", H * dim), ("dbhead", dim), ("losses", 2), ("dlog_std", dim)):
            tol, scale = (1e-5, 1.0) if name == "losses" else (c["bound"], None)
            assert_close(tot[o : o + k], g[name].reshape(-1), tol, f"{name} ({n_slab} slabs)", scale=scale)
            o += k


@pytest.mark.parametrize("dim,n_slab,short,want", [(17, 1, 0, 1), (16, 7, 0, 1), (16, 1, 1, -1002)], ids=["17-dims", "7-slabs", "short-stride"])
def test_refusals(dev, dim, n_slab, short, want):  # 1: not instantiated; -1002: the argument error of slab_stride; nothing is launched
    rc, dh, slab = launch(dev, case(16, 0), n_slab, dim, short)
    assert rc == want and (dh == np.float32(SENT)).all() and (slab == np.float32(SENT)).all()


def test_learner_switch(dev, monkeypatch):
    """rec_mappo on spread-2a, f16x2: fused against layer-wise at conftest.check_and_sync_f16x2_state's allowance (<= 12 entries beyond 1e-4, none 1e-3)."""
    from mava_amd import envs
    from mava_amd.config import compose
    from mava_amd.systems.ppo import rec_mappo

    monkeypatch.setenv("MAVA_MATMUL", "f16x2")
    grads = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("MAVA_REC_FUSED_OUT_CONTINUOUS", switch)
        cfg = compose("default_rec_mappo", ["env=spread", "env/scenario=spread-2a", "network=rnn", "arch.num_envs=16", "system.rollout_length=4",
                                            "system.num_minibatches=1", "network.action_head._target_=mava.networks.ContinuousActionHead"])
        L = rec_mappo.learner_setup(envs.make(cfg, add_global_state=True, device=dev)[0], (42, 43, 44), cfg, device=dev)[0].learner
        assert L.fused_out_continuous == (switch == "1") and not L.fused_out
        monkeypatch.setattr(L, "_clip_adam", lambda n, k, mb: None)  # keep the raw gradient of the first minibatch
        L._rollout(0), L._bootstrap_and_gae(), L._minibatch(0, 0, 0, torch.arange(L.E, device=dev, dtype=torch.int32))
        torch.cuda.synchronize()
        grads[switch] = L.g[: L.P].cpu().numpy().astype(np.float64), L.actor_network.log_std(L.g[: L.Pa]).cpu().numpy()
    (got, ls), (want, ls_ref) = grads["1"], grads["0"]
    assert np.count_nonzero(ls) == ls.size and np.count_nonzero(ls_ref) == ls.size
    assert_close(ls, ls_ref, 1e-4, "log_std gradient")
    assert (np.abs(got - want) > 1e-4 * (np.abs(want) + np.sqrt(np.mean(want * want)))).sum() <= 12
    assert_close(got, want, 1e-3, "flat gradient (hard bound)")
