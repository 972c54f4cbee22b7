"""mava_rollout_ff_flags_f32's skip bits and mava_rollout_expand_f32 (csrc/rollout_h2.hip), kernel level: for every case a full
launch (flags 0) and a lean launch run from identical inputs into separate buffers.  The lean launch's f32 agents_view /
global_state are prefilled with a finite sentinel and followed by guard words: a skipped array keeps the sentinel in slots
1 .. T - 1 - the launch did not touch the bytes - slot T and every other output, both records and both words have the full
launch's bits, and the expand kernel turns the records back into the full launch's f32 arrays.  Launches are compared with
each other, bit for bit: no tolerance anywhere."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rollout_model as M

pytestmark = pytest.mark.gpu

SENT, GUARD, NG = -12345.5, 7.25, 64  # sentinel of the skipped slots; value and count of the guard words behind each f32 array
AV, GS = 1, 2  # ops.ROLLOUT_SKIP_AGENTS_VIEW / _GLOBAL_STATE


def _mk(name, shared, A, O, E, T, inst):
    return M.Case(name, shared, A, O, 5, E, inst, t0=3, row_offset=1037, env_offset=148, reward_mode=1,
                  policy_seed=(0x1234ABCD << 32) | 42, env_seed=(0x9E3779B9 << 32) | 7, T=T, time_limit=3)


# the headline instance at one full block and at a partial second block, T = 1 (no slot between 0 and T), 2 and 3; the
# two-agent instance (O = 66: the tiny-2ag shape, A * O % 8 != 0 and so no state record: bit 0 only; O = 64: both records);
# the decentralised instance (no global state: bit 0 only)
CASES = [(_mk(f"s-A4-O66-E{E}-T{T}", True, 4, 66, E, T, 805171), (AV, GS, AV | GS)) for E in (16, 24) for T in (1, 2, 3)]
CASES += [(_mk("s-A2-O66-E32-T3", True, 2, 66, 32, 3, 805091), (AV,)), (_mk("s-A2-O64-E32-T3", True, 2, 64, 32, 3, 805091), (AV, GS, AV | GS)),
          (_mk("d-A4-O66-E24-T3", False, 4, 66, 24, 3, 805050), (AV,))]
PARAMS = [pytest.param(c, f, id=f"{c.name}-flags{f}") for c, fl in CASES for f in fl]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    """(array, guard): a contiguous f32 array of `shape` full of SENT with NG guard words right behind it."""
    n = int(np.prod(shape))
    flat = torch.full((n + NG,), SENT, device=dev)
    flat[n:] = GUARD
    return flat[:n].view(shape), flat[n:]


def _launch(dev, c, init, flags, records=(True, True)):
    """One launch.  Returns (outputs, guards): every buffer the launch may write, as tensors."""
    from mava_amd import ops

    E, A, T, W, AO, nA = c.E, c.A, c.T, c.A + c.O, c.A * c.O, c.nA
    f = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)  # noqa: E731
    av, g_av = _guarded((T + 1, E, A, W), dev)
    gs, g_gs = _guarded((T + 1, E, 1, AO), dev) if c.shared else (None, None)
    b = dict(agents_view=av, global_state=gs, action_mask=f((T + 1, E, A, nA), torch.uint8, 0xAB),
             obs_step_count=f((T + 1, E, A), torch.int32, -7), action=f((T, E, A), torch.int32, -7), value=f((T, E, A), torch.float32, SENT),
             reward=f((T, E, A), torch.float32, SENT), log_prob=f((T, E, A), torch.float32, SENT), done=f((T, E, A), torch.uint8, 0xAB),
             last_val=f((E, A), torch.float32, SENT), info_return=f((T, E), torch.float32, SENT), info_length=f((T, E), torch.int32, -7),
             info_terminal=f((T, E), torch.uint8, 0xAB), adv=f((T, E, A), torch.float32, SENT), tgt=f((T, E, A), torch.float32, SENT),
             last_reward=f((E, A), torch.float32, SENT), last_done=f((E, A), torch.uint8, 0xAB), step_counter=f((1,), torch.int32, 11))
    if records[0]:
        b.update(view16=f((T + 1, E, A, 8 * ((W + 8) // 8)), torch.float16, -3.0), view16_valid=f((1,), torch.int32, 0))
    if records[1] and c.shared and AO % 8 == 0:
        b.update(state16=f((T + 1, E, 1, AO), torch.float16, -3.0), state16_valid=f((1,), torch.int32, 0))
    av[0] = _t(np.asarray(init["agents_view"], np.float32), dev)
    if c.shared:
        gs[0] = _t(np.asarray(init["global_state"], np.float32), dev).view(E, 1, AO)
    b["action_mask"][0] = _t(np.asarray(init["action_mask"]).astype(np.uint8), dev)
    b["obs_step_count"][0] = _t(np.asarray(init["step_count"], np.int32), dev)
    st = SimpleNamespace(**{k: _t(init[k], dev).clone() for k in ("step_count", "run_return", "run_length", "ep_return", "ep_length")})
    pa, pc = (_t(p, dev) for p in M.case_params(c))
    ok = ops.rollout_ff(pa, pc, n_actions=nA, critic_shared=c.shared, E=E, A=A, O=c.O, T=T, time_limit=c.time_limit,
                        policy_seed=c.policy_seed, env_seed=c.env_seed, t0=c.t0, row_offset=c.row_offset, env_offset=c.env_offset,
                        reward_mode=c.reward_mode, env_state=st, gamma=M.GAMMA, gae_lambda=M.LAMBDA,
                        skip_agents_view=bool(flags & AV), skip_global_state=bool(flags & GS), **b)
    torch.cuda.synchronize()
    assert ok, f"{c.name}: the fused rollout does not instantiate this shape"
    out = {k: v for k, v in b.items() if v is not None}
    out.update({f"state.{k}": v for k, v in vars(st).items()})
    return out, {"agents_view": g_av, "global_state": g_gs}


_FULL = {}


def _full(dev, c, init, key=None):
    """The full launch of a case, run once and shared by its flag variants (nobody writes into it)."""
    key = key or c.name
    if key not in _FULL:
        from mava_amd._lib import lib

        _FULL[key] = _launch(dev, c, init, 0)[0]
        assert lib().mava_debug_rollout_last_instance() == c.inst
    return _FULL[key]


def _expand(out, force):
    from mava_amd import ops

    ops.rollout_expand(out["agents_view"], out["view16"], out["view16_valid"], out.get("global_state") if "state16" in out else None,
                       out.get("state16"), out.get("state16_valid"), force=force)
    torch.cuda.synchronize()


def _check_lean(c, full, lean, guards, flags, words=(1, 1)):
    T = c.T
    for k, v in full.items():
        if k in ("agents_view", "global_state"):
            continue
        assert torch.equal(lean[k], v), f"{c.name} flags {flags}: {k} differs from the full launch"
    assert int(lean["view16_valid"].item()) == words[0]
    if "state16_valid" in lean:
        assert int(lean["state16_valid"].item()) == words[1]
    for k, bit in (("agents_view", AV), ("global_state", GS)):
        if k not in full:
            continue
        assert torch.equal(lean[k][0], full[k][0]) and torch.equal(lean[k][T], full[k][T]), f"{c.name}: slots 0 and T of {k}"
        if flags & bit:
            assert bool((lean[k][1:T] == SENT).all()), f"{c.name}: a skipped slot of {k} was written"
        else:
            assert torch.equal(lean[k], full[k]), f"{c.name}: {k} (not skipped)"
        assert bool((guards[k] == GUARD).all()), f"{c.name}: the guard words behind {k}"


@pytest.mark.parametrize("c,flags", PARAMS)
def test_lean_launch_skips_only_the_inner_f32_slots(dev, c, flags):
    from mava_amd._lib import lib

    init = M.case_init(c)
    full = _full(dev, c, init)
    lean, guards = _launch(dev, c, init, flags)
    assert lib().mava_debug_rollout_last_instance() == c.inst
    _check_lean(c, full, lean, guards, flags)
    # the environment's own observations are exact in f16: both words are 1 and the conditional expand leaves the sentinel
    _expand(lean, force=False)
    _check_lean(c, full, lean, guards, flags)
    # forced: the records converted are the full launch's f32 arrays, in every slot
    _expand(lean, force=True)
    for k in ("agents_view", "global_state"):
        if k in full:
            assert torch.equal(lean[k], full[k]), f"{c.name} flags {flags}: {k} after the forced expand"
            assert bool((guards[k] == GUARD).all()), f"{c.name}: the guard words behind {k} after the expand"


@pytest.mark.parametrize("where", ["agents_view", "global_state"])
def test_low_term_in_slot0_clears_the_word_and_the_conditional_expand_repairs(dev, where):
    """0.1 (not exact in f16) in one slot-0 element of one array: that array's word ends 0 - the gradient kernels will read its
    f32 record - and the conditional expand rebuilds exactly that array; the other keeps word 1 and its sentinel."""
    c = CASES[5][0]  # s-A4-O66-E24-T3
    assert (c.E, c.T) == (24, 3)
    init = dict(M.case_init(c))
    init[where] = np.array(init[where], np.float32)
    per_env = init[where].size // c.E
    init[where].reshape(-1)[17 * per_env + 7] = 0.1  # (environment 17: the partial second block's)
    full = _full(dev, c, init, key="planted-" + where)
    words = (0, 1) if where == "agents_view" else (1, 0)
    assert (int(full["view16_valid"].item()), int(full["state16_valid"].item())) == words
    lean, guards = _launch(dev, c, init, AV | GS)
    _check_lean(c, full, lean, guards, AV | GS, words)
    _expand(lean, force=False)
    other = "global_state" if where == "agents_view" else "agents_view"
    assert torch.equal(lean[where], full[where]), f"{where}: the conditional expand with the word at 0"
    assert bool((lean[other][1 : c.T] == SENT).all()), f"{other}: its word is 1, the conditional expand must leave it alone"
    for k in guards:
        assert bool((guards[k] == GUARD).all())


def test_skip_without_its_record_is_refused_before_the_launch(dev):
    from mava_amd._lib import MavaHipError

    c = CASES[5][0]
    init = M.case_init(c)
    for flags, records, what in ((AV, (False, True), "view16"), (GS, (True, False), "state16")):
        with pytest.raises(MavaHipError, match=what):
            _launch(dev, c, init, flags, records)
    d = CASES[-1][0]  # decentralised: there is no state record to skip by
    with pytest.raises(MavaHipError, match="state16"):
        _launch(dev, d, M.case_init(d), GS)


# ------------------------------------------------------------------------------------------------ the expand kernel alone
# (T, E, A, O): rows that are no multiple of the 64-row tile, a destination that is not 16-byte aligned at slot 1 (E * A * (A + O)
# % 4 != 0: the one-float stores), more tiles than the launch has blocks (the grid-stride loop), the widest record row
EXPAND_SHAPES = [(3, 24, 4, 66), (2, 33, 2, 13), (4, 5, 1, 70), (3, 16400, 4, 12), (3, 9, 8, 35)]


@pytest.mark.parametrize("T,E,A,O", EXPAND_SHAPES)
@pytest.mark.parametrize("force", [True, False])
def test_expand_converts_the_records(dev, T, E, A, O, force):
    from mava_amd import ops

    W, AO = A + O, A * O
    RP = 8 * ((W + 8) // 8)
    g = torch.Generator(device="cpu").manual_seed(T * 1000 + E)
    v16 = (torch.randint(-40, 40, (T + 1, E, A, RP), generator=g).float() / 8).half().to(dev)
    with_state = AO % 8 == 0
    s16 = (torch.randint(-40, 40, (T + 1, E, 1, AO), generator=g).float() / 8).half().to(dev) if with_state else None
    av, g_av = _guarded((T + 1, E, A, W), dev)
    gs, g_gs = _guarded((T + 1, E, 1, AO), dev) if with_state else (None, None)
    # conditional: agents_view's word says "not valid" (rebuilt), the state's says valid (left alone)
    wv, ws = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    ops.rollout_expand(av, v16, wv, gs, s16, ws if with_state else None, force=force)
    torch.cuda.synchronize()
    assert bool((av[0] == SENT).all()) and bool((av[T] == SENT).all()), "slots 0 and T are not the expand's"
    assert torch.equal(av[1:T], v16[1:T, :, :, :W].float())
    assert bool((g_av == GUARD).all())
    if with_state:
        assert bool((gs[0] == SENT).all()) and bool((gs[T] == SENT).all())
        assert torch.equal(gs[1:T], s16[1:T].float()) if force else bool((gs == SENT).all())
        assert bool((g_gs == GUARD).all())
