"""CPU: the entry points of the lean rollout - mava_rollout_ff_flags_f32, mava_rollout_expand_f32 and the two host-only
questions mava_ppo_{actor,critic}_grad_reads_input16 - are bound, refuse bad arguments on the host before any launch, and the
questions answer by the launchers' own rule (no GPU: nothing here launches)."""
import ctypes as C

import pytest

from mava_amd import _lib

NEW = ("mava_rollout_ff_flags_f32", "mava_rollout_expand_f32", "mava_ppo_actor_grad_reads_input16",
       "mava_ppo_critic_grad_reads_input16")


def test_new_symbols_are_bound_and_the_old_rollout_entry_point_stays():
    lib = _lib.lib()
    for name in NEW + ("mava_rollout_ff_f32",):
        assert name in _lib._SIGNATURES and hasattr(lib, name)
    old, new = _lib._SIGNATURES["mava_rollout_ff_f32"], _lib._SIGNATURES["mava_rollout_ff_flags_f32"]
    assert new == old[:-1] + [C.c_uint32, old[-1]], "the same arguments with flags in front of the stream"
    assert lib.mava_abi_version() == 4


def _rollout_args(flags, view16, state16, shared=1):
    """Arguments of mava_rollout_ff_flags_f32 for the headline shape with host memory behind every pointer: a call that is
    refused never reads through them."""
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf) & ~15
    rec = lambda on: [p, p] if on else [None, None]  # noqa: E731
    return ([p, 5, p, shared, 16, 4, 66, 3, 5, 1, 2, 0, 0, 0, 0] + [p] * 18 + [None, None, 0.99, 0.95] + [None] * 3
            + rec(state16) + rec(view16) + [flags, None]), buf


@pytest.mark.parametrize("flags,view16,state16,shared,msg", [
    (1, False, True, 1, b"MAVA_ROLLOUT_SKIP_AGENTS_VIEW needs view16"),
    (2, True, False, 1, b"MAVA_ROLLOUT_SKIP_GLOBAL_STATE needs state16"),
    (3, False, False, 1, b"needs view16"),
    (2, True, False, 0, b"MAVA_ROLLOUT_SKIP_GLOBAL_STATE needs state16"),
    (4, True, True, 1, b"unknown flags"),
])
def test_skip_bits_are_refused_without_their_records(flags, view16, state16, shared, msg):
    lib = _lib.lib()
    args, keep = _rollout_args(flags, view16, state16, shared)
    rc = lib.mava_rollout_ff_flags_f32(*args)
    assert rc <= -1000 and msg in lib.mava_last_error(), (rc, lib.mava_last_error())
    del keep


def test_expand_argument_errors():
    lib = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf) & ~15
    assert lib.mava_rollout_expand_f32(0, 4, 4, 66, p, p, p, None, None, None, 0, None) <= -1000 and b"bad shape" in lib.mava_last_error()
    assert lib.mava_rollout_expand_f32(3, 4, 4, 66, None, None, None, None, None, None, 0, None) <= -1000
    assert b"no record" in lib.mava_last_error()
    assert lib.mava_rollout_expand_f32(3, 4, 4, 66, p, p, None, None, None, None, 0, None) <= -1000
    assert b"go together" in lib.mava_last_error()
    assert lib.mava_rollout_expand_f32(3, 4, 4, 66, p, p + 2, p, None, None, None, 0, None) <= -1000 and b"alignment" in lib.mava_last_error()
    assert lib.mava_rollout_expand_f32(3, 4, 2, 65, None, None, None, p, p, p, 0, None) <= -1000 and b"A*O % 8" in lib.mava_last_error()
    assert lib.mava_rollout_expand_f32(3, 4, 4, 300, p, p, p, None, None, None, 0, None) <= -1000 and b"not supported" in lib.mava_last_error()
    # T = 1 has no slot between 0 and T: nothing to do, and nothing is launched
    assert lib.mava_rollout_expand_f32(1, 4, 4, 66, p, p, p, None, None, None, 1, None) == 0


def test_the_library_answers_the_launch_rule():
    """The headline shapes: actor on 70 inputs (view16 rows of 72 halves), the wide critic on 264 (state16), the decentralised
    critic on 70.  The answers follow what the launchers document in include/mava_hip.h."""
    lib = _lib.lib()
    x, r16 = 0x10000, 0x20000  # (addresses only: the questions never read through them)
    actor = lambda ctx, x=x, r=r16, ld=72: lib.mava_ppo_actor_grad_reads_input16(ctx, 70, 5, x, 4, r, ld)  # noqa: E731
    critic = lambda ctx, din=264, share=4, ld=0, x=x, r=r16: lib.mava_ppo_critic_grad_reads_input16(ctx, din, x, share, 4, r, ld)  # noqa: E731
    assert actor(None) == 0 and critic(None) == 0, "no handle: exact f32, no record is ever read"
    f32 = _lib.Ctx("f32")
    assert actor(f32.handle) == 0 and critic(f32.handle) == 0
    h = _lib.Ctx("f16x2")
    assert actor(h.handle) == 1 and critic(h.handle) == 1 and critic(h.handle, 70, 1, 72) == 1
    assert h.get(h.H2_LAUNCHES) == 0 and h.get(h.W8_LAUNCHES) == 0, "a question is not a launch"
    assert actor(h.handle, r=None) == 0 and critic(h.handle, r=None) == 0
    assert actor(h.handle, r=r16 + 8) == 0 and actor(h.handle, ld=70) == 0 and actor(h.handle, x=x + 4) == 0
    assert critic(h.handle, ld=272) == 0 and critic(h.handle, din=260) == 0 and critic(h.handle, x=x + 8) == 0
    assert critic(h.handle, 70, 4, 72) == 0, "a shared narrow input (aggregated): the eight-wave kernel does not take it"
    h.set(h.TRAIN_VARIANT, 1)  # four-wave kernels only: the actor has no record path there, the wide critic keeps its own
    assert actor(h.handle) == 0 and critic(h.handle) == 1 and critic(h.handle, 70, 1, 72) == 0
    h.set(h.TRAIN_VARIANT, 2)  # forced x_lo products: nobody reads a record
    assert actor(h.handle) == 0 and critic(h.handle) == 0
    h.set(h.TRAIN_VARIANT, 0)
    assert actor(h.handle) == 1
    assert lib.mava_ppo_actor_grad_reads_input16(h.handle, 0, 5, x, 4, r16, 72) <= -1000
    assert lib.mava_ppo_critic_grad_reads_input16(h.handle, 264, x, 0, 4, r16, 0) <= -1000
    h.close()
    f32.close()
