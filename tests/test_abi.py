"""CPU: the C-ABI library loads and exports every symbol include/mava_hip.h declares, and the ctypes table of
mava_amd/_lib.py states every prototype of that header argument by argument (no compute)."""
import ctypes as C
import os
import re

from mava_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mava_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mava_[a-z0-9_]+)\s*\(", text)))


_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "long": C.c_long, "float": C.c_float, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "size_t": C.c_uint64}
# the entry points that were folded into their neighbours by ABI version 4
FOLDED = ("mava_rollout_ff_tail_f32", "mava_rollout_ff_x16_f32", "mava_rollout_ff_records16_f32", "mava_ppo_actor_grad_x16_f32",
          "mava_ppo_critic_grad_x16_f32", "mava_lbf_step_real_next", "mava_rware_step_real_next",
          "mava_connector_step_real_next", "mava_cleaner_step_real_next", "mava_smax_step_real_next",
          "mava_spread_step_real_next")


def _header_prototypes():
    """name -> (return type, [parameter type]) of every prototype in the header, as C type strings without names:
    "ptr" for any pointer and for mava_stream_t, else the scalar's type name."""
    text = open(os.path.join(ROOT, "include", "mava_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def ctype(decl, named):
        words = decl.replace("*", " * ").split()
        if "*" in words or "mava_stream_t" in words:
            return "ptr"
        words = [w for w in words if w != "const"]
        if named:
            words = words[:-1]  # the parameter's name
        assert len(words) == 1, decl
        return words[0]

    protos = {}
    for ret, name, params in re.findall(r"^([\w \*]+?)\s*\b(mava_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        protos[name] = (ctype(ret, False), [] if params == "void" else [ctype(q, True) for q in params.split(",")])
    return protos


def _table_mismatches(protos, signatures, restypes):
    """The names whose ctypes entry does not state the header's prototype, each with what differs."""
    bad = {}

    def same(c, t):
        if c == "ptr":
            return t is C.c_void_p or t is C.c_char_p or (isinstance(t, type) and issubclass(t, C._Pointer))
        return t is _SCALARS[c]

    for name, (ret, params) in protos.items():
        if name == "mava_last_error":  # bound by hand in _lib.lib(): no arguments
            args = []
        elif name not in signatures:
            bad[name] = "no entry"
            continue
        else:
            args = signatures[name]
        if len(args) != len(params):
            bad[name] = f"{len(args)} arguments, the header has {len(params)}"
            continue
        wrong = [i for i, (c, t) in enumerate(zip(params, args)) if not same(c, t)]
        if wrong:
            bad[name] = f"argument {wrong[0]} is {args[wrong[0]].__name__}, the header has {params[wrong[0]]}"
        elif not same(ret, restypes.get(name, C.c_int)):
            bad[name] = f"return type {restypes.get(name, C.c_int).__name__}, the header has {ret}"
    for name in signatures:
        if name not in protos:
            bad[name] = "not in the header"
    return bad


def test_binding_table_states_every_prototype():
    protos = _header_prototypes()
    assert sorted(protos) == _header_symbols() and len(protos) >= 80
    assert _table_mismatches(protos, _lib._SIGNATURES, _lib._RESTYPES) == {}
    # the check can fail: an argument dropped from one entry, then an int / float pair swapped in another
    name = "mava_rollout_ff_f32"
    short = dict(_lib._SIGNATURES, **{name: _lib._SIGNATURES[name][:-1]})
    assert list(_table_mismatches(protos, short, _lib._RESTYPES)) == [name]
    name = "mava_ppo_critic_grad_f32"
    args = list(_lib._SIGNATURES[name])
    i = next(k for k in range(len(args) - 1) if args[k] is C.c_int and args[k + 1] is C.c_float)
    args[i], args[i + 1] = args[i + 1], args[i]
    swapped = dict(_lib._SIGNATURES, **{name: args})
    bad = _table_mismatches(protos, swapped, _lib._RESTYPES)
    assert list(bad) == [name] and f"argument {i} is c_float, the header has int" in bad[name]
    # a wrong return type is seen too
    assert list(_table_mismatches(protos, _lib._SIGNATURES, {})) == sorted(_lib._RESTYPES, key=list(protos).index)


def test_folded_entry_points_are_gone():
    lib = _lib.lib()
    assert len(FOLDED) == 11
    for gone in FOLDED:
        assert not hasattr(lib, gone), gone
        assert gone not in _lib._SIGNATURES


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    syms = _header_symbols()
    assert len(syms) >= 14
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in mava_hip.h but not exported by libmavahip.so"
    assert lib.mava_abi_version() == 4


def test_python_binding_matches_header():
    assert _header_symbols() == _lib.declared_symbols()


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.lib()
    # rejected on the host before any launch
    rc = lib.mava_gae_f32(None, None, None, None, None, None, -1, 4, 0.99, 0.95, None, None, None)
    assert rc <= -1000
    assert b"negative shape" in lib.mava_last_error()
    assert lib.mava_mlp_param_count(70, 5) == 26245 and lib.mava_mlp_param_count(264, 1) == 50561
    rc = lib.mava_mlp_forward_f32(None, None, 70, 99, None, 1, 8, None, None)
    assert rc <= -1000


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch

    from mava_amd import ops

    r = torch.zeros(4, 8)
    with pytest.raises(_lib.MavaHipError):
        ops.gae(r, r.clone(), torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(8), 0.99, 0.95)


def test_comm_abi_argument_errors():
    """mava_comm_* (csrc/comm.cpp): argument checks run before RCCL is touched."""
    lib = _lib.lib()
    assert lib.mava_comm_create(None, 0, 1, None) <= -1000
    h = C.c_void_p()
    idb = (C.c_uint8 * 128)()
    assert lib.mava_comm_create(C.byref(h), 3, 2, idb) <= -1000 and b"rank 3 of 2" in lib.mava_last_error()
    assert lib.mava_allreduce_sum_f32(None, None, 4, None) <= -1000
    assert lib.mava_comm_destroy(None) == 0


def test_permutation_abi_argument_errors():
    """mava_permutation_i32: range and pointer checks come before the launch."""
    lib = _lib.lib()
    assert lib.mava_permutation_i32(0, 1, 0, None, None) <= -1000 and b"n=0" in lib.mava_last_error()
    assert lib.mava_permutation_i32(1 << 31, 1, 0, None, None) <= -1000
    assert lib.mava_permutation_i32(8, 1, 0, None, None) <= -1000 and b"null pointer" in lib.mava_last_error()


def test_context_handles_are_independent():
    """mava_ctx_*: settings live in handles, not in the process - two handles (two learners) keep their own values, and a
    NULL handle means the defaults."""
    a, b = _lib.Ctx("f16x2"), _lib.Ctx("f32", critic_aggregation=False)
    assert a.matmul_mode == "f16x2" and b.matmul_mode == "f32"
    assert a.get(a.CRITIC_AGGREGATION) == 1 and b.get(b.CRITIC_AGGREGATION) == 0
    b.set(b.GAE_VARIANT, 13)
    assert a.get(a.GAE_VARIANT) == 0 and b.get(b.GAE_VARIANT) == 13 and a.h2_launches == 0
    lib = _lib.lib()
    assert lib.mava_ctx_set(a.handle, 99, 0) <= -1000 and b"unknown key" in lib.mava_last_error()
    assert lib.mava_ctx_set(a.handle, a.MATMUL_MODE, 7) <= -1000
    assert lib.mava_ctx_set(None, 0, 0) <= -1000 and lib.mava_ctx_destroy(None) == 0
    a.close()
    b.close()
    assert a.handle is None
    for name in dir(lib):  # no process-wide setters are left in the ABI
        assert "set_variant" not in name and "set_matmul" not in name
    for gone in ("mava_ppo_set_matmul_mode", "mava_gae_set_variant", "mava_policy_set_variant", "mava_ppo_set_critic_aggregation"):
        assert not hasattr(lib, gone), gone
