"""CPU: the C ABI of ff_mat's fused acting step (csrc/mat_act.hip) - its symbols, the parameter layout the kernel derives
against MATNet's, the argument checks that come before any launch, and the network.acting config key."""
import ctypes as C

import pytest

from mava_amd import _lib
from mava_amd.config import compose
from mava_amd.mat_learner import MATNet

# (B, A, O, nA, D, H, n_block): the shapes tests/test_gpu_mat_fused_act.py runs
SHAPES = [(1, 1, 3, 1, 32, 1, 1), (11, 3, 7, 5, 32, 1, 1), (43, 3, 7, 5, 64, 2, 2), (11, 4, 70, 5, 64, 1, 1), (43, 5, 33, 33, 96, 4, 1),
          (7, 7, 12, 6, 64, 2, 1), (3, 20, 9, 64, 128, 4, 2), (2, 32, 5, 3, 128, 1, 1), (5, 16, 1024, 7, 128, 4, 1)]


def test_symbols_and_abi_version():
    lib = _lib.lib()
    for name in ("mava_transformer_param_count", "mava_transformer_act_workspace_bytes", "mava_transformer_act_f32"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES
    assert lib.mava_abi_version() == 4


@pytest.mark.parametrize("shape", SHAPES)
def test_param_count_is_the_learners_layout(shape):
    B, A, O, nA, D, H, nb = shape
    assert _lib.lib().mava_transformer_param_count(O, nA, D, nb) == MATNet(O, nA, A, D, H, nb).num_params


def test_workspace_bytes():
    lib = _lib.lib()
    one = lib.mava_transformer_act_workspace_bytes(11, 4, 64, 1, 1)
    assert one >= 4 * 4 * 4 * 64 * 4  # at least the self- and cross-attention keys and values of one sample's agents
    assert lib.mava_transformer_act_workspace_bytes(11, 4, 64, 2, 3) == 6 * one  # per block of the grid and per decoder block


GOOD = dict(B=2, A=4, O=7, nA=5, D=64, H=2, nb=1, n_blocks=1)


def _call(lib, fake, ws_bytes=None, null=(), **over):
    a = dict(GOOD, **over)
    need = lib.mava_transformer_act_workspace_bytes(a["B"], a["A"], a["D"], a["nb"], max(a["n_blocks"], 1))
    p = {k: (None if k in null else fake) for k in ("params", "agents_view", "action", "log_prob")}
    return lib.mava_transformer_act_f32(p["params"], p["agents_view"], None, a["B"], a["A"], a["O"], a["nA"], a["D"], a["H"], a["nb"], 1, 2, 3,
                                        0, p["action"], p["log_prob"], None, fake, need if ws_bytes is None else ws_bytes, a["n_blocks"], None)


@pytest.mark.parametrize("bad,word", [(dict(A=0), b"A=0"), (dict(A=33), b"A=33"), (dict(D=48), b"D=48"), (dict(D=160), b"D=160"),
                                      (dict(D=64, H=3), b"n_head=3"), (dict(nA=65), b"n_actions=65"), (dict(O=0), b"O=0"),
                                      (dict(O=1025), b"O=1025"), (dict(B=0), b"B=0"), (dict(n_blocks=0), b"n_blocks=0"),
                                      (dict(nb=0), b"n_block=0")])
def test_bad_shapes_are_refused_before_any_launch(bad, word):
    """No GPU here: a call that got as far as a launch would fail with a HIP error (a small negative code), not <= -1000."""
    lib = _lib.lib()
    buf = (C.c_uint8 * 64)()
    fake = C.cast(buf, C.c_void_p)  # never dereferenced: the checks come first
    rc = _call(lib, fake, **bad)
    assert rc <= -1000, rc
    assert word in lib.mava_last_error(), lib.mava_last_error()


@pytest.mark.parametrize("null", ["params", "agents_view", "action", "log_prob"])
def test_null_pointers_are_refused(null):
    lib = _lib.lib()
    fake = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    rc = _call(lib, fake, null=(null,))
    assert rc <= -1000 and b"null pointer" in lib.mava_last_error()


def test_short_or_missing_workspace_is_refused():
    lib = _lib.lib()
    fake = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    need = lib.mava_transformer_act_workspace_bytes(GOOD["B"], GOOD["A"], GOOD["D"], GOOD["nb"], GOOD["n_blocks"])
    rc = _call(lib, fake, ws_bytes=need - 1)
    assert rc <= -1000 and b"workspace" in lib.mava_last_error()
    a = GOOD
    rc = lib.mava_transformer_act_f32(fake, fake, None, a["B"], a["A"], a["O"], a["nA"], a["D"], a["H"], a["nb"], 1, 2, 3, 0, fake, fake, None,
                                      None, need, 1, None)
    assert rc <= -1000 and b"workspace" in lib.mava_last_error()


def test_depth_beyond_the_cap_is_not_instantiated():
    """Return code 1 (launch(..., ok=(0, 1))): nothing launched, the caller runs layer by layer.  The cap is at least 4."""
    lib = _lib.lib()
    fake = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    assert _call(lib, fake, nb=64) == 1
    assert lib.mava_transformer_act_workspace_bytes(2, 4, 64, 4, 1) > 0  # four blocks are taken


def test_config_key():
    assert compose("default_ff_mat").network.acting == "layerwise"
    assert compose("default_ff_mat", ["network.acting=fused"]).network.acting == "fused"
