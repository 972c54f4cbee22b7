"""No GPU: mava_rec_out_continuous_f32 on both sides of the C ABI; RecLearner's gate (fused_out_modes) is off by default, on for one combination."""
import itertools
import os
import re

from mava_amd import _lib
from mava_amd.rec_learner import fused_out_modes


def test_symbol_declared_on_both_sides():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mava_hip.h")).read()
    m = re.search(r"int mava_rec_out_continuous_f32\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == len(_lib._SIGNATURES["mava_rec_out_continuous_f32"]) == 26


def test_gate():
    for switch, mode, cont, ind, n, generic in itertools.product((None, "0", "1"), ("f32", "f16x2"), (False, True), (False, True), (2, 16, 17), (False, True)):
        env = {} if switch is None else {"MAVA_REC_FUSED_OUT_CONTINUOUS": switch}
        fused, fused_cont = fused_out_modes(mode, cont, ind, n, generic, env)
        assert fused_cont == (switch == "1" and mode == "f16x2" and cont and ind and n <= 16 and not generic)
        assert fused == (mode == "f16x2" and not cont and n <= 16 and not generic)  # the discrete gate does not move
