"""Host side of the fused soft actor-critic train step: the envelope decision and the tile geometry (no GPU)."""
import pytest

from mava_amd.sac_learner import sac_fused_mode, sac_tiles

MLP = {"_target_": "mava.networks.MLPTorso", "layer_sizes": [128, 128], "activation": "relu", "use_layer_norm": False}
ON, OFF = {"MAVA_SAC_FUSED": "1"}, {"MAVA_SAC_FUSED": "0"}


@pytest.mark.parametrize("want,mode,actor,critic,D,O,Kq,A,env", [
    (True, "f16x2", MLP, MLP, 2, 18, 20, 3, ON),
    (True, "f16x2", MLP, MLP, 16, 127, 127, 16, ON),          # every width at its edge
    (False, "f16x2", MLP, MLP, 2, 18, 20, 3, OFF),
    (False, "f16x2", MLP, MLP, 2, 18, 20, 3, {}),             # off by default
    (False, "f32", MLP, MLP, 2, 18, 20, 3, ON),
    (False, "f16x2", dict(MLP, layer_sizes=[64, 64]), MLP, 2, 18, 20, 3, ON),
    (False, "f16x2", MLP, dict(MLP, layer_sizes=[64, 64]), 2, 18, 20, 3, ON),
    (False, "f16x2", MLP, dict(MLP, activation="tanh"), 2, 18, 20, 3, ON),
    (False, "f16x2", dict(MLP, use_layer_norm=True), MLP, 2, 18, 20, 3, ON),
    (False, "f16x2", MLP, MLP, 17, 18, 35, 3, ON),
    (False, "f16x2", MLP, MLP, 2, 128, 20, 3, ON),
    (False, "f16x2", MLP, MLP, 2, 18, 128, 3, ON),
    (False, "f16x2", MLP, MLP, 2, 18, 20, 17, ON),
])
def test_envelope(want, mode, actor, critic, D, O, Kq, A, env):
    assert sac_fused_mode(mode, actor, critic, D, O, Kq, A, env=env) is want


@pytest.mark.parametrize("A,B,want", [(2, 16, (16, 1, 32)), (3, 12, (10, 2, 6)), (5, 7, (6, 2, 5)), (8, 9, (4, 3, 8)),
                                      (16, 3, (2, 2, 16)), (3, 32, (10, 4, 6))])
def test_tile_geometry(A, B, want):
    assert sac_tiles(B, A) == want
