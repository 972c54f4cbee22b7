"""CPU: qmix_fused_mode, the predicate that sends rec_qmix's train step to the fused mixer kernel (csrc/qmix_fused.hip)."""
import pytest

from mava_amd.qmix_learner import qmix_fused_mode

ON = {"MAVA_QMIX_FUSED": "1"}


# (env, matmul mode, mixer, A, Em, Hh, actions) -> fused
@pytest.mark.parametrize("env,mode,mixer,A,Em,Hh,nA,want", [
    (ON, "f16x2", "qmix", 3, 32, 64, 6, True),     # the defaults
    ({}, "f16x2", "qmix", 3, 32, 64, 6, False),    # opt-in
    ({"MAVA_QMIX_FUSED": "0"}, "f16x2", "qmix", 3, 32, 64, 6, False),
    (ON, "f32", "qmix", 3, 32, 64, 6, False),      # f16x2 products only
    (ON, "f16x2", "vdn", 3, 32, 64, 6, False),     # no mixer
    (ON, "f16x2", "qmix", 16, 32, 64, 6, True),    # A * Em = 512
    (ON, "f16x2", "qmix", 9, 57, 64, 6, False),    # A * Em = 513
    (ON, "f16x2", "qmix", 3, 32, 128, 6, True),
    (ON, "f16x2", "qmix", 3, 32, 129, 6, False),
    (ON, "f16x2", "qmix", 3, 64, 64, 6, True),
    (ON, "f16x2", "qmix", 3, 65, 64, 6, False),
    (ON, "f16x2", "qmix", 16, 1, 1, 1, True),
    (ON, "f16x2", "qmix", 17, 1, 1, 1, False),
    (ON, "f16x2", "qmix", 3, 32, 64, 32, True),
    (ON, "f16x2", "qmix", 3, 32, 64, 33, False),
    (ON, "f16x2", "qmix", 3, 0, 64, 6, False),
    (ON, "f16x2", "qmix", 3, 32, 0, 6, False),
])
def test_qmix_fused_mode(env, mode, mixer, A, Em, Hh, nA, want):
    assert qmix_fused_mode(mode, mixer, A, Em, Hh, nA, env=env) is want


def test_qmix_fused_mode_reads_the_process_environment_by_default(monkeypatch):
    monkeypatch.delenv("MAVA_QMIX_FUSED", raising=False)
    assert not qmix_fused_mode("f16x2", "qmix", 3, 32, 64, 6)
    monkeypatch.setenv("MAVA_QMIX_FUSED", "1")
    assert qmix_fused_mode("f16x2", "qmix", 3, 32, 64, 6)
