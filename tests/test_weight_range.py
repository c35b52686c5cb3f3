"""Load-time refusal of weights that fp16 operand planes cannot hold (weights.check_f16_weight; -m "not gpu").  The activations' range
guard (ser_hip.h range_flag) never sees the weights: a weight beyond +-65504, or a NaN / Inf, would saturate silently in every fp16-plane
mode, so the encoders refuse it at load and point to --mode fp32x."""
import pytest
import torch

from interspeech_ser_amd.weights import F16_MAX, check_f16_weight


def test_accepts_the_full_fp16_range():
    w = torch.randn(16, 64)
    w[3, 5] = F16_MAX
    w[7, 1] = -F16_MAX
    check_f16_weight(w, "layer.weight")
    check_f16_weight(torch.zeros(0, 64), "empty.weight")


@pytest.mark.parametrize("value", [F16_MAX * 1.0001, -7.0e4, 1.0e30])
def test_refuses_a_weight_beyond_the_fp16_range(value):
    w = torch.randn(16, 64)
    w[15, 63] = value
    with pytest.raises(ValueError) as e:
        check_f16_weight(w, "encoder.layers.3.fc2.weight")
    assert "encoder.layers.3.fc2.weight" in str(e.value) and "--mode fp32x" in str(e.value)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_refuses_a_non_finite_weight(value):
    w = torch.randn(8, 64)
    w[0, 0] = value
    with pytest.raises(ValueError) as e:
        check_f16_weight(w, "feature_projection.projection.weight")
    assert "feature_projection.projection.weight" in str(e.value) and "--mode fp32x" in str(e.value)


def test_checks_the_gamma_folded_weight():
    """_linear_ln splits W * gamma: a fold that leaves the range is refused though W and gamma each fit"""
    w = torch.full((4, 64), 300.0)
    gamma = torch.full((64,), 300.0)
    check_f16_weight(w, "w")
    check_f16_weight(gamma[None], "gamma")
    with pytest.raises(ValueError, match="folded"):
        check_f16_weight((w.double() * gamma.double()[None]).float(), "fc1.weight (folded with its LayerNorm weight)")
