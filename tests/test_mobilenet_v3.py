"""MobileNetV3 small / large: parameter counts, torchvision's state-dict keys, forward shapes and
the forward_partial stage rule."""
import pytest
import torch
import torch.nn as nn

from torchpruner_amd.models import mobilenet_v3_large, mobilenet_v3_small
from torchpruner_amd.models.mobilenet_v3 import SqueezeExcitation
from torchpruner_amd.utils import is_channel_gate


@pytest.mark.parametrize("factory, count", [(mobilenet_v3_small, 2_542_856), (mobilenet_v3_large, 5_483_032)])
def test_parameter_counts(factory, count):
    assert sum(p.numel() for p in factory().parameters()) == count


def test_state_dict_keys_and_module_tree():
    small, large = mobilenet_v3_small(), mobilenet_v3_large()
    sd_s, sd_l = small.state_dict(), large.state_dict()
    assert tuple(sd_s["features.1.block.1.fc1.weight"].shape) == (8, 16, 1, 1)
    assert tuple(sd_l["features.4.block.2.fc2.bias"].shape) == (72,)
    assert tuple(sd_s["classifier.3.weight"].shape) == (1000, 1024)
    assert tuple(sd_l["classifier.3.weight"].shape) == (1000, 1280)
    assert tuple(sd_s["features.0.0.weight"].shape) == (16, 3, 3, 3)
    assert tuple(sd_s["features.12.0.weight"].shape) == (576, 96, 1, 1)
    assert tuple(sd_l["features.16.0.weight"].shape) == (960, 160, 1, 1)
    se = small.features[1].block[1]
    assert isinstance(se, SqueezeExcitation) and is_channel_gate(se)
    assert [n for n, _ in se.named_children()] == ["avgpool", "fc1", "fc2", "activation", "scale_activation"]
    assert isinstance(se.activation, nn.ReLU) and isinstance(se.scale_activation, nn.Hardsigmoid)
    assert large.features[4].block[2].fc1.out_channels == 24 and small.features[4].block[2].fc1.out_channels == 24
    for m in small.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert m.eps == 1e-3 and m.momentum == 0.01
    assert type(small.features[2].block) is nn.Sequential and isinstance(small.features[2].use_res_connect, bool)
    assert isinstance(small.features[2].block[0][2], nn.ReLU) and isinstance(small.features[4].block[0][2], nn.Hardswish)
    assert isinstance(small.classifier[1], nn.Hardswish) and small.classifier[2].p == 0.2


@pytest.mark.parametrize("factory", [mobilenet_v3_small, mobilenet_v3_large])
def test_forward_shapes_small_input(factory):
    torch.manual_seed(0)
    model = factory(10, small_input=True).eval()
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        assert model.features(x).shape[2:] == (8, 8)
        assert model(x).shape == (2, 10)
    half = factory(10, width_mult=0.5, small_input=True).eval()
    with torch.no_grad():
        assert half(x).shape == (2, 10)


def test_forward_partial_stage_rule():
    torch.manual_seed(0)
    model = mobilenet_v3_small(10, small_input=True).eval()
    x = torch.randn(2, 3, 32, 32)
    stage = model.features[4]
    with torch.no_grad():
        mid = model.forward_partial(x, to_module=stage)
        torch.testing.assert_close(model.forward_partial(mid, from_module=stage), model(x))
    assert model.is_partial_stage(stage) and model.is_partial_stage(model.classifier[0])
    nested = stage.block[2]
    assert not model.is_partial_stage(nested)
    with pytest.raises(ValueError, match="stage"):
        model.forward_partial(x, to_module=nested)
