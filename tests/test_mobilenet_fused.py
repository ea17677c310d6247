"""Structural recognition of inverted-residual blocks (engine/train.py::_ir_kind): the blocks of
models/mobilenet.py (torchvision's layout) are recognised with and without an expand unit, anything
else keeps its current path."""
import torch.nn as nn

from torchpruner_amd.engine.train import _ir_kind
from torchpruner_amd.models import mobilenet_v2
from torchpruner_amd.models.mobilenet import InvertedResidual, conv_bn_relu6


def test_ir_kind_recognises_every_mobilenet_block():
    model = mobilenet_v2(10, width_mult=0.5, small_input=True)
    blocks = [m for m in model.modules() if isinstance(m, InvertedResidual)]
    kinds = [_ir_kind(b) for b in blocks]
    assert len(blocks) == 17 and kinds == ["dw"] + ["expand"] * 16
    assert any(b.use_res_connect for b in blocks) and not all(b.use_res_connect for b in blocks)
    # nothing else in the model is one: the units, the Sequentials, the model itself
    assert [m for m in model.modules() if _ir_kind(m) is not None] == blocks
    # ReLU units are taken like ReLU6 ones
    b = InvertedResidual(16, 16, 1, 6)
    b.conv[0][2], b.conv[1][2] = nn.ReLU(inplace=True), nn.ReLU()
    assert _ir_kind(b) == "expand"


def test_ir_kind_rejects_other_layouts():
    from torchpruner_amd.models.resnet import BasicBlock, Bottleneck
    b = InvertedResidual(16, 16, 1, 6)
    assert _ir_kind(b) == "expand"
    b.conv = nn.Sequential(*b.conv, nn.Identity())  # an extra module
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 16, 1, 6)
    b.conv = nn.Sequential(nn.Identity(), *b.conv)
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 2, 6)
    b.conv[1] = conv_bn_relu6(96, 96, stride=2, groups=2)  # grouped, not depthwise
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[2] = nn.Conv2d(96, 24, 3, 1, 1, bias=False)  # project conv not 1x1
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[2] = nn.Conv2d(96, 24, 1, 2, 0, bias=False)  # strided project conv
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[2] = nn.Conv2d(96, 24, 1, 1, 0, groups=2, bias=False)  # grouped project conv
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[0][2] = nn.Hardswish()  # another activation
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[1] = nn.Sequential(*b.conv[1], nn.Identity())  # a unit with an extra module
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.conv[3] = nn.GroupNorm(4, 24)  # no BatchNorm tail
    assert _ir_kind(b) is None
    b = InvertedResidual(16, 24, 1, 6)
    b.use_res_connect = None  # no bool
    assert _ir_kind(b) is None

    class Sub(nn.Sequential):  # not a plain nn.Sequential: it may have its own forward
        pass

    b = InvertedResidual(16, 24, 1, 6)
    b.conv = Sub(*b.conv)
    assert _ir_kind(b) is None
    for block in (BasicBlock, Bottleneck):
        assert _ir_kind(block(16, 16)) is None
