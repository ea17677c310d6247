"""MobileNetV3 (Howard et al. 2019, "Searching for MobileNetV3"), small and large.

Defined directly, like ``models/mobilenet.py``, with torchvision's module tree and state-dict keys:
``features.0`` is the stem unit ``(conv3x3 s2, BN, Hardswish)``, then :class:`InvertedResidualV3`
blocks whose ``.block`` is a plain ``nn.Sequential`` of ``[expand unit,] depthwise unit,
[SqueezeExcitation,] project unit`` (every unit a plain ``nn.Sequential(conv, BN[, activation])``),
a last 1x1 unit to 6 x its input, global average pooling and
``classifier = Sequential(Linear, Hardswish, Dropout, Linear)``.

What sets the family apart from MobileNetV2 is the squeeze-and-excitation gate between the
depthwise conv and the project conv: out = x * hardsigmoid(fc2(relu(fc1(mean_hw(x))))). For
pruning it is a per-channel pass-through (``utils.graph.is_channel_gate``): hidden channel c of a
block is one filter of the expand conv, one entry of each BN, one k x k filter of the depthwise
conv, one input column of ``fc1``, one output row of ``fc2`` and one input column of the project
conv (``utils.graph.get_mobilenet_pruning_graph``).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .mobilenet import _make_divisible
from .partial import PartialForwardMixin

# (kernel, expanded channels, output channels, SE, Hardswish, stride) per block (the paper's tables 1, 2)
SMALL = [(3, 16, 16, 1, 0, 2), (3, 72, 24, 0, 0, 2), (3, 88, 24, 0, 0, 1), (5, 96, 40, 1, 1, 2), (5, 240, 40, 1, 1, 1),
         (5, 240, 40, 1, 1, 1), (5, 120, 48, 1, 1, 1), (5, 144, 48, 1, 1, 1), (5, 288, 96, 1, 1, 2),
         (5, 576, 96, 1, 1, 1), (5, 576, 96, 1, 1, 1)]
LARGE = [(3, 16, 16, 0, 0, 1), (3, 64, 24, 0, 0, 2), (3, 72, 24, 0, 0, 1), (5, 72, 40, 1, 0, 2), (5, 120, 40, 1, 0, 1),
         (5, 120, 40, 1, 0, 1), (3, 240, 80, 0, 1, 2), (3, 200, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1),
         (3, 184, 80, 0, 1, 1), (3, 480, 112, 1, 1, 1), (3, 672, 112, 1, 1, 1), (5, 672, 160, 1, 1, 2),
         (5, 960, 160, 1, 1, 1), (5, 960, 160, 1, 1, 1)]


def _bn(c: int) -> nn.BatchNorm2d:
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)


def conv_bn_act(cin: int, cout: int, kernel_size: int = 3, stride: int = 1, groups: int = 1, act=None) -> nn.Sequential:
    layers = [nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False), _bn(cout)]
    if act is not None:
        layers.append(act(inplace=True))
    return nn.Sequential(*layers)


class SqueezeExcitation(nn.Module):
    """out = x * scale_activation(fc2(activation(fc1(avgpool(x)))))."""

    def __init__(self, channels: int, squeeze: int):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Hardsigmoid()

    def forward(self, x):
        s = self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))
        return s * x


class InvertedResidualV3(nn.Module):
    def __init__(self, inp: int, kernel: int, expanded: int, oup: int, use_se: bool, use_hs: bool, stride: int):
        super().__init__()
        assert stride in (1, 2)
        self.use_res_connect = stride == 1 and inp == oup
        act = nn.Hardswish if use_hs else nn.ReLU
        layers = []
        if expanded != inp:
            layers.append(conv_bn_act(inp, expanded, kernel_size=1, act=act))
        layers.append(conv_bn_act(expanded, expanded, kernel_size=kernel, stride=stride, groups=expanded, act=act))
        if use_se:
            layers.append(SqueezeExcitation(expanded, _make_divisible(expanded // 4, 8)))
        layers.append(conv_bn_act(expanded, oup, kernel_size=1))  # linear bottleneck
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.block(x) if self.use_res_connect else self.block(x)


class MobileNetV3(nn.Module, PartialForwardMixin):
    """``small_input``: stride 1 in the stem and in the first two strided blocks (32-px inputs end
    at an 8 x 8 map instead of 1 x 1)."""

    def __init__(self, table, last_channel: int, num_classes: int = 1000, width_mult: float = 1.0,
                 small_input: bool = False, dropout: float = 0.2):
        super().__init__()
        cin = _make_divisible(16 * width_mult)
        features = [conv_bn_act(3, cin, stride=1 if small_input else 2, act=nn.Hardswish)]
        strided = 0
        for k, exp, c, se, hs, s in table:
            if s == 2:
                strided += 1
                if small_input and strided <= 2:
                    s = 1
            cout = _make_divisible(c * width_mult)
            features.append(InvertedResidualV3(cin, k, _make_divisible(exp * width_mult), cout, bool(se), bool(hs), s))
            cin = cout
        features.append(conv_bn_act(cin, 6 * cin, kernel_size=1, act=nn.Hardswish))
        self.features = nn.Sequential(*features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(6 * cin, last_channel), nn.Hardswish(inplace=True),
                                        nn.Dropout(p=dropout, inplace=True), nn.Linear(last_channel, num_classes))
        self._initialize_weights()

    def _pool(self, x):
        return torch.flatten(self.avgpool(x), 1)

    def _stages(self):
        return list(self.features.children()) + [self._pool] + list(self.classifier.children())

    def is_partial_stage(self, module) -> bool:
        """Only the top-level units of ``features`` and the classifier layers are stages (the rule
        of :class:`~torchpruner_amd.models.mobilenet.MobileNetV2`): a block's shortcut runs around
        everything nested in it."""
        return any(module is s for s in self._stages())

    def forward_partial(self, x, to_module=None, from_module=None):
        for m in (to_module, from_module):
            if m is not None and not self.is_partial_stage(m):
                raise ValueError("forward_partial of MobileNetV3 starts and stops at the top-level units of "
                                 "`features` and the classifier layers only; a module nested in a block is no stage")
        return super().forward_partial(x, to_module=to_module, from_module=from_module)

    def forward(self, x, to_module=None, from_module=None):
        return self.forward_partial(x, to_module=to_module, from_module=from_module)

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)


def mobilenet_v3_small(num_classes: int = 1000, width_mult: float = 1.0, small_input: bool = False) -> MobileNetV3:
    return MobileNetV3(SMALL, 1024, num_classes, width_mult=width_mult, small_input=small_input)


def mobilenet_v3_large(num_classes: int = 1000, width_mult: float = 1.0, small_input: bool = False) -> MobileNetV3:
    return MobileNetV3(LARGE, 1280, num_classes, width_mult=width_mult, small_input=small_input)
