"""MobileNetV2 (Sandler et al. 2018, "MobileNetV2: Inverted Residuals and Linear Bottlenecks").

The project does not depend on torchvision, so the network is defined directly (like
``models/vgg.py``) with torchvision's module tree: ``features`` is a Sequential of conv-BN-ReLU6 units and
:class:`InvertedResidual` blocks whose ``.conv`` Sequential holds
``[expand 1x1 unit,] depthwise 3x3 unit, project 1x1 conv, BN``; then global average pooling and
``classifier = Sequential(Dropout, Linear)``. The state_dict keys (``features.0.0.weight``,
``features.2.conv.1.0.weight``, ..., ``classifier.1.bias``) match torchvision's ``mobilenet_v2``.

The hidden (expanded) channels of a block are private to it: pruning hidden channel c removes one
filter of the expand conv, one entry of each BN, one k x k filter of the depthwise conv and one
input column of the project conv (``utils.graph.get_mobilenet_pruning_graph``).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .partial import PartialForwardMixin

# (expansion t, output channels c, repeats n, stride s) per stage
SETTINGS = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:  # never round down by more than 10 %
        new_v += divisor
    return new_v


def conv_bn_relu6(cin: int, cout: int, kernel_size: int = 3, stride: int = 1, groups: int = 1) -> nn.Sequential:
    return nn.Sequential(
        nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False),
        nn.BatchNorm2d(cout),
        nn.ReLU6(inplace=True),
    )


class InvertedResidual(nn.Module):
    def __init__(self, inp: int, oup: int, stride: int, expand_ratio: int):
        super().__init__()
        assert stride in (1, 2)
        hidden = int(round(inp * expand_ratio))
        self.stride = stride
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(conv_bn_relu6(inp, hidden, kernel_size=1))
        layers += [
            conv_bn_relu6(hidden, hidden, stride=stride, groups=hidden),  # depthwise
            nn.Conv2d(hidden, oup, 1, 1, 0, bias=False),                  # linear bottleneck
            nn.BatchNorm2d(oup),
        ]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


class MobileNetV2(nn.Module, PartialForwardMixin):
    """``small_input``: stride 1 in the stem and in the first two strided stages (32-px inputs end
    at an 8 x 8 map instead of 1 x 1)."""

    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0, small_input: bool = False,
                 dropout: float = 0.2):
        super().__init__()
        cin = _make_divisible(32 * width_mult)
        self.last_channel = _make_divisible(1280 * max(1.0, width_mult))
        features = [conv_bn_relu6(3, cin, stride=1 if small_input else 2)]
        strided = 0
        for t, c, n, s in SETTINGS:
            cout = _make_divisible(c * width_mult)
            if s == 2:
                strided += 1
                if small_input and strided <= 2:
                    s = 1
            for i in range(n):
                features.append(InvertedResidual(cin, cout, s if i == 0 else 1, t))
                cin = cout
        features.append(conv_bn_relu6(cin, self.last_channel, kernel_size=1))
        self.features = nn.Sequential(*features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout), nn.Linear(self.last_channel, num_classes))
        self._initialize_weights()

    def _pool(self, x):
        return torch.flatten(self.avgpool(x), 1)

    def _stages(self):
        return list(self.features.children()) + [self._pool] + list(self.classifier.children())

    def is_partial_stage(self, module) -> bool:
        """Whether ``forward_partial`` can stop after / start after ``module``: only the top-level
        units of ``features`` and the classifier layers are stages. A module inside an
        :class:`InvertedResidual` (every entry of the pruning graph and its evaluation module) is
        not: the block's shortcut runs around it, so a chain cannot be cut there. Shapley takes
        its masking-hook path for such modules."""
        return any(module is s for s in self._stages())

    def forward_partial(self, x, to_module=None, from_module=None):
        for m in (to_module, from_module):
            if m is not None and not self.is_partial_stage(m):
                raise ValueError("forward_partial of MobileNetV2 starts and stops at the top-level units of "
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


def mobilenet_v2(num_classes: int = 1000, width_mult: float = 1.0, small_input: bool = False) -> MobileNetV2:
    return MobileNetV2(num_classes, width_mult=width_mult, small_input=small_input)
