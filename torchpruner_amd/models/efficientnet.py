"""EfficientNet (Tan & Le 2019, "EfficientNet: Rethinking Model Scaling for Convolutional Neural
Networks"), the B0 baseline and its width / depth scalings.

Defined directly, like ``models/mobilenet_v3.py``, with torchvision's module tree and state-dict
keys: ``features.0`` is the stem unit ``(conv3x3 s2, BN, SiLU)``, ``features.1`` .. ``features.7`` are
the seven stages, each a plain ``nn.Sequential`` of :class:`MBConv` blocks (``features.N.M.block.K...``),
``features.8`` the last 1x1 unit to 4 x its input, then global average pooling and
``classifier = Sequential(Dropout, Linear)``. A block's ``.block`` is a plain ``nn.Sequential`` of
``[expand unit,] depthwise unit, SqueezeExcitation(SiLU, Sigmoid), project unit`` (the MobileNetV3
block with SiLU for the unit activation and inside the gate), so ``get_mobilenet_pruning_graph``
and the pruner take it as they take a V3 block; its ``stochastic_depth`` member drops the residual
branch of whole samples ("row" mode) in training.

EfficientNetV2 (Tan & Le 2021, "EfficientNetV2: Smaller Models and Faster Training") is the same tree
over the ``V2_S`` table: its first three stages are :class:`FusedMBConv` blocks (``.block`` is
``[dense kxk unit, project unit]``, or the single ``kxk`` unit at expand ratio 1; no depthwise conv,
no gate) and the last unit has 1280 channels.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .mobilenet import _make_divisible
from .mobilenet_v3 import SqueezeExcitation
from .partial import PartialForwardMixin

# (expand ratio, kernel, stride, input channels, output channels, layers) per stage (the paper's table 1)
B0 = [(1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
      (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1)]
# the same columns + "fused" for EfficientNetV2-S (the 2021 paper's table 4)
V2_S = [(1, 3, 1, 24, 24, 2, True), (4, 3, 2, 24, 48, 4, True), (4, 3, 2, 48, 64, 4, True), (4, 3, 2, 64, 128, 6),
        (6, 3, 1, 128, 160, 9), (6, 3, 2, 160, 256, 15)]


def conv_bn_silu(cin: int, cout: int, kernel_size: int = 3, stride: int = 1, groups: int = 1, act: bool = True):
    layers = [nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False),
              nn.BatchNorm2d(cout)]
    if act:
        layers.append(nn.SiLU(inplace=True))
    return nn.Sequential(*layers)


class StochasticDepth(nn.Module):
    """Row mode: in training a sample's branch is zeroed with probability ``p`` and the survivors are
    scaled by 1 / (1 - p); the identity in eval mode and for p = 0."""

    def __init__(self, p: float):
        super().__init__()
        self.p, self.mode = float(p), "row"

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        keep = 1.0 - self.p
        noise = torch.empty((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device).bernoulli_(keep)
        if keep > 0.0:
            noise.div_(keep)
        return x * noise


class MBConv(nn.Module):
    def __init__(self, inp: int, expand_ratio: int, kernel: int, stride: int, oup: int, sd_prob: float):
        super().__init__()
        assert stride in (1, 2)
        self.use_res_connect = stride == 1 and inp == oup
        expanded = _make_divisible(inp * expand_ratio)
        layers = []
        if expanded != inp:
            layers.append(conv_bn_silu(inp, expanded, kernel_size=1))
        layers.append(conv_bn_silu(expanded, expanded, kernel_size=kernel, stride=stride, groups=expanded))
        gate = SqueezeExcitation(expanded, max(1, inp // 4))
        gate.activation, gate.scale_activation = nn.SiLU(inplace=True), nn.Sigmoid()
        layers.append(gate)
        layers.append(conv_bn_silu(expanded, oup, kernel_size=1, act=False))  # linear bottleneck
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob)

    def forward(self, x):
        out = self.block(x)
        return x + self.stochastic_depth(out) if self.use_res_connect else out


class FusedMBConv(nn.Module):
    def __init__(self, inp: int, expand_ratio: int, kernel: int, stride: int, oup: int, sd_prob: float):
        super().__init__()
        assert stride in (1, 2)
        self.use_res_connect = stride == 1 and inp == oup
        expanded = _make_divisible(inp * expand_ratio)
        if expanded != inp:
            layers = [conv_bn_silu(inp, expanded, kernel_size=kernel, stride=stride),
                      conv_bn_silu(expanded, oup, kernel_size=1, act=False)]
        else:
            layers = [conv_bn_silu(inp, oup, kernel_size=kernel, stride=stride)]
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob)

    def forward(self, x):
        out = self.block(x)
        return x + self.stochastic_depth(out) if self.use_res_connect else out


class EfficientNet(nn.Module, PartialForwardMixin):
    """``small_input``: stride 1 in the stem and in the first two strided stages (32-px inputs end
    at an 8 x 8 map instead of 1 x 1)."""

    def __init__(self, width_mult: float = 1.0, depth_mult: float = 1.0, num_classes: int = 1000,
                 small_input: bool = False, dropout: float = 0.2, stochastic_depth_prob: float = 0.2,
                 table=B0, last_channels: int | None = None):
        super().__init__()
        width = lambda c: _make_divisible(c * width_mult)
        depths = [int(math.ceil(row[5] * depth_mult)) for row in table]
        features = [conv_bn_silu(3, width(table[0][3]), stride=1 if small_input else 2)]
        total, done, strided = sum(depths), 0, 0
        for (ratio, k, s, cin, cout, _, *fused), n in zip(table, depths):
            block = FusedMBConv if fused else MBConv
            if s == 2:
                strided += 1
                if small_input and strided <= 2:
                    s = 1
            stage = []
            for i in range(n):
                stage.append(block(width(cout) if i else width(cin), ratio, k, 1 if i else s, width(cout),
                                   stochastic_depth_prob * done / total))
                done += 1
            features.append(nn.Sequential(*stage))
        last = width(table[-1][4])
        head = width(last_channels) if last_channels else 4 * last
        features.append(conv_bn_silu(last, head, kernel_size=1))
        self.features = nn.Sequential(*features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        # (Dropout out of place, where torchvision's is in place: its input is the flattened output of the
        # pool, a view that autograd does not let the native pool's consumer overwrite)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout), nn.Linear(head, num_classes))
        self._initialize_weights()

    def _pool(self, x):
        return torch.flatten(self.avgpool(x), 1)

    def _stages(self):
        return list(self.features.children()) + [self._pool] + list(self.classifier.children())

    def is_partial_stage(self, module) -> bool:
        """Only the top-level units of ``features`` (the stem, the seven stages, the last unit) and
        the classifier layers are stages, the rule of :class:`~torchpruner_amd.models.mobilenet_v3.MobileNetV3`."""
        return any(module is s for s in self._stages())

    def forward_partial(self, x, to_module=None, from_module=None):
        for m in (to_module, from_module):
            if m is not None and not self.is_partial_stage(m):
                raise ValueError("forward_partial of EfficientNet starts and stops at the top-level units of "
                                 "`features` and the classifier layers only; a module nested in a stage is no stage")
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
                bound = 1.0 / math.sqrt(m.out_features)
                nn.init.uniform_(m.weight, -bound, bound)
                nn.init.zeros_(m.bias)


def efficientnet(width_mult: float = 1.0, depth_mult: float = 1.0, num_classes: int = 1000,
                 small_input: bool = False) -> EfficientNet:
    return EfficientNet(width_mult, depth_mult, num_classes, small_input)


def efficientnet_b0(num_classes: int = 1000, small_input: bool = False) -> EfficientNet:
    return efficientnet(1.0, 1.0, num_classes, small_input)


def efficientnet_v2(width_mult: float = 1.0, depth_mult: float = 1.0, num_classes: int = 1000,
                    small_input: bool = False) -> EfficientNet:
    """EfficientNetV2-S scaled in width and depth (torchvision's ``efficientnet_v2_s`` tree and keys at 1.0)."""
    return EfficientNet(width_mult, depth_mult, num_classes, small_input, table=V2_S, last_channels=1280)


def efficientnet_v2_s(num_classes: int = 1000, small_input: bool = False) -> EfficientNet:
    return efficientnet_v2(1.0, 1.0, num_classes, small_input)
