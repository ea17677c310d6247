"""Pruning-graph utilities.

* :func:`find_best_module_for_attributions` — parity with the reference
  (torchpruner/utils/graph.py:9-34): walk ``model.modules()`` after ``module`` and move the
  evaluation point past any directly following BatchNorm / activation modules.
* :func:`get_vgg_pruning_graph` — parity with graph.py:37-61 for chain CNNs.
* :func:`get_resnet_pruning_graph` — new: residual-aware graph for bottleneck/basic-block
  ResNets (prune the block-internal convs, leave residual-tied convs alone).
* :func:`get_mobilenet_pruning_graph` — new: the hidden channels of inverted-residual blocks
  (expand conv -> BN -> depthwise conv -> BN -> project conv).
* :func:`discover_cascade` — new: NaN-probe based consumer discovery for arbitrary graphs
  (SURVEY.md §7.3 hard part 6).
* :func:`is_channel_gate` — new: structural test for squeeze-and-excitation style gates, which
  the pruner and the probe treat as one per-channel pass-through module.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
from torch.nn.modules.activation import Hardswish, LeakyReLU, ReLU, ReLU6, RReLU, Sigmoid, Softplus, Tanh
from torch.nn.modules.batchnorm import _BatchNorm
from torch.nn.modules.conv import _ConvNd
from torch.nn.modules.dropout import _DropoutNd

logger = logging.getLogger("torchpruner")

# (Hardswish: the unit activation of MobileNetV3; scored after it like a ReLU6 of MobileNetV2)
ACTIVATIONS = (ReLU, ReLU6, RReLU, LeakyReLU, Sigmoid, Softplus, Tanh, Hardswish)


def _dense_fc(m) -> bool:
    if isinstance(m, nn.Linear):
        return m.weight.dim() == 2
    return (isinstance(m, nn.Conv2d) and m.groups == 1 and m.weight.dim() == 4
            and tuple(m.weight.shape[2:]) == (1, 1))


def is_channel_gate(module) -> bool:
    """Whether ``module`` is a channel gate: its output is its input times a per-channel factor
    computed from the pooled input (torchvision's ``SqueezeExcitation``). Structural: attributes
    ``fc1`` and ``fc2``, each a dense 1x1 ``Conv2d`` (groups 1) or an ``nn.Linear``, with ``fc2``'s
    output width equal to ``fc1``'s input width (both read from the weight tensors, not from the
    modules' metadata, which user code may leave stale).

    The test does not look at what the module computes. Any module with such ``fc1`` / ``fc2``
    attributes matches, a transformer MLP block (d -> k -> d) for one, whose output is NOT its
    input times a per-channel factor. The pruner and :func:`discover_cascade` pass the input of
    every match through during their probe, so for such a non-gate they would report a cascade
    that is wrong (every consumer behind it sees the pruned channels of the block's INPUT). A
    model that holds such blocks must not list them as cascading modules, and
    :func:`discover_cascade` must be called with ``gates=False`` for it."""
    fc1, fc2 = getattr(module, "fc1", None), getattr(module, "fc2", None)
    if not (isinstance(module, nn.Module) and _dense_fc(fc1) and _dense_fc(fc2)):
        return False
    return fc2.weight.shape[0] == fc1.weight.shape[1]


def gate_inner_modules(model: nn.Module) -> set:
    """ids of every module nested inside a channel gate of ``model`` (the gates themselves not)."""
    inner = set()
    for m in model.modules():
        if is_channel_gate(m):
            inner.update(id(c) for c in m.modules() if c is not m)
    return inner


def find_best_module_for_attributions(model: nn.Module, module: nn.Module) -> nn.Module:
    """Return the last BatchNorm/activation that directly follows ``module``.

    Relies on registration order == execution order, exactly like the reference.
    Quirk preserved: if the chain of BN/activations runs to the end of ``modules()`` the
    original ``module`` is returned (reference graph.py:34).
    """
    modules = list(model.modules())
    try:
        current_idx = next(i for i, m in enumerate(modules) if m is module)
    except StopIteration:
        logger.error("Provided module is not in model")
        return module
    eval_module = module
    for next_module in modules[current_idx + 1:]:
        if isinstance(next_module, _BatchNorm):
            logger.info("BatchNorm detected: shifting evaluation after %s", next_module)
            eval_module = next_module
        elif isinstance(next_module, ACTIVATIONS):
            logger.info("Activation detected: shifting evaluation after %s", next_module)
            eval_module = next_module
        else:
            return eval_module
    return module


def get_vgg_pruning_graph(vgg: nn.Module):
    """List of ``(prunable_module, [cascading modules])`` for a chain CNN, last layer first.

    The cascade of a layer is ``[next Linear/Conv2d, BatchNorm2d..., Dropout...]`` — the same
    order the reference builds with append + reverse (graph.py:47-58) — and the final
    classifier is dropped.
    """
    pruning = []
    current = None
    for module in vgg.modules():
        if isinstance(module, (nn.Linear, nn.Conv2d)):
            if current is not None:
                pruning[-1][1].append(module)
                pruning[-1][1].reverse()
            current = module
            pruning.append((module, []))
        elif isinstance(module, (nn.BatchNorm2d, nn.Dropout)) and current is not None:
            pruning[-1][1].append(module)
    return pruning[::-1][1:]


def get_resnet_pruning_graph(model: nn.Module):
    """Residual-aware pruning graph for torchvision-style ResNets.

    For every residual block, the output channels of each internal conv (``conv1`` and, in a
    bottleneck, ``conv2``) can be pruned freely: the cut cascades into the block's BN and the
    next conv's input. The last conv of a block (``conv2`` of a BasicBlock / ``conv3`` of a
    Bottleneck) and the ``downsample`` convs write into the residual stream and stay intact.
    Returned last-block-first, like :func:`get_vgg_pruning_graph`.
    """
    graph = []
    for block in model.modules():
        convs = [(n, m) for n, m in block.named_children() if isinstance(m, nn.Conv2d) and n.startswith("conv")]
        if len(convs) < 2 or not any(n.startswith("bn") for n, _ in block.named_children()):
            continue
        convs.sort(key=lambda nm: int(nm[0][4:]) if nm[0][4:].isdigit() else 0)
        for i in range(len(convs) - 1):
            name, conv = convs[i]
            bn = getattr(block, "bn" + name[4:], None)
            nxt = convs[i + 1][1]
            cascade = [nxt] + ([bn] if isinstance(bn, _BatchNorm) else [])
            cascade.reverse()  # BN first, then the consumer conv (matches get_vgg_pruning_graph)
            graph.append((conv, cascade))
    return graph[::-1]


def get_mobilenet_pruning_graph(model: nn.Module):
    """Pruning graph for MobileNetV2-style nets (inverted-residual blocks with a ``.conv``
    Sequential of expand 1x1 conv, BN, activation, depthwise conv, BN, activation, project 1x1
    conv, BN).

    The expanded (hidden) channels of a block are private to it: cutting hidden channel c of the
    expand conv cascades into its BN, the depthwise conv (a per-channel pass-through: one k x k
    filter), the depthwise BN and one input column of the project conv. Blocks without expansion,
    the stem, the project convs and the head write to the residual / inter-block stream and stay
    intact, as in :func:`get_resnet_pruning_graph`. Returned last-block-first.

    MobileNetV3-style blocks (torchvision's layout, :func:`_v3_block_entry`) are taken too: their
    entry is ``(expand conv, [BN, depthwise conv, BN, gate?, project conv])``, the
    squeeze-and-excitation gate (:func:`is_channel_gate`) listed as a whole where the block has one.
    """
    graph = []
    for block in model.modules():
        seq = getattr(block, "conv", None)
        if not isinstance(seq, nn.Sequential):
            entry = _v3_block_entry(block)
            if entry is not None:
                graph.append(entry)
            continue
        layers = [m for m in seq.modules() if isinstance(m, (nn.Conv2d, _BatchNorm))]
        if len(layers) != 6 or not all(isinstance(layers[i], nn.Conv2d) for i in (0, 2, 4)) \
                or not all(isinstance(layers[i], _BatchNorm) for i in (1, 3, 5)):
            continue
        expand, bn_expand, dw, bn_dw, project = layers[:5]
        if expand.groups != 1 or project.groups != 1 or dw.groups == 1 \
                or not (dw.groups == dw.in_channels == dw.out_channels == expand.out_channels):
            continue
        graph.append((expand, [bn_expand, dw, bn_dw, project]))
    return graph[::-1]


def _v3_block_entry(block):
    """The graph entry of a MobileNetV3-style block (torchvision's layout: ``block.block`` is a
    Sequential of ``[expand unit,] depthwise unit, [gate,] project unit``, every unit a Sequential
    that starts with ``Conv2d, BatchNorm``), or None (no expansion, or another layout)."""
    seq = getattr(block, "block", None)
    if not isinstance(seq, nn.Sequential):
        return None
    mods = list(seq)
    gates = [m for m in mods if is_channel_gate(m)]
    units = [m for m in mods if not is_channel_gate(m)]
    if len(units) != 3 or len(gates) > 1 or (gates and mods[2] is not gates[0]):
        return None
    if not all(isinstance(u, nn.Sequential) and len(u) >= 2 and isinstance(u[0], nn.Conv2d)
               and isinstance(u[1], _BatchNorm) for u in units):
        return None
    (expand, bn_expand), (dw, bn_dw), project = units[0][:2], units[1][:2], units[2][0]
    if expand.groups != 1 or project.groups != 1 or dw.groups == 1 \
            or not (dw.groups == dw.in_channels == dw.out_channels == expand.out_channels):
        return None
    return expand, [bn_expand, dw, bn_dw, *gates, project]


def discover_cascade(model: nn.Module, module: nn.Module, input_size, device=None, candidates=None, gates=True):
    """Find the modules whose *input* channels depend on ``module``'s output channels.

    NaN-probe: nanify channel 0 of ``module``'s output, run one eval-mode no-grad forward on a
    random (2, *input_size) batch and report every Linear/Conv/BatchNorm/Dropout whose input
    picked up NaNs (the same trick the pruner uses, pruner.py:21-57, generalised to discover
    the cascade rather than requiring the user to spell it out). A channel gate
    (:func:`is_channel_gate`) is a candidate as a whole, the modules inside it are not, and the
    probe passes its input through: a gate pools and mixes every channel, so it would otherwise
    spread one NaN channel over all of them and hide every consumer behind it. ``gates=False``
    turns that off (no module is treated as a gate: the plain probe), for models whose ``fc1`` /
    ``fc2`` blocks are no gates (see :func:`is_channel_gate`).
    """
    if device is None:
        device = next(model.parameters()).device
    if candidates is None:
        inner = gate_inner_modules(model) if gates else set()
        candidates = [m for m in model.modules() if m is not module and id(m) not in inner and
                      (isinstance(m, (nn.Linear, _ConvNd, _BatchNorm, _DropoutNd)) or (gates and is_channel_gate(m)))]
    found = []
    handles = []

    def nanify(_m, _i, out):
        out = out.clone()
        out[:, 0] = float("nan")
        return out

    def detect(m):
        def _h(_m, inp, _o):
            x = inp[0]
            v = x
            while v.dim() > 2:
                v = v.sum(-1)
            nan = torch.isnan(v.sum(0))
            # a direct consumer sees NaN in *some* input channels; anything past a
            # channel-mixing op sees NaN everywhere and is not part of the cascade
            if nan.any() and not nan.all():
                found.append(m)
            if gates and is_channel_gate(m):
                return x
        return _h

    handles.append(module.register_forward_hook(nanify))
    for m in candidates:
        handles.append(m.register_forward_hook(detect(m)))
    hooked = {id(m) for m in candidates}
    for m in model.modules():  # gates outside a caller's candidate list pass through as well
        if gates and is_channel_gate(m) and id(m) not in hooked and m is not module:
            handles.append(m.register_forward_hook(lambda _m, inp, _o: inp[0]))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            model(torch.rand((2,) + tuple(input_size), device=device))
    finally:
        for h in handles:
            h.remove()
        model.train(was_training)
    seen = []
    for m in found:
        if not any(m is s for s in seen):
            seen.append(m)
    return seen
