"""Structured pruning through squeeze-and-excitation gates: the cascade expand conv -> BN ->
depthwise conv -> BN -> gate -> project conv of a MobileNetV3 block, the rejections that leave the
model untouched, the MobileNetV3 pruning graph against the NaN probe, and the checkpoint round trip."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from torchpruner_amd import Pruner, get_mobilenet_pruning_graph, is_channel_gate
from torchpruner_amd.checkpoint import load_pruned, save_pruned
from torchpruner_amd.models import mobilenet_v2, mobilenet_v3_small
from torchpruner_amd.models.mobilenet_v3 import SMALL, SqueezeExcitation
from torchpruner_amd.utils import discover_cascade

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]


def _dev(dev):
    if dev == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device(dev)


def _chain(d):
    """Conv1x1(8->24) BN Hardswish Conv3x3(24, groups=24) BN Hardswish SE(24, 8) Conv1x1(24->8) BN."""
    torch.manual_seed(0)
    model = nn.Sequential(
        nn.Conv2d(8, 24, 1, bias=False), nn.BatchNorm2d(24), nn.Hardswish(),
        nn.Conv2d(24, 24, 3, padding=1, groups=24, bias=False), nn.BatchNorm2d(24), nn.Hardswish(),
        SqueezeExcitation(24, 8),
        nn.Conv2d(24, 8, 1, bias=False), nn.BatchNorm2d(8))
    for i, m in enumerate(model):
        if isinstance(m, nn.BatchNorm2d):  # non-trivial eval-mode statistics
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            if i != 4:  # the depthwise BN keeps mean 0 / shift 0: a zeroed hidden channel stays zero
                m.running_mean.uniform_(-0.5, 0.5)
                m.bias.data.uniform_(-0.5, 0.5)
    model[6].fc1.bias.data.uniform_(-0.5, 0.5)
    model[6].fc2.bias.data.uniform_(-0.5, 0.5)
    return model.to(d)


def _shapes(model):
    return {n: tuple(t.shape) for n, t in model.state_dict().items()}


def test_is_channel_gate():
    se = SqueezeExcitation(24, 8)
    assert is_channel_gate(se)
    assert not is_channel_gate(se.fc1) and not is_channel_gate(nn.Sequential(se))

    class LinearGate(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = nn.Linear(12, 3), nn.Linear(3, 12)

    assert is_channel_gate(LinearGate())
    se.fc2 = nn.Conv2d(8, 20, 1)  # fc2's outputs are not fc1's inputs
    assert not is_channel_gate(se)
    se.fc2 = nn.Conv2d(8, 24, 3, padding=1)  # no 1x1 conv
    assert not is_channel_gate(se)
    se.fc2 = nn.Conv2d(8, 24, 1, groups=2)
    assert not is_channel_gate(se)
    se.fc2 = nn.Conv2d(8, 24, 1)
    se.fc2.out_channels = 99  # stale metadata: the widths are the weight tensors'
    assert is_channel_gate(se)


def test_native_eligibility_reads_the_children():
    from torchpruner_amd.engine.train import se_eligible
    se = SqueezeExcitation(24, 8)
    assert se_eligible(se)
    se.scale_activation = nn.Sigmoid()
    assert se_eligible(se)
    se.activation = nn.SiLU()  # EfficientNet's inner activation: the module's forward
    assert not se_eligible(se)
    se.activation = nn.ReLU()
    for pool in (nn.AdaptiveAvgPool2d(None), nn.AdaptiveAvgPool2d((None, 1)), nn.AdaptiveAvgPool2d(2), nn.AvgPool2d(7)):
        se.avgpool = pool
        assert not se_eligible(se)
    se.avgpool = nn.AdaptiveAvgPool2d((1, 1))
    assert se_eligible(se)
    se.scale_activation = nn.Tanh()
    assert not se_eligible(se)


def test_discover_cascade_without_gates_for_mlp_blocks():
    """A d -> k -> d block with fc1 / fc2 matches the structural test without being a gate:
    ``gates=False`` gives the plain probe, which finds its fc1 as the consumer."""

    class Mlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = nn.Linear(6, 12), nn.Linear(12, 6)

        def forward(self, x):
            return self.fc2(torch.relu(self.fc1(x)))

    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(4, 6), Mlp(), nn.Linear(6, 2))
    assert is_channel_gate(model[1])
    assert discover_cascade(model, model[0], (4,), gates=False) == [model[1].fc1]
    assert discover_cascade(model, model[0], (4,)) == [model[1], model[2]]  # what a real gate would give


@pytest.mark.parametrize("dev", DEVICES)
def test_gate_cascade(dev):
    d = _dev(dev)
    model = _chain(d)
    expand, bn1, _, dw, bn2, _, gate, project, _ = model
    cascade = discover_cascade(model, expand, (8, 9, 9))
    assert cascade == [bn1, dw, bn2, gate, project]
    x = torch.randn(3, 8, 9, 9, device=d)
    idx = [1, 5, 7]
    model.eval()
    opt = torch.optim.SGD(model.parameters(), lr=0.0, momentum=0.9)
    model(x).square().mean().backward()
    opt.step()  # (lr 0, eval mode: gradients and momentum buffers exist, the model is unchanged)
    ref = copy.deepcopy(model)
    with torch.no_grad():  # the unpruned model with the three hidden channels zeroed after the first activation
        ref[6].fc2.weight[idx] = 0  # (their gate factors do not matter: they multiply zeros)
        ref[6].fc2.bias[idx] = 0
        h = ref[:3](x)
        h[:, idx] = 0
        want = ref[3:](h)
    Pruner(model, (8, 9, 9), d, optimizer=opt).prune_model(expand, idx, cascade)
    assert tuple(expand.weight.shape) == (21, 8, 1, 1) and expand.out_channels == 21
    assert tuple(dw.weight.shape) == (21, 1, 3, 3) and dw.groups == dw.in_channels == dw.out_channels == 21
    assert bn1.num_features == bn2.num_features == 21
    assert tuple(gate.fc1.weight.shape) == (8, 21, 1, 1) and gate.fc1.in_channels == 21
    assert tuple(gate.fc1.bias.shape) == (8,)
    assert tuple(gate.fc2.weight.shape) == (21, 8, 1, 1) and gate.fc2.out_channels == 21
    assert tuple(gate.fc2.bias.shape) == (21,)
    assert tuple(project.weight.shape) == (8, 21, 1, 1) and project.in_channels == 21
    assert is_channel_gate(gate)
    for p in (expand.weight, dw.weight, bn1.weight, bn2.bias, gate.fc1.weight, gate.fc1.bias, gate.fc2.weight,
              gate.fc2.bias, project.weight):
        assert opt.state[p]["momentum_buffer"].shape == p.shape
        assert p.grad.shape == p.shape
    with torch.no_grad():
        got = model(x)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("dev", DEVICES)
def test_gate_in_direction_slices_both_fcs(dev):
    d = _dev(dev)
    torch.manual_seed(1)
    gate = SqueezeExcitation(10, 8).to(d)
    w1, b1 = gate.fc1.weight.detach().clone(), gate.fc1.bias.detach().clone()
    w2, b2 = gate.fc2.weight.detach().clone(), gate.fc2.bias.detach().clone()
    Pruner(gate, (10, 6, 6), d).prune_module(gate, [0, 4, 9], "in")
    keep = [1, 2, 3, 5, 6, 7, 8]
    assert torch.equal(gate.fc1.weight, w1[:, keep]) and torch.equal(gate.fc1.bias, b1)
    assert torch.equal(gate.fc2.weight, w2[keep]) and torch.equal(gate.fc2.bias, b2[keep])
    assert gate(torch.randn(2, 7, 6, 6, device=d)).shape == (2, 7, 6, 6)


@pytest.mark.parametrize("dev", DEVICES)
def test_gate_out_direction_rejected(dev):
    d = _dev(dev)
    model = _chain(d)
    before = _shapes(model)
    with pytest.raises(NotImplementedError, match="cascading"):
        Pruner(model, (8, 9, 9), d).prune_module(model[6], [0], "out")
    assert _shapes(model) == before


@pytest.mark.parametrize("dev", DEVICES)
def test_gate_listed_with_inner_module_rejected(dev):
    d = _dev(dev)
    model = _chain(d)
    expand, bn1, _, dw, bn2, _, gate, project, _ = model
    before = _shapes(model)
    with pytest.raises(ValueError, match="gate"):
        Pruner(model, (8, 9, 9), d).prune_model(expand, [1, 5, 7], [bn1, dw, bn2, gate, gate.fc1, project])
    assert _shapes(model) == before and expand.out_channels == 24


@pytest.mark.parametrize("dev", DEVICES)
def test_unlisted_gate_rejected_instead_of_zero_width(dev):
    d = _dev(dev)
    model = _chain(d)
    expand, bn1, _, dw, bn2, _, gate, project, _ = model
    before = _shapes(model)
    # the cascade a user of the plain NaN probe would write: the gate spreads the NaNs over every
    # channel of fc2's input and the project conv's input
    with pytest.raises(ValueError, match="Conv2d"):
        Pruner(model, (8, 9, 9), d).prune_model(expand, [1, 5, 7], [bn1, dw, bn2, gate.fc1, gate.fc2, project])
    assert _shapes(model) == before and bn1.num_features == 24
    # pruning every output stays allowed
    two = nn.Sequential(nn.Linear(4, 3), nn.Linear(3, 2)).to(d)
    Pruner(two, (4,), d).prune_model(two[0], [0, 1, 2], [two[1]])
    assert tuple(two[1].weight.shape) == (2, 0)


@pytest.fixture(scope="module")
def v3_small():
    torch.manual_seed(0)
    return mobilenet_v3_small(10, small_input=True)


def test_v3_graph_matches_probe_and_table(v3_small):
    model = copy.deepcopy(v3_small)
    graph = get_mobilenet_pruning_graph(model)
    blocks = list(model.features)[1:-1]
    expanding = [(b, row) for b, row in zip(blocks, SMALL) if len(b.block) - row[3] == 3]
    assert len(expanding) == 10 and len(graph) == 10  # every block but the first (16 -> 16, no expansion)
    for (module, cascade), (block, row) in zip(graph, expanding[::-1]):  # last block first
        assert module is block.block[0][0]
        assert [is_channel_gate(m) for m in cascade] == [False, False, False] + [True] * row[3] + [False]
        assert cascade[-1] is block.block[-1][0]
        assert cascade == discover_cascade(model, module, (3, 32, 32))


def test_v2_graph_unchanged():
    torch.manual_seed(0)
    model = mobilenet_v2(10, width_mult=0.5, small_input=True)
    want = []
    for block in model.features:
        if hasattr(block, "conv") and len(block.conv) == 4:
            (expand, bn_e, _), (dw, bn_d, _), project, _ = block.conv
            want.append((expand, [bn_e, dw, bn_d, project]))
    got = get_mobilenet_pruning_graph(model)
    assert len(got) == 16 and len(got) == len(want)
    for (gm, gc), (wm, wc) in zip(got, want[::-1]):
        assert gm is wm and len(gc) == len(wc) and all(a is b for a, b in zip(gc, wc))


@pytest.mark.parametrize("dev", DEVICES)
def test_v3_checkpoint_round_trip(dev, v3_small, tmp_path):
    d = _dev(dev)
    model = copy.deepcopy(v3_small).to(d)
    rng = np.random.RandomState(0)
    pruner = Pruner(model, (3, 32, 32), d)
    for module, cascade in get_mobilenet_pruning_graph(model):
        n = module.weight.shape[0]
        pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    x = torch.randn(2, 3, 32, 32, device=d)
    model.eval()
    with torch.no_grad():
        want = model(x)
    path = str(tmp_path / "pruned.pt")
    save_pruned(model, path)
    torch.manual_seed(1)
    fresh = load_pruned(mobilenet_v3_small(10, small_input=True), path).to(d).eval()
    for m in fresh.modules():
        if is_channel_gate(m):
            assert m.fc1.in_channels == m.fc1.weight.shape[1] == m.fc2.out_channels == m.fc2.weight.shape[0]
    with torch.no_grad():
        got = fresh(x)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
