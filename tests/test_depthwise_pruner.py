"""Structured pruning through depthwise convolutions: the cascade expand conv -> BN -> depthwise
conv -> BN -> project conv of an inverted-residual block, rejections that leave the model
untouched, the MobileNetV2 pruning graph against the NaN probe, and the checkpoint round trip."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
from torchpruner_amd.checkpoint import load_pruned, save_pruned
from torchpruner_amd.models import mobilenet_v2
from torchpruner_amd.utils import discover_cascade, find_best_module_for_attributions

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]


def _dev(dev):
    if dev == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device(dev)


def _chain(d):
    """Conv1x1(8->24) BN ReLU6 Conv3x3(24, groups=24, stride 2) BN ReLU6 Conv1x1(24->8) BN."""
    torch.manual_seed(0)
    model = nn.Sequential(
        nn.Conv2d(8, 24, 1, bias=False), nn.BatchNorm2d(24), nn.ReLU6(),
        nn.Conv2d(24, 24, 3, stride=2, padding=1, groups=24, bias=False), nn.BatchNorm2d(24), nn.ReLU6(),
        nn.Conv2d(24, 8, 1, bias=False), nn.BatchNorm2d(8))
    for i, m in enumerate(model):
        if isinstance(m, nn.BatchNorm2d):  # non-trivial eval-mode statistics
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            if i != 4:  # the depthwise BN keeps mean 0 / shift 0: a zeroed hidden channel stays zero
                m.running_mean.uniform_(-0.5, 0.5)
                m.bias.data.uniform_(-0.5, 0.5)
    return model.to(d)


def _shapes(model):
    return {n: tuple(t.shape) for n, t in model.state_dict().items()}


@pytest.mark.parametrize("dev", DEVICES)
def test_depthwise_cascade(dev):
    d = _dev(dev)
    model = _chain(d)
    expand, bn1, act1, dw, bn2, _, project, _ = model
    cascade = discover_cascade(model, expand, (8, 9, 9))
    assert cascade == [bn1, dw, bn2, project]
    assert find_best_module_for_attributions(model, expand) is act1
    x = torch.randn(3, 8, 9, 9, device=d)
    idx = [1, 5, 7]
    model.eval()
    opt = torch.optim.SGD(model.parameters(), lr=0.0, momentum=0.9)
    model(x).square().mean().backward()
    opt.step()  # (lr 0, eval mode: gradients and momentum buffers exist, the model is unchanged)
    with torch.no_grad():  # the unpruned model with the three hidden channels zeroed after the first ReLU6
        h = model[:3](x)
        h[:, idx] = 0
        want = model[3:](h)
    Pruner(model, (8, 9, 9), d, optimizer=opt).prune_model(expand, idx, cascade)
    assert tuple(expand.weight.shape) == (21, 8, 1, 1) and expand.out_channels == 21
    assert tuple(dw.weight.shape) == (21, 1, 3, 3) and dw.bias is None
    assert dw.groups == dw.in_channels == dw.out_channels == 21
    assert bn1.num_features == bn2.num_features == 21 and tuple(bn2.running_var.shape) == (21,)
    assert tuple(project.weight.shape) == (8, 21, 1, 1) and project.in_channels == 21
    for p in (expand.weight, dw.weight, bn1.weight, bn2.bias, project.weight):
        assert opt.state[p]["momentum_buffer"].shape == p.shape
        assert p.grad.shape == p.shape
    with torch.no_grad():
        got = model(x)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("dev", DEVICES)
def test_depthwise_in_direction_slices_filters_and_bias(dev):
    d = _dev(dev)
    torch.manual_seed(1)
    dw = nn.Conv2d(10, 10, 5, padding=2, groups=10).to(d)
    w0, b0 = dw.weight.detach().clone(), dw.bias.detach().clone()
    Pruner(dw, (10, 6, 6), d).prune_module(dw, [0, 4, 9], "in")
    keep = [1, 2, 3, 5, 6, 7, 8]
    assert torch.equal(dw.weight, w0[keep]) and torch.equal(dw.bias, b0[keep])
    assert dw.groups == dw.in_channels == dw.out_channels == 7
    assert dw(torch.randn(2, 7, 6, 6, device=d)).shape == (2, 7, 6, 6)


@pytest.mark.parametrize("dev", DEVICES)
def test_rejected_cascade_leaves_model_untouched(dev):
    d = _dev(dev)
    model = nn.Sequential(nn.Conv2d(4, 8, 1), nn.BatchNorm2d(8), nn.Conv2d(8, 8, 3, padding=1, groups=2),
                          nn.Conv2d(8, 4, 1)).to(d)
    before = _shapes(model)
    with pytest.raises(NotImplementedError):
        Pruner(model, (4, 6, 6), d).prune_model(model[0], [0, 3], [model[1], model[2]])
    assert _shapes(model) == before
    assert model[1].num_features == 8 and model[0].out_channels == 8


@pytest.mark.parametrize("dev", DEVICES)
def test_depthwise_out_direction_rejected(dev):
    d = _dev(dev)
    model = _chain(d)
    before = _shapes(model)
    with pytest.raises(NotImplementedError, match="cascading"):
        Pruner(model, (8, 9, 9), d).prune_module(model[3], [0], "out")
    assert _shapes(model) == before
    # a transposed depthwise conv is rejected like every other grouped conv
    t = nn.ConvTranspose2d(6, 6, 3, groups=6).to(d)
    with pytest.raises(NotImplementedError):
        Pruner(t, (6, 5, 5), d).prune_module(t, [0], "in")


@pytest.fixture(scope="module")
def mobilenet():
    torch.manual_seed(0)
    return mobilenet_v2(10, width_mult=0.5, small_input=True)


def test_mobilenet_graph_matches_probe(mobilenet):
    model = copy.deepcopy(mobilenet)
    graph = get_mobilenet_pruning_graph(model)
    blocks = [b for b in model.features if hasattr(b, "conv")]
    assert len(graph) == sum(len(b.conv) == 4 for b in blocks) == 16  # every block but the t = 1 one
    assert graph[0][0] is blocks[-1].conv[0][0]  # last block first
    for module, cascade in graph:
        assert module.kernel_size == (1, 1) and module.groups == 1
        assert set(cascade) == set(discover_cascade(model, module, (3, 32, 32)))


@pytest.mark.parametrize("dev", DEVICES)
def test_mobilenet_checkpoint_round_trip(dev, mobilenet, tmp_path):
    d = _dev(dev)
    model = copy.deepcopy(mobilenet).to(d)
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
    fresh = load_pruned(mobilenet_v2(10, width_mult=0.5, small_input=True), path).to(d).eval()
    for m in fresh.modules():
        if isinstance(m, nn.Conv2d) and m.groups != 1:
            assert m.groups == m.in_channels == m.out_channels == m.weight.shape[0] and m.weight.shape[1] == 1
    with torch.no_grad():
        got = fresh(x)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
