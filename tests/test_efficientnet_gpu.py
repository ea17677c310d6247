"""An EfficientNet training step with the fused BN + SiLU tails and the SiLU gates on the native kernels.
efficientnet(0.25, 0.34, 10, small_input=True): ten blocks, one without an expand unit, a 5x5 stride-2
layer; B = 4 at 32 px; dropout and stochastic depth off. Against the model in float64 on the library path
with the bounds of test_mobilenet_gpu._compare_step (which itself compares with fp32 autograd), as
test_mobilenet_v3_hswish_gpu._assert_same_step applies them. Dense, and with two blocks cut to odd widths."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_mobilenet_gpu import ROOT
from test_mobilenet_v3_hswish_gpu import _assert_same_step, _batch, _gpu_model, _node_names

pytestmark = pytest.mark.gpu


def _tiny(pruned=False):
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.models import StochasticDepth, efficientnet
    torch.manual_seed(0)
    model = efficientnet(0.25, 0.34, 10, small_input=True)
    if pruned:
        for module, cascade in get_mobilenet_pruning_graph(model)[2:4]:
            n = module.weight.shape[0]  # n / 2 - 1 channels stay: odd
            Pruner(model, (3, 32, 32), "cpu").prune_model(module, list(range(n // 2 + 1)), cascade)
    gen = torch.Generator().manual_seed(5)
    for m in model.modules():
        if isinstance(m, (nn.Dropout, StochasticDepth)):
            m.p = 0.0
        elif isinstance(m, nn.Conv2d) and m.bias is not None:  # the gates' fcs: no symmetric start
            nn.init.normal_(m.bias, std=0.5, generator=gen)
    return model.train()


def _pairs(model):
    return [(a, b) for s in model.modules() if type(s) is nn.Sequential
            for a, b in zip(list(s), list(s)[1:]) if isinstance(a, nn.BatchNorm2d) and type(b) is nn.SiLU]


def _step(model, x, y, native):
    """(loss, gradients, buffers, node names, (bn_silu tails, gate forwards, gate backwards)) of one step."""
    from torchpruner_amd.engine.train import FUSE_COUNTS, SE_COUNTS, native_convs
    count = lambda: (FUSE_COUNTS["bn_silu"], SE_COUNTS["fwd"], SE_COUNTS["bwd"])
    model.zero_grad(set_to_none=True)
    before = count()
    with native_convs(model, enable=native):
        loss = F.cross_entropy(model(x), y)
        names = _node_names(loss)
        loss.backward()
    grads, bufs = ({n: t.detach().double().cpu() for n, t in d} for d in
                   (((n, p.grad) for n, p in model.named_parameters()), model.named_buffers()))
    return float(loss.detach()), grads, bufs, names, tuple(a - b for a, b in zip(count(), before))


def _fp64(base):
    return _step(copy.deepcopy(base).double().train(), *_batch(dtype=torch.float64), False)


@pytest.mark.parametrize("pruned", [False, True], ids=["dense", "pruned"])
def test_fused_step_matches_fp64(cuda, pruned):
    from torchpruner_amd.engine.train import native_convs
    base = _tiny(pruned)
    dws = [m for m in base.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(dws) == 10 and len(_pairs(base)) == 21  # one block has no expand unit; a gate per block
    assert any(m.kernel_size == (5, 5) and m.stride == (2, 2) for m in dws) and sum(m.groups % 2 for m in dws) == 2 * pruned
    x, y = _batch(cuda)
    got = _step(_gpu_model(base, cuda), x, y, True)
    assert got[4] == (21, 10, 10), got[4]
    # no SiLU node of autograd's is left (out-of-place SiLUs: an in-place op on a view hides behind CopySlices)
    m = _gpu_model(base, cuda)
    for a in (a for a in m.modules() if isinstance(a, nn.SiLU)):
        a.inplace = False
    with native_convs(m):
        names = _node_names(F.cross_entropy(m(x), y))
    assert not any(k.startswith("SiluBackward") for k in names) and sum(k.startswith("_NativeBNSiLU") for k in names) == 21
    _assert_same_step(got, _fp64(base), "pruned" if pruned else "dense")


def test_hooked_silu_takes_its_own_forward(cuda):
    model, (x, y), seen = _gpu_model(_tiny(), cuda), _batch(cuda), []
    h = _pairs(model)[3][1].register_forward_hook(lambda m, i, o: seen.append(type(m).__name__))
    hooked = _step(model, x, y, True)
    h.remove()
    assert hooked[4][0] == 20 and seen == ["SiLU"] and _step(model, x, y, True)[4][0] == 21


def _ab_child():
    """(child process, both switches off) the step still matches float64, no fused tail or gate kernel ran."""
    from torchpruner_amd.engine import train
    assert not train._SILU_FUSE and not train._NATIVE_SE
    base, dev = _tiny(), torch.device("cuda")
    got = _step(_gpu_model(base, dev), *_batch(dev), True)
    assert got[4] == (0, 0, 0), got[4]
    _assert_same_step(got, _fp64(base), "switches off")
    print("silu switches off ok")


def test_switches_off_keep_the_unfused_path(cuda):
    env = dict(os.environ, TORCHPRUNER_FUSE_SILU="0", TORCHPRUNER_NATIVE_SE="0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            "import test_efficientnet_gpu as t; t._ab_child()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "silu switches off ok" in r.stdout, r.stdout + r.stderr
