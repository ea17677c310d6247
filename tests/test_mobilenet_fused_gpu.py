"""The fused MobileNet path of engine/train.py: BN + ReLU6 tails in one apply pass, hidden widths
carried from the expand conv through the depthwise conv into the project conv, and the
inverted-residual block forward (_native_ir_forward), on the pruned model of
tests/test_mobilenet_gpu.py (odd hidden widths; B = 4, 32 px, seed 5, mid-range BN as there and for
the reason given there: the comparison must measure kernels, not ReLU6 decisions flipped by
rounding) against the unfused native path (TORCHPRUNER_FUSE_RELU6=0 at enable time) and against
plain autograd, with that file's bounds."""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_mobilenet_gpu import _mid_range_bn, _pruned_mobilenet, _step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pruned():
    """(model, x, y) on the CPU, built once: the pruned model with mid-range BN, one batch."""
    gen = torch.Generator().manual_seed(5)
    model = _pruned_mobilenet()
    _mid_range_bn(model, gen)
    return model, torch.randn(4, 3, 32, 32, generator=gen), torch.randint(0, 10, (4,), generator=gen)


@pytest.fixture
def setup(cuda, pruned):
    model, x, y = pruned
    model = copy.deepcopy(model).to(cuda).to(memory_format=torch.channels_last).train()
    return model, x.to(cuda).contiguous(memory_format=torch.channels_last), y.to(cuda)


def _counts(tr):
    return dict(tr.FUSE_COUNTS), dict(tr.DW_COUNTS)


def _delta(tr, before):
    return ({k: tr.FUSE_COUNTS[k] - before[0][k] for k in before[0]},
            {k: tr.DW_COUNTS[k] - before[1][k] for k in before[1]})


def _graph_names(model, x, y, tr):
    """Names of the autograd nodes of one native training forward."""
    with tr.native_convs(model):
        loss = F.cross_entropy(model(x), y)
    seen, stack, names = set(), [loss.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def test_fused_step_matches_unfused_and_autograd(setup, monkeypatch):
    from torchpruner_amd.engine import train as tr
    from torchpruner_amd.models.mobilenet import InvertedResidual
    base, x, y = setup
    models = {k: copy.deepcopy(base) for k in ("fused", "unfused", "autograd")}
    monkeypatch.setattr(tr, "_MB_FUSE", True)
    before = _counts(tr)
    l_f, g_f = _step(models["fused"], x, y, True)
    fuse, dw = _delta(tr, before)
    monkeypatch.setattr(tr, "_MB_FUSE", False)
    before = _counts(tr)
    l_u, g_u = _step(models["unfused"], x, y, True)
    fuse_u, dw_u = _delta(tr, before)
    l_a, g_a = _step(models["autograd"], x, y, False)
    print(f"loss fused {l_f:.7f} unfused {l_u:.7f} autograd {l_a:.7f}")

    # counters, derived from the model
    m = models["fused"]
    dws = [c for c in m.modules() if isinstance(c, torch.nn.Conv2d) and c.groups != 1]
    n_ir = sum(isinstance(c, InvertedResidual) for c in m.modules())
    n_relu6 = sum(isinstance(c, torch.nn.ReLU6) for c in m.modules())
    n_carried = sum(c.weight.shape[0] % 8 != 0 for c in dws)
    assert n_ir == 17 and n_relu6 == 35 and n_carried > 0
    assert (fuse["ir_block"], fuse["bn_relu6"], fuse["dw_carried"]) == (n_ir, n_relu6, n_carried), fuse
    assert (fuse_u["ir_block"], fuse_u["bn_relu6"], fuse_u["dw_carried"]) == (0, 0, 0), fuse_u
    assert dw == dw_u == {"fwd": len(dws), "dgrad": len(dws), "wgrad": len(dws)}, (dw, dw_u)

    # one step: the bounds of tests/test_mobilenet_gpu.py
    for what, l_ref, g_ref, ref_model in (("unfused", l_u, g_u, models["unfused"]),
                                          ("autograd", l_a, g_a, models["autograd"])):
        assert abs(l_f - l_ref) < 1e-4 * max(1.0, abs(l_ref)), what
        worst = 0.0
        for (name, _), a, b in zip(m.named_parameters(), g_f, g_ref):
            err, lim = (a - b).abs().max().item(), 2e-3 * b.abs().max().item() + 1e-6
            worst = max(worst, err / lim)
            assert torch.isfinite(a).all() and err <= lim, (what, name, err, lim)
        print(f"vs {what}: worst gradient error / bound {worst:.3f}")
        for (n1, b1), (_, b2) in zip(m.named_buffers(), ref_model.named_buffers()):
            torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-4, atol=1e-5, msg=f"{what}: {n1}")


def test_fused_graph_has_no_hardtanh_and_no_slice(setup, monkeypatch):
    """On the fused path no ATen hardtanh runs and no hidden activation is sliced; the unfused path
    (the one before the fusions) has both kinds of node."""
    from torchpruner_amd.engine import train as tr
    base, x, y = setup
    monkeypatch.setattr(tr, "_MB_FUSE", True)
    names = _graph_names(copy.deepcopy(base), x, y, tr)
    # (an in-place ReLU6 on a slice turns the slice's node into CopySlices: neither may appear)
    assert not [n for n in names if n.startswith(("Hardtanh", "SliceBackward", "CopySlices"))], sorted(set(names))
    assert sum(n.startswith("_NativeBNAct") for n in names) == 35 + 17  # ReLU6 tails + linear bottlenecks
    assert sum(n.startswith("_NativeDWConv2d") for n in names) == 17
    monkeypatch.setattr(tr, "_MB_FUSE", False)
    names = _graph_names(copy.deepcopy(base), x, y, tr)
    assert any(n.startswith("Hardtanh") for n in names)
    assert any(n.startswith(("SliceBackward", "CopySlices")) for n in names), sorted(set(names))


def test_hooked_block_takes_the_fallback(setup, monkeypatch):
    """A forward hook on a module the fused block forward would skip: that block runs its own
    forward (the hook fires), the others stay fused."""
    from torchpruner_amd.engine import train as tr
    from torchpruner_amd.models.mobilenet import InvertedResidual
    base, x, y = setup
    monkeypatch.setattr(tr, "_MB_FUSE", True)
    model = copy.deepcopy(base)
    blocks = [m for m in model.modules() if isinstance(m, InvertedResidual)]
    fired = []
    h = blocks[5].conv[1][1].register_forward_hook(lambda m, i, o: fired.append(tuple(o.shape)))
    before = _counts(tr)
    l_h, g_h = _step(model, x, y, True)
    h.remove()
    fuse, dw = _delta(tr, before)
    assert len(fired) == 1 and fired[0][1] == blocks[5].conv[1][1].num_features
    assert fuse["ir_block"] == len(blocks) - 1, fuse
    assert dw == {"fwd": 17, "dgrad": 17, "wgrad": 17}
    l_f, g_f = _step(copy.deepcopy(base), x, y, True)
    assert abs(l_h - l_f) < 1e-4 * max(1.0, abs(l_f))
    for a, b in zip(g_h, g_f):
        assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-6


def test_eval_mode_is_the_modules_own_forward(setup, monkeypatch):
    from torchpruner_amd.engine import train as tr
    base, x, y = setup
    monkeypatch.setattr(tr, "_MB_FUSE", True)
    model = copy.deepcopy(base).eval()
    before = _counts(tr)
    with torch.no_grad():
        ref = model(x)
        with tr.native_convs(model, fuse=False):
            plain = model(x)
        with tr.native_convs(model, fuse=True) as switched:
            assert any(type(m).__name__ == "InvertedResidual" for m in switched)
            got = model(x)
    assert torch.equal(got, plain)  # the block path adds nothing in eval mode
    assert _delta(tr, before)[0]["ir_block"] == 0
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert not any("forward" in m.__dict__ for m in model.modules())  # everything restored


def test_unpruned_shortcut_block_matches_fp64(cuda, monkeypatch):
    """A dense block with the shortcut, alone: output and input gradient vs fp64 autograd at the
    tolerances of test_bn_on_padded_activation."""
    from torchpruner_amd.engine import train as tr
    from torchpruner_amd.models import mobilenet_v2
    monkeypatch.setattr(tr, "_MB_FUSE", True)
    torch.manual_seed(3)
    net = mobilenet_v2(10, width_mult=0.5, small_input=True)
    block = next(m for m in net.modules() if type(m).__name__ == "InvertedResidual" and m.use_res_connect)
    gen = torch.Generator().manual_seed(5)
    _mid_range_bn(block, gen)
    cin = block.conv[0][0].in_channels
    block = block.to(cuda).to(memory_format=torch.channels_last).train()
    b64 = copy.deepcopy(block).double()
    x = torch.randn(2, cin, 8, 8, generator=gen).to(cuda).contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, cin, 8, 8, generator=gen).to(cuda).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    before = _counts(tr)
    with tr.native_convs(block):
        out = block(x)
        out.backward(g)
    fuse, _ = _delta(tr, before)
    assert (fuse["ir_block"], fuse["bn_relu6"], fuse["dw_carried"]) == (1, 2, 0), fuse
    x64 = x.detach().double().requires_grad_(True)
    o64 = b64(x64)
    o64.backward(g.double())
    torch.testing.assert_close(out.double(), o64, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-4, atol=1e-4)
    for (n, p), p64 in zip(block.named_parameters(), b64.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, n
    for (n, b), r in zip(block.named_buffers(), b64.buffers()):
        torch.testing.assert_close(b.double(), r.double(), rtol=1e-4, atol=1e-5, msg=n)
