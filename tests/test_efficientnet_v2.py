"""EfficientNetV2 on the CPU: the model's tree and keys, the pruning-graph entries of its Fused-MBConv blocks,
the engine plan (accepted blocks, rejections that name the block) and the torch bodies of the SiLU-on-load
project GEMM ops against ``F.silu`` + matmul + autograd in float64."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def _model():
    from torchpruner_amd.models import efficientnet_v2
    torch.manual_seed(0)
    return efficientnet_v2(0.25, 0.34, 10, small_input=True).eval()


def test_tree_and_state_dict_keys_follow_torchvision():
    from torchpruner_amd.models import FusedMBConv, MBConv, efficientnet_v2_s
    m = efficientnet_v2_s()
    assert sum(p.numel() for p in m.parameters()) == 21_458_488  # torchvision's efficientnet_v2_s
    assert [len(st) for st in list(m.features)[1:-1]] == [2, 4, 4, 6, 9, 15]
    assert isinstance(m.features[2][0], FusedMBConv) and isinstance(m.features[4][0], MBConv)
    keys = set(m.state_dict())
    fused = {"features.1.0.block.0.0.weight", "features.2.0.block.0.0.weight", "features.2.0.block.0.1.running_var",
             "features.2.0.block.1.0.weight", "features.2.0.block.1.1.bias"}
    mb = {"features.4.0.block.0.0.weight", "features.4.0.block.1.0.weight", "features.4.0.block.2.fc1.weight",
          "features.4.0.block.2.fc2.bias", "features.4.0.block.3.1.weight", "features.7.1.weight", "classifier.1.weight"}
    assert fused | mb <= keys and "features.1.0.block.1.0.weight" not in keys
    assert m.features[2][0].use_res_connect is False and m.features[2][1].use_res_connect is True
    assert m.features[2][0].stochastic_depth.mode == "row"


def test_graph_entries_and_a_prune_through_them():
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    m = _model()
    graph = get_mobilenet_pruning_graph(m)
    fused = [(mod, c) for mod, c in graph if len(c) == 2]
    assert len(graph) == 17 and len(fused) == 4
    blk = m.features[2][0].block
    assert any(mod is blk[0][0] and c[0] is blk[0][1] and c[1] is blk[1][0] for mod, c in fused)
    rng = np.random.RandomState(0)
    pruner = Pruner(m, (3, 32, 32), "cpu")
    for mod, cascade in graph:
        n = mod.weight.shape[0]
        pruner.prune_model(mod, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    assert blk[0][0].weight.shape[0] == blk[1][0].weight.shape[1] == 22
    assert m(torch.randn(2, 3, 32, 32)).shape == (2, 10)


def test_plan_accepts_fused_blocks_and_names_the_block_it_rejects():
    from torchpruner_amd.engine.mobilenet_engine import EfficientNetEngine, build_efficientnet_plan
    m = _model()
    plan, why = build_efficientnet_plan(m)
    assert plan is not None, why
    kinds = [(b.dw is None, b.project is None) for b in plan.blocks]
    assert kinds.count((True, True)) == 1 and kinds.count((True, False)) == 4 and kinds.count((False, False)) == 13
    eng = EfficientNetEngine(m, plan)
    assert len(eng.eval_modules()) == 4 + 2 * 13 and eng.eval_modules()[0] is m.features[2][0].block[0][2]
    # 8 -> 8, 8 -> 16, 16 -> 16, then (small_input: stride 1, and 48 and 64 both scale to 16) 16 -> 16 twice
    assert [b.shortcut for b in plan.blocks[:5]] == [True, False, True, True, True]
    unit = m.features[2][1].block[0]
    unit[2] = nn.ReLU()
    plan, why = build_efficientnet_plan(m)
    assert plan is None and "features.2.1" in why and "SiLU" in why
    unit[2] = nn.SiLU()
    unit[0] = nn.Conv2d(16, 64, 3, 1, 1, groups=4, bias=False)
    plan, why = build_efficientnet_plan(m)
    assert plan is None and "features.2.1" in why and "grouped" in why


@pytest.mark.parametrize("B,HW,C,Co", [(2, 9, 8, 4), (1, 70, 12, 8)])
def test_torch_bodies_equal_silu_matmul_and_autograd(B, HW, C, Co):
    from torchpruner_amd import ops
    g = torch.Generator().manual_seed(HW)
    z = (torch.randn(B * HW, C, generator=g, dtype=torch.float64) * 3).requires_grad_()
    wt, res, gr = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((C, Co), (B * HW, Co), (B * HW, Co)))
    scale, shift = torch.rand(Co, generator=g, dtype=torch.float64) + 0.5, torch.randn(Co, generator=g, dtype=torch.float64)
    apoz = torch.zeros(B, C, dtype=torch.float64)
    out = ops.silu_project_fwd(z.detach(), wt, scale, shift, res, apoz)
    a = F.silu(z)
    a.retain_grad()
    ref = (a @ wt) * scale + shift + res
    torch.testing.assert_close(out, ref.detach(), rtol=1e-13, atol=1e-13)
    assert torch.equal(apoz, (z.detach() > 0).view(B, HW, C).sum(1).double())
    ref.backward(gr)
    for mode in (0, 1):
        tay = torch.zeros(ops.silu_project_tay_slots(HW, C), B, C, dtype=torch.float64)
        dz = ops.silu_project_dgrad(gr, z.detach(), (wt * scale).t().contiguous(), tay, mode)
        torch.testing.assert_close(dz, z.grad, rtol=1e-12, atol=1e-13)
        score = a.grad.abs() if mode else -(a.grad * a.detach())
        torch.testing.assert_close(tay.sum(0), score.view(B, HW, C).sum(1), rtol=1e-12, atol=1e-13)
    assert ops.silu_project_tay_slots(64, 8) == 1 and ops.silu_project_tay_slots(65, 8) == 2 and \
        ops.silu_project_tay_slots(1, 8) == 1 and ops.silu_project_tay_slots(150, 8) == 4
