"""(CPU) models.efficientnet: torchvision's state-dict keys and parameter count, the pruning graph with
the gates listed, the attribution module behind the SiLU, and a cut through one block."""
import torch
import torch.nn as nn

from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
from torchpruner_amd.models import efficientnet, efficientnet_b0
from torchpruner_amd.utils.graph import find_best_module_for_attributions, is_channel_gate


def test_b0_layout_and_parameter_count():
    model = efficientnet_b0().eval()
    sd = model.state_dict()
    assert sum(p.numel() for p in model.parameters()) == 5288548
    for key, shape in (("features.0.0.weight", (32, 3, 3, 3)),
                       ("features.1.0.block.0.0.weight", (32, 1, 3, 3)),  # no expand unit: depthwise first
                       ("features.1.0.block.1.fc1.weight", (8, 32, 1, 1)),
                       ("features.2.0.block.0.0.weight", (96, 16, 1, 1)),
                       ("features.3.0.block.1.0.weight", (144, 1, 5, 5)),
                       ("features.6.3.block.2.fc2.bias", (1152,)), ("features.8.1.running_var", (1280,)),
                       ("classifier.1.weight", (1000, 1280))):
        assert tuple(sd[key].shape) == shape, key
    block = model.features[2][1]
    assert block.use_res_connect and block.stochastic_depth.mode == "row" and 0 < block.stochastic_depth.p < 0.2
    assert type(block.block[2].activation) is nn.SiLU and type(block.block[2].scale_activation) is nn.Sigmoid


def test_graph_attribution_module_and_pruning():
    torch.manual_seed(0)
    model = efficientnet(0.25, 0.34, 10, small_input=True).eval()
    graph = get_mobilenet_pruning_graph(model)
    blocks = [b for s in list(model.features)[1:-1] for b in s]
    assert len(graph) == sum(len(b.block) == 4 for b in blocks) == len(blocks) - 1
    assert all(sum(is_channel_gate(m) for m in cascade) == 1 for _, cascade in graph)
    module, cascade = graph[-1]  # features.2.0: the first expanding block
    blk = model.features[2][0].block
    assert module is blk[0][0] and find_best_module_for_attributions(model, module) is blk[0][2]
    k = module.weight.shape[0] // 2
    Pruner(model, (3, 32, 32), "cpu").prune_model(module, list(range(0, 2 * k, 2)), cascade)
    assert blk[0][0].weight.shape[0] == k and blk[1][0].weight.shape[0] == k and blk[1][0].groups == k
    assert blk[2].fc1.weight.shape[1] == k and blk[2].fc2.weight.shape[0] == k and blk[3][0].weight.shape[1] == k
    assert model(torch.randn(2, 3, 32, 32)).shape == (2, 10)
