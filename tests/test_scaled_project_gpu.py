"""The channel-scaled project GEMM (csrc/kernels/scaled_project.hip, ``ops.scaled_project``) against its
float64 body, and the binding's rejections. Measured figures: profiles/numerics/scaled_project.txt."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

# cnt = 6: above the kernel's JC = 4 copies per pass and no multiple of it (a second pass with a partial
# copy group). The last shape is the only one whose grid reaches the launcher's switch to the 64-row tile
# (89 row tiles x 3 column tiles x 2 copy groups >= 512), with a partial last row and column tile.
SHAPES = list(itertools.product([(3, 49), (5, 1), (2, 196), (70, 4)], [40, 160], [36, 160], [1, 2, 6]))
SHAPES.append(((29, 196), 160, 160, 6))


def _case(B, HW, C, Co, cnt, with_res):
    g = torch.Generator().manual_seed(B * 1000 + HW + C + Co + cnt)
    N = B * HW
    a = torch.rand(N, C, generator=g) * 6
    sc = torch.rand(cnt, B, C, generator=g)
    sc = torch.where(torch.rand(cnt, B, C, generator=g) < 0.25, torch.zeros(()), sc)  # masked channels
    wt = torch.randn(C, Co, generator=g)
    bias = torch.randn(cnt, B, Co, generator=g) * 3
    res = torch.randn(N, Co, generator=g) * 3 if with_res else None
    return a, sc, wt, bias, res


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape,C,Co,cnt", SHAPES)
def test_kernel_matches_the_fp64_body(cuda, shape, C, Co, cnt, with_res):
    """|out - ref| <= (C + 5) 2^-24 (|a sc| @ |wt| + |bias| + |res|) elementwise: one rounding for the
    scale product, one per multiply-add step, the rest for the bias and residual adds (derived, not
    measured); two launches return the same bits."""
    from torchpruner_amd import ops
    B, HW = shape
    a, sc, wt, bias, res = _case(B, HW, C, Co, cnt, with_res)
    dev = [None if t is None else t.to(cuda) for t in (a, sc, wt, bias, res)]
    out = ops.scaled_project(*dev, hw=HW)
    assert out.shape == (cnt, B * HW, Co) and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(out, ops.scaled_project(*dev, hw=HW))
    a64, sc64, wt64, b64 = a.double(), sc.double(), wt.double(), bias.double()
    r64 = None if res is None else res.double()
    ref = ops.scaled_project(a64, sc64, wt64, b64, r64, hw=HW)
    mag = ops.scaled_project(a64, sc64, wt64.abs(), b64.abs(), None if res is None else r64.abs(), hw=HW)
    bound = (C + 5) * 2.0 ** -24 * mag
    ratio = float(((out.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"scaled_project B={B} HW={HW} C={C} Co={Co} cnt={cnt} res={int(with_res)}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def _reject_args(name, cuda):
    a, sc, wt, bias, res = (t.to(cuda) for t in _case(3, 49, 40, 36, 2, True))
    hw = 49
    if name == "cnt0":
        sc, bias = sc[:0], bias[:0]
    elif name == "hw0":
        hw = 0
    elif name == "hw_not_dividing":
        hw = 50
    elif name == "sc_wrong_B":
        sc = sc[:, :2].contiguous()
    elif name == "bias_wrong_Co":
        bias = bias[:, :, :32].contiguous()
    elif name == "C42":
        a, sc, wt = (torch.rand(s, device=cuda) for s in ((147, 42), (2, 3, 42), (42, 36)))
    elif name == "Co30":
        wt, bias, res = (torch.rand(s, device=cuda) for s in ((40, 30), (2, 3, 30), (147, 30)))
    elif name == "noncontiguous_a":
        a = torch.rand(40, 147, device=cuda).t()
    elif name == "cpu_operand":
        wt = wt.cpu()
    elif name == "double_operand":
        sc = sc.double()
    elif name == "res_wrong_shape":
        res = res[:146].contiguous()
    return a, sc, wt, bias, res, hw


@pytest.mark.parametrize("name", ["cnt0", "hw0", "hw_not_dividing", "sc_wrong_B", "bias_wrong_Co", "C42", "Co30",
                                  "noncontiguous_a", "cpu_operand", "double_operand", "res_wrong_shape"])
def test_binding_rejects(cuda, name):
    from torchpruner_amd import ops
    with pytest.raises(RuntimeError):
        ops.require().scaled_project(*_reject_args(name, cuda))
