"""The float64 body of ``ops.silu_prefix_project`` (the oracle of tests/test_silu_prefix_project_gpu.py) against
what it stands for: cnt explicitly masked copies of silu(z) through a 1x1 conv, BN affine and shortcut."""
import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_body_equals_masked_copies_through_a_1x1_conv(with_res):
    from torchpruner_amd import ops
    g = torch.Generator().manual_seed(5)
    B, H, W, C, n, Co, p0, cnt = 2, 3, 5, 12, 10, 8, 2, 6  # two padding channels, nonzero, ranked last
    z = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 3
    w = torch.randn(Co, C, generator=g, dtype=torch.float64)
    scale, shift = torch.rand(Co, generator=g, dtype=torch.float64) + 0.5, torch.randn(Co, generator=g, dtype=torch.float64)
    res = torch.randn(B, H, W, Co, generator=g, dtype=torch.float64) if with_res else None
    perm = torch.randperm(n, generator=g)
    rank = torch.full((C,), n + 1)
    rank[perm] = torch.arange(n)
    got = ops.silu_prefix_project(z.view(-1, C), (w * scale[:, None]).t(), shift, None if res is None else res.view(-1, Co),
                                  perm.int(), rank.int(), p0, cnt)
    assert got.shape == (cnt, B * H * W, Co) and got.dtype == torch.float64
    a = F.silu(z).permute(0, 3, 1, 2)
    for j in range(cnt):
        masked = a.clone()
        masked[:, perm[:p0 + j]] = 0.0
        ref = F.conv2d(masked, w.view(Co, C, 1, 1)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if with_res:
            ref = ref + res.permute(0, 3, 1, 2)
        torch.testing.assert_close(got[j].view(B, H, W, Co).permute(0, 3, 1, 2), ref, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):  # p0 + cnt - 1 past the permutation
        ops.silu_prefix_project(z.view(-1, C), w.t(), shift, None, perm.int(), rank.int(), 6, 6)
