"""The nine-product algorithm of the 2x2-map conv layers (csrc/kernels/conv2x2_fast.hip) in plain
torch fp64: V = Bt x Bt^T, U = G w G^T, M = sum_c V U, Y = At M At^T must be the 3x3 / pad-1 conv,
forward and data gradient, and the packed U9 operand must be the einsum G w G^T."""
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd.engine.fused_chain import _AT2, _BT2, _G2, fast2x2_weights


def _mats():
    return (torch.tensor(_BT2, dtype=torch.float64), torch.tensor(_G2, dtype=torch.float64),
            torch.tensor(_AT2, dtype=torch.float64))


def _fast2x2(x, w):
    """x (B, C, 2, 2), w (K, C, 3, 3) -> (B, K, 2, 2) with 9 channel products per image."""
    Bt, G, At = _mats()
    V = torch.einsum("ia,bcad,jd->ijbc", Bt, x, Bt)
    U = torch.einsum("ia,kcad,jd->ijkc", G, w, G)
    M = torch.einsum("ijbc,ijkc->ijbk", V, U)  # nine independent (B x C).(C x K) products
    return torch.einsum("ai,ijbk,dj->bkad", At, M, At)


@pytest.mark.parametrize("B,C,K", [(1, 3, 5), (4, 32, 16), (3, 64, 96)])
def test_forward_and_data_gradient_match_conv2d(B, C, K):
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, C, 2, 2, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(K, C, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, padding=1)
    got = _fast2x2(x.detach(), w)
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    # data gradient: the same algorithm on the flipped, transposed weight
    gy = torch.randn(B, K, 2, 2, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(ref, x, gy)
    got = _fast2x2(gy, w.flip(2, 3).transpose(0, 1))
    assert (got - gx).abs().max() <= 1e-12 * gx.abs().max()


@pytest.mark.parametrize("dgrad", [False, True])
def test_packed_u9_is_g_w_gt(dgrad):
    g = torch.Generator().manual_seed(7)
    w = torch.randn(24, 40, 3, 3, generator=g)
    u9 = fast2x2_weights(w, dgrad)
    _, G, _ = _mats()
    wd = w.double().flip(2, 3).transpose(0, 1) if dgrad else w.double()
    ref = torch.einsum("ia,kcad,jd->ijkc", G, wd, G).reshape(9, wd.shape[0], wd.shape[1])
    assert u9.dtype == torch.float32 and u9.is_contiguous() and u9.shape == ref.shape
    assert torch.equal(u9, ref.float())  # computed in fp64, rounded once
    # the centre tap alone is product 0; the corner taps only reach the last products
    assert torch.equal(u9[0], wd[:, :, 1, 1].float())


def test_nan_reaches_every_output_like_the_dense_form():
    """Every input pixel reaches every output pixel of a 2x2 map, in the dense form and (through
    V[0][0], the sum of the four pixels, which feeds all four outputs) in this one."""
    x = torch.zeros(2, 4, 2, 2, dtype=torch.float64)
    x[1, 2, 0, 1] = float("nan")
    w = torch.randn(3, 4, 3, 3, dtype=torch.float64)
    got, ref = _fast2x2(x, w), F.conv2d(x, w, padding=1)
    assert torch.equal(got.isnan(), ref.isnan()) and got[1].isnan().all() and not got[0].isnan().any()
