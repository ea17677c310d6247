"""(CPU) The float64 PyTorch bodies of ops.bn_silu_fwd / bn_silu_bwd (the oracle of test_bn_silu_gpu.py)
against autograd through F.batch_norm(training=True) + F.silu, on the cases of tests/test_bn_hswish.py.
SiLU has no kink: no element is excluded."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_bn_hswish import CASES, EPS, IDS, MOM, inputs, nhwc
from torchpruner_amd import ops


def saturated(gamma, beta):
    """Pre-activations of +100 and -100 (to within 1e-2) in channels 1 and 2: the sigmoid is 1 and 0."""
    gamma, beta = gamma.clone(), beta.clone()
    gamma[1:3] = 1e-3
    beta[1], beta[2] = 100.0, -100.0
    return gamma, beta


@functools.lru_cache(maxsize=None)
def reference(shape, C, saturate=False):
    """float64 autograd: NHWC y, dx and dgamma, dbeta, running statistics; shared, never modified."""
    x, gamma, beta, g = (t.double() for t in inputs(shape, C))
    if saturate:
        gamma, beta = saturated(gamma, beta)
    leaves = [t.requires_grad_(True) for t in (x, gamma, beta)]
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y = F.silu(F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS))
    dx, dgamma, dbeta = torch.autograd.grad((y * g).sum(), leaves)
    return dict(y=nhwc(y.detach(), C), dx=nhwc(dx, C), dgamma=dgamma, dbeta=dbeta, rm=rm, rv=rv)


@pytest.mark.parametrize("carried", [False, True], ids=["module_width", "carried"])
@pytest.mark.parametrize("shape,C", CASES, ids=IDS)
def test_torch_bodies_match_autograd(shape, C, carried):
    from torchpruner_amd.engine.train import _act_w
    ref = reference(shape, C)
    x, gamma, beta, g = (t.double() for t in inputs(shape, C))
    Cp = _act_w(C) if carried else C
    xh, gh = nhwc(x, Cp), nhwc(g, Cp, fill=1.0)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y, mean, invstd, ab = ops.bn_silu_fwd(xh, gamma, beta, rm, rv, EPS, MOM, None, C)
    dx, dgamma, dbeta = ops.bn_silu_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    for got, want in ((y[..., :C], ref["y"]), (rm, ref["rm"]), (rv, ref["rv"]), (dx[..., :C], ref["dx"]),
                      (dgamma, ref["dgamma"]), (dbeta, ref["dbeta"])):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-11)
    assert (y[..., C:] == 0).all() and (ab[:, C:] == 0).all() and (dx[..., C:] == 0).all()
    assert ops.bn_silu_bwd(gh, xh, gamma, mean, invstd, ab, False, C)[0] is None
