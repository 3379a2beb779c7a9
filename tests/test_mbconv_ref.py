"""tests/mbconv_ref.py (the float64 restatement the GPU kernels of
csrc/mbconv.hip are compared against) pinned to torch autograd at 1e-12."""
import math

import pytest
import torch

from tests import mbconv_ref as R

TOL = 1e-12


def _close(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


def _torch_act(z, act):
    return z * torch.sigmoid(z) if act == "swish" else torch.sigmoid(z)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("act", R.ACTS)
def test_bn_act_matches_autograd(act, affine):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 5, 3, 6, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dy = torch.randn(2, 5, 3, 6, generator=g, dtype=torch.float64)
    eps = 1e-3
    gamma = beta = None
    if affine:
        gamma = (torch.randn(6, generator=g, dtype=torch.float64) + 1).requires_grad_(True)
        beta = torch.randn(6, generator=g, dtype=torch.float64).requires_grad_(True)
    z = x * gamma / math.sqrt(1 + eps) + beta if affine else x
    y = _torch_act(z, act)
    y.backward(dy)
    _close(R.bn_act_fwd(x.detach(), None if gamma is None else gamma.detach(),
                        None if beta is None else beta.detach(), eps, act), y.detach(), "y")
    dx, dgamma, dbeta = R.bn_act_bwd(x.detach(), dy, None if gamma is None else gamma.detach(),
                                     None if beta is None else beta.detach(), eps, act)
    _close(dx, x.grad, "dx")
    if affine:
        _close(dgamma, gamma.grad, "dgamma")
        _close(dbeta, beta.grad, "dbeta")
    else:
        assert dgamma is None and dbeta is None


@pytest.mark.parametrize("act", R.ACTS)
def test_large_arguments_stay_finite(act):
    z = torch.tensor([-800.0, -100.0, -20.0, 0.0, 20.0, 100.0, 800.0], dtype=torch.float64)
    y = R.bn_act_fwd(z, None, None, 0.0, act)
    dx, _, _ = R.bn_act_bwd(z, torch.ones_like(z), None, None, 0.0, act)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    _close(y, _torch_act(z, act), "y")
    assert y[3].item() == (0.0 if act == "swish" else 0.5)
    assert dx[3].item() == (0.5 if act == "swish" else 0.25)
    # the tails: sigmoid -> 0 / 1, swish -> 0 / z, their slopes -> 0 / (0 or 1)
    assert y[0].item() == 0.0 and y[-1].item() == (800.0 if act == "swish" else 1.0)
    assert dx[0].item() == 0.0 and dx[-1].item() == (1.0 if act == "swish" else 0.0)


def test_squeeze_and_excite_match_autograd():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    s = torch.rand(2, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64)
    y = x * s.reshape(2, 1, 1, 6)
    y.backward(dy)
    _close(R.se_excite_fwd(x.detach(), s.detach()), y.detach(), "y")
    dx, ds = R.se_excite_bwd(x.detach(), s.detach(), dy)
    _close(dx, x.grad, "dx")
    _close(ds, s.grad, "ds")
    _close(R.se_squeeze(x.detach(), 1.0 / 20), x.detach().mean((1, 2)), "squeeze")


def test_a_whole_squeeze_excite_block_matches_autograd():
    """pool -> reduce + swish -> expand + sigmoid -> multiply: the gradient of x
    is the sum of the multiply's and the pool's shares."""
    g = torch.Generator().manual_seed(9)
    N, H, W, C, Cr = 2, 3, 4, 8, 2
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64).requires_grad_(True)
    w1 = torch.randn(C, Cr, generator=g, dtype=torch.float64)
    w2 = torch.randn(Cr, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    m = x.mean((1, 2))
    r = m @ w1
    a = r * torch.sigmoid(r)
    e = a @ w2
    s = torch.sigmoid(e)
    (x * s.reshape(N, 1, 1, C)).backward(dy)

    xd = x.detach()
    m_ = R.se_squeeze(xd, 1.0 / (H * W))
    r_ = m_ @ w1
    e_ = R.bn_act_fwd(r_, None, None, 0.0, "swish") @ w2
    s_ = R.bn_act_fwd(e_, None, None, 0.0, "sigmoid")
    dx, ds = R.se_excite_bwd(xd, s_, dy)
    de, _, _ = R.bn_act_bwd(e_, ds, None, None, 0.0, "sigmoid")
    dr, _, _ = R.bn_act_bwd(r_, de @ w2.T, None, None, 0.0, "swish")
    dm = dr @ w1.T
    dx = dx + dm[:, None, None, :] / (H * W)
    _close(dx, x.grad, "dx")
