"""float64 restatements of the MBConvBlock operations of csrc/mbconv.hip
(Network/model/EfficientNet.py:153-210) and their gradients, written out as
formulae -- no autograd; tests/test_mbconv_ref.py pins them to torch's.

Tensors are float64 torch tensors, NHWC (or [P, C]); gamma / beta are [C] or
None (the plain activation)."""
import math

import torch

ACTS = ("swish", "sigmoid")


def sigmoid(z):
    """1 / (1 + exp(-z)) evaluated on the side that cannot overflow."""
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def affine(x, gamma, beta, eps):
    """(z, scale): z = x * gamma / sqrt(1 + eps) + beta, or z = x."""
    if gamma is None:
        return x, torch.ones(x.shape[-1], dtype=torch.float64)
    scale = gamma / math.sqrt(1.0 + eps)
    return x * scale + beta, scale


def bn_act_fwd(x, gamma, beta, eps, act):
    z, _ = affine(x, gamma, beta, eps)
    s = sigmoid(z)
    return z * s if act == "swish" else s


def act_grad(z, act):
    """d act(z) / dz."""
    s = sigmoid(z)
    return s * (1.0 + z * (1.0 - s)) if act == "swish" else s * (1.0 - s)


def bn_act_bwd(x, dy, gamma, beta, eps, act):
    """(dx, dgamma, dbeta); the last two None without an affine."""
    z, scale = affine(x, gamma, beta, eps)
    dz = dy * act_grad(z, act)
    dx = dz * scale
    if gamma is None:
        return dx, None, None
    red = tuple(range(x.dim() - 1))
    return dx, (dz * x).sum(red) / math.sqrt(1.0 + eps), dz.sum(red)


def se_squeeze(x, scale):
    """[N, H, W, C] -> [N, C]."""
    return x.sum((1, 2)) * scale


def se_excite_fwd(x, s):
    """x [N, H, W, C] times s [N, C]."""
    return x * s[:, None, None, :]


def se_excite_bwd(x, s, dy):
    """(dx, ds)."""
    return dy * s[:, None, None, :], (dy * x).sum((1, 2))
