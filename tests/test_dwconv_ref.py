"""tests/dwconv_ref.py (the float64 reference of seg_dwconv2d_*) pinned on the
CPU: hand answers on a 3x3 map, and torch's grouped convolution with the TF
padding made explicit -- forward and both gradients, float64, over the case
list the GPU kernels are tested on."""
import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_ref as D


def test_geometry_known_answers():
    assert D.geometry(8, 3, 2, 1, "SAME") == (4, 0, 1)            # asymmetric: nothing before, one after
    assert D.geometry(20, 3, 1, 18, "SAME") == (20, 18, 18)       # rate 18 on a 20-row map
    assert D.geometry(6, 3, 1, 6, "SAME") == (6, 6, 6)
    assert D.geometry(7, 3, 1, 2, "VALID") == (3, 0, 0)
    assert D.geometry(6, 2, 2, 1, "SAME") == (3, 0, 0)
    assert D.geometry(10, 3, 3, 1, "SAME") == (4, 1, 1)
    assert D.geometry(9, 5, 1, 1, "SAME") == (9, 2, 2)


def test_hand_answers_on_a_3x3_map():
    x = torch.arange(1.0, 10.0, dtype=torch.float64).reshape(1, 3, 3, 1)      # 1 2 3 / 4 5 6 / 7 8 9
    w = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], dtype=torch.float64).reshape(3, 3, 1)
    y = D.forward(x, w, 1, (1, 1), "SAME")[0, :, :, 0]
    # centre: the full correlation; corner (0, 0): taps (1..2, 1..2) on pixels (0..1, 0..1)
    assert y[1, 1].item() == sum(i * i for i in range(1, 10))
    assert y[0, 0].item() == 5 * 1 + 6 * 2 + 8 * 4 + 9 * 5
    assert y[2, 2].item() == 1 * 5 + 2 * 6 + 4 * 8 + 5 * 9
    assert y[0, 2].item() == 4 * 2 + 5 * 3 + 7 * 5 + 8 * 6
    # VALID: one output, the full correlation; its gradients are the other operand
    assert D.forward(x, w, 1, (1, 1), "VALID").reshape(-1).tolist() == [285.0]
    dy = torch.full((1, 1, 1, 1), 2.0, dtype=torch.float64)
    assert torch.equal(D.input_grad(dy, w, (1, 3, 3, 1), 1, (1, 1), "VALID")[0, :, :, 0], 2 * w[:, :, 0])
    assert torch.equal(D.filter_grad(x, dy, 3, 3, 1, (1, 1), "VALID")[:, :, 0], 2 * x[0, :, :, 0])
    # rate 2 SAME on 3x3: only the centre tap and, for a corner, the opposite corner are in-image
    y2 = D.forward(x, w, 1, (2, 2), "SAME")[0, :, :, 0]
    assert y2[1, 1].item() == 5 * 5
    assert y2[0, 0].item() == 5 * 1 + 6 * 3 + 8 * 7 + 9 * 9
    # stride 2 SAME on 3x3: pad 1 / 1, outputs at pixels (0, 0), (0, 2), (2, 0), (2, 2)
    y3 = D.forward(x, w, 2, (1, 1), "SAME")[0, :, :, 0]
    assert y3.shape == (2, 2) and y3[0, 0].item() == y[0, 0].item() and y3[1, 1].item() == y[2, 2].item()
    # the input gradient of ones through stride 2: pixel (1, 1) is reached by all four outputs' corner taps
    dx3 = D.input_grad(torch.ones(1, 2, 2, 1, dtype=torch.float64), w, (1, 3, 3, 1), 2, (1, 1), "SAME")[0, :, :, 0]
    assert dx3[1, 1].item() == 9 + 7 + 3 + 1 and dx3[0, 0].item() == 5


def _torch_depthwise(x, w, stride, rate, padding):
    N, H, W, C = x.shape
    R, S, _ = w.shape
    _, pt, pb = D.geometry(H, R, stride, rate[0], padding)
    _, pl, pr = D.geometry(W, S, stride, rate[1], padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.permute(2, 0, 1).unsqueeze(1), stride=stride, dilation=rate, groups=C)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_against_torch_grouped_conv(case):
    N, H, W, C, R, S, stride, rate, padding = case
    g = torch.Generator().manual_seed(D.CASES.index(case))
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(R, S, C, generator=g, dtype=torch.float64, requires_grad=True)
    y_t = _torch_depthwise(x, w, stride, rate, padding)
    dy = torch.randn(y_t.shape, generator=g, dtype=torch.float64)
    dx_t, dw_t = torch.autograd.grad(y_t, (x, w), dy)
    y = D.forward(x.detach(), w.detach(), stride, rate, padding)
    assert y.shape == y_t.shape == D.out_shape(x.shape, R, S, stride, rate, padding)
    assert (y - y_t).abs().max().item() <= 1e-12
    assert (D.input_grad(dy, w.detach(), tuple(x.shape), stride, rate, padding) - dx_t).abs().max().item() <= 1e-12
    assert (D.filter_grad(x.detach(), dy, R, S, stride, rate, padding) - dw_t).abs().max().item() <= 1e-12
    # and the autograd wrapper returns the same three
    x2, w2 = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    y2 = D.depthwise_ad(x2, w2.unsqueeze(-1), stride, rate, padding)
    dx2, dw2 = torch.autograd.grad(y2, (x2, w2), dy)
    assert torch.equal(y2, y) and (dx2 - dx_t).abs().max().item() <= 1e-12
    assert (dw2 - dw_t).abs().max().item() <= 1e-12
