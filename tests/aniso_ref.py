"""float64 CPU reference of tf.nn.conv2d with per-axis dilation
(dilations=[1, dh, dw, 1], Network/model/LidCamNet.py:45-53): oracle.tf1_ops
takes one dilation, so this states the per-axis form from the oracle's own
padding rule (T.conv_pads, per axis) and torch's conv2d with a dilation tuple.
Differentiable (autograd gives Conv2DBackpropInput / Conv2DBackpropFilter).
Pinned on the CPU by tests/test_conv_desc2.py."""
import torch
import torch.nn.functional as F

from oracle import tf1_ops as T


def conv2d(x, w, stride=1, padding="SAME", dilation=(1, 1)):
    """x [N,H,W,C], w [R,S,C,K] (HWIO), float64 -> [N,OH,OW,K]."""
    dh, dw = dilation
    N, H, W, C = x.shape
    R, S, _, K = w.shape
    oh, pt, pb = T.conv_pads(H, R, stride, dh, padding)
    ow, pl, pr = T.conv_pads(W, S, stride, dw, padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.permute(3, 2, 0, 1), stride=stride, dilation=(dh, dw))
    assert y.shape[2:] == (oh, ow), (y.shape, oh, ow)
    return y.permute(0, 2, 3, 1)
