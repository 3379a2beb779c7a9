"""seg_conv_desc_init2 (stride and dilation per axis), ops.conv_desc's (h, w)
pairs, tf.nn.conv2d's per-axis dilations argument, and the CPU pins of the
per-axis reference tests/aniso_ref.py.  No GPU."""
import ctypes
import itertools

import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import _lib, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import tf
from tests import aniso_ref

FIELDS = [n for n, _ in _lib.SegConvDesc._fields_]


def _bytes(d):
    return bytes(memoryview(d).cast("B"))


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
def test_init2_applies_the_padding_rule_per_axis(padding):
    lib = _lib.load()
    pad = 0 if padding == "SAME" else 1
    n = 0
    for H, W in [(20, 72), (21, 71), (9, 14), (160, 576), (97, 130)]:
        for R in (1, 3, 4):
            for (sh, sw), (dh, dw) in itertools.product(itertools.product((1, 2), repeat=2),
                                                        itertools.product((1, 2, 3, 16, 32), repeat=2)):
                oh, pt, pb = T.conv_pads(H, R, sh, dh, padding)
                ow, pl, pr = T.conv_pads(W, R, sw, dw, padding)
                d = _lib.SegConvDesc()
                st = lib.seg_conv_desc_init2(ctypes.byref(d), 2, H, W, 12, 24, R, R, sh, sw, dh, dw, pad, ops.BF16)
                if oh <= 0 or ow <= 0:
                    assert st != 0, (H, W, R, sh, sw, dh, dw)
                    continue
                assert st == 0, (H, W, R, sh, sw, dh, dw)
                assert (d.OH, d.pad_top, d.pad_bottom) == (oh, pt, pb), (H, R, sh, dh)
                assert (d.OW, d.pad_left, d.pad_right) == (ow, pl, pr), (W, R, sw, dw)
                assert (d.stride_h, d.stride_w, d.dil_h, d.dil_w) == (sh, sw, dh, dw)
                assert (d.C, d.K, d.c_valid, d.k_valid, d.ldx, d.ldy) == (16, 24, 12, 24, 16, 24)
                n += 1
    assert n > 1000


def test_init_is_init2_with_equal_axes_byte_for_byte():
    lib = _lib.load()
    for H, W, C, K, R, s, dil, pad, dt in [(20, 72, 128, 128, 3, 1, 2, 0, ops.BF16), (21, 71, 3, 64, 4, 2, 1, 0, ops.F16),
                                           (33, 17, 12, 24, 3, 2, 3, 1, ops.F32), (9, 9, 8, 8, 1, 1, 1, 1, ops.BF16),
                                           (160, 576, 4, 32, 4, 2, 1, 0, ops.BF16)]:
        a, b = _lib.SegConvDesc(), _lib.SegConvDesc()
        ctypes.memset(ctypes.byref(a), 0x5A, ctypes.sizeof(a))
        ctypes.memset(ctypes.byref(b), 0xA5, ctypes.sizeof(b))
        assert lib.seg_conv_desc_init(ctypes.byref(a), 2, H, W, C, K, R, R, s, dil, pad, dt) == 0
        assert lib.seg_conv_desc_init2(ctypes.byref(b), 2, H, W, C, K, R, R, s, s, dil, dil, pad, dt) == 0
        assert _bytes(a) == _bytes(b), {f: (getattr(a, f), getattr(b, f)) for f in FIELDS}
    d = _lib.SegConvDesc()
    for bad in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)]:
        assert lib.seg_conv_desc_init2(ctypes.byref(d), 1, 8, 8, 8, 8, 3, 3, *bad, 0, ops.BF16) != 0
    # VALID with a dilated filter wider than the map: TF's shape error
    assert lib.seg_conv_desc_init2(ctypes.byref(d), 1, 20, 40, 8, 8, 3, 3, 1, 1, 2, 32, 1, ops.BF16) != 0


def test_ops_conv_desc_takes_ints_or_pairs():
    a = ops.conv_desc(2, 20, 72, 128, 128, 3, 3, 1, 2, "SAME", ops.BF16)
    b = ops.conv_desc(2, 20, 72, 128, 128, 3, 3, (1, 1), (2, 2), "SAME", ops.BF16)
    assert _bytes(a) == _bytes(b)
    c = ops.conv_desc(2, 20, 72, 128, 128, 3, 3, 1, (16, 32), "SAME", ops.BF16)
    assert (c.dil_h, c.dil_w, c.OH, c.OW) == (16, 32, 20, 72)
    assert (c.pad_top, c.pad_bottom, c.pad_left, c.pad_right) == (16, 16, 32, 32)
    e = ops.conv_desc(1, 11, 13, 16, 32, 4, 4, (2, 2), 1, "SAME", ops.F16)
    assert (e.stride_h, e.stride_w, e.OH, e.OW, e.pad_top, e.pad_bottom) == (2, 2, 6, 7, 1, 2)


def _conv(dilations, strides=(1, 1, 1, 1), padding="SAME"):
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 20, 72, 8])
    w = tf.get_variable("w", shape=[3, 3, 8, 16], initializer=tf.constant_initializer(0.0))
    return tf.nn.conv2d(x, w, strides=list(strides), padding=padding, dilations=dilations)


def test_graph_conv2d_dilation_argument_rules():
    y = _conv([1, 1, 2, 1])
    assert y.op.attrs["dilation_hw"] == (1, 2)
    assert tuple(y.shape[1:]) == (20, 72, 16)
    assert _conv([2, 4]).op.attrs["dilation_hw"] == (2, 4)
    # isotropic convs keep the int attrs they always had
    for arg in (2, [2, 2], [1, 2, 2, 1]):
        at = _conv(arg).op.attrs
        assert at["dilation"] == 2 and isinstance(at["dilation"], int) and at["dilation_hw"] == (2, 2)
        assert at["stride"] == 1 and isinstance(at["stride"], int)
    # VALID shape rule per axis
    assert tuple(_conv([1, 2, 3, 1], padding="VALID").shape[1:3]) == (20 - 4, 72 - 6)
    # TF: the batch and depth entries must be 1
    for bad in ([2, 1, 1, 1], [1, 1, 1, 2]):
        with pytest.raises(ValueError):
            _conv(bad)
    with pytest.raises(NotImplementedError):
        _conv([1, 1, 2, 1], strides=(1, 2, 2, 1))
    with pytest.raises(NotImplementedError):
        _conv(2, strides=(1, 2, 2, 1))


def test_dilations_1_1_2_1_reaches_the_descriptor_as_dil_h_1_dil_w_2():
    y = _conv([1, 1, 2, 1])
    d = ops.conv_desc(2, 20, 72, 8, 16, 3, 3, y.op.attrs["stride"], y.op.attrs["dilation_hw"], "SAME", ops.BF16)
    assert (d.dil_h, d.dil_w) == (1, 2)
    assert (d.pad_top, d.pad_bottom, d.pad_left, d.pad_right) == (1, 1, 2, 2)


# ---- the per-axis reference itself ------------------------------------------
@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("stride,dil", [(1, 1), (1, 2), (1, 3), (2, 1)])
def test_aniso_ref_equals_the_oracle_when_the_axes_agree(stride, dil, padding):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 11, 14, 5, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, 5, 7, generator=g, dtype=torch.float64)
    got = aniso_ref.conv2d(x, w, stride, padding, (dil, dil))
    assert torch.equal(got, T.conv2d(x, w, stride, padding, dil))


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("dil", [(1, 2), (2, 3), (3, 1), (4, 8)])
def test_aniso_ref_commutes_with_the_hw_transpose(dil, padding):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 19, 23, 5, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, 5, 7, generator=g, dtype=torch.float64)
    a = aniso_ref.conv2d(x, w, 1, padding, dil)
    b = aniso_ref.conv2d(x.transpose(1, 2), w.transpose(0, 1), 1, padding, dil[::-1]).transpose(1, 2)
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= 1e-12 * a.abs().max().item()
