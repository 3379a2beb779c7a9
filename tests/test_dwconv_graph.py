"""tf.nn.depthwise_conv2d, the glorot initializer and layers.SepConv_BN at
graph-construction time, and the host half of the C-ABI (no GPU): static
shapes, argument errors, seg_dwconv_desc_init's geometry against
tests/dwconv_ref.geometry and its refusals through ctypes.  Kernels:
tests/test_gpu_dwconv.py."""
import ctypes
import math

import numpy as np
import pytest

from semanticsegmentation_tensorflow_amd import _lib, layers, ops, variables
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import tf
from tests import dwconv_ref as D

EINVAL, ESHAPE, EALIGN = 1, 2, 3


def _filter(k, C, m=1, name="f"):
    return tf.get_variable(name, [k, k, C, m], initializer=tf.glorot_uniform_initializer())


# ------------------------------------------------------------------ graph
@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_static_shapes(case):
    N, H, W, C, R, S, stride, rate, padding = case
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, H, W, C])
    f = tf.get_variable("f", [R, S, C, 1])
    y = tf.nn.depthwise_conv2d(x, f, [1, stride, stride, 1], padding, rate=list(rate), name="dw")
    assert y.op.type == "DepthwiseConv2D" and y.op.name.endswith("dw")
    assert y.op.attrs == {"stride": stride, "rate": tuple(rate), "padding": padding}
    assert tuple(y.shape) == (None,) + D.out_shape((N, H, W, C), R, S, stride, rate, padding)[1:]


def test_stride_and_rate_forms_and_unknown_dims():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, None, 20, 8])
    f = _filter(3, 8)
    assert tuple(tf.nn.depthwise_conv2d(x, f, 2, "SAME").shape) == (None, None, 10, 8)           # int stride
    assert tuple(tf.nn.depthwise_conv2d(x, f, [1, 2, 2, 1], "VALID").shape) == (None, None, 9, 8)
    y = tf.nn.depthwise_conv2d(x, f, 1, "VALID", rate=3)                                         # int rate
    assert y.op.attrs["rate"] == (3, 3) and tuple(y.shape) == (None, None, 14, 8)
    y = tf.nn.depthwise_conv2d(x, f, [1, 1, 1, 1], "VALID", rate=[1, 4])
    assert y.op.attrs["rate"] == (1, 4) and tuple(y.shape) == (None, None, 12, 8)
    assert tf.nn.depthwise_conv2d(x, f, 1, "SAME", rate=None).op.attrs["rate"] == (1, 1)


def test_argument_errors():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 8, 8, 8])
    f = _filter(3, 8)
    with pytest.raises(NotImplementedError):
        tf.nn.depthwise_conv2d(x, f, [1, 1, 2, 1], "SAME")                  # anisotropic stride
    with pytest.raises(NotImplementedError):
        tf.nn.depthwise_conv2d(x, _filter(3, 8, 2, "f2"), 1, "SAME")        # channel multiplier 2
    with pytest.raises(ValueError):
        tf.nn.depthwise_conv2d(x, f, 2, "SAME", rate=2)                     # TF: rate > 1 needs stride 1
    with pytest.raises(ValueError):
        tf.nn.depthwise_conv2d(x, f, [1, 2, 2, 1], "SAME", rate=[1, 2])
    with pytest.raises(ValueError):
        tf.nn.depthwise_conv2d(x, f, 1, "FULL")
    with pytest.raises(ValueError):
        tf.nn.depthwise_conv2d(x, _filter(3, 16, 1, "f16"), 1, "SAME")      # depth mismatch


def test_glorot_uniform_limits_and_values():
    lim = G.glorot_uniform_initializer.limit
    assert lim([3, 3, 512, 1]) == math.sqrt(6.0 / (9 * 512 + 9))           # depthwise: fan_in k k C, fan_out k k
    assert lim([1, 1, 256, 19]) == math.sqrt(6.0 / (256 + 19))
    assert lim([3, 3, 64, 128]) == math.sqrt(6.0 / (9 * 64 + 9 * 128))
    assert lim([10]) == math.sqrt(6.0 / 20) and lim([4, 6]) == math.sqrt(6.0 / 10)
    G.reset_default_graph()
    v = _filter(3, 512, name="aspp1_filter")
    a = variables.init_value(v, seed=3)
    assert a.shape == (3, 3, 512, 1) and a.dtype == np.float32
    L = lim(v.shape)
    assert np.abs(a).max() <= L and np.abs(a).max() > 0.95 * L             # 4608 draws fill the range
    assert abs(float(a.mean())) < 0.05 * L and abs(float(a.std()) - L / math.sqrt(3)) < 0.05 * L
    assert np.array_equal(a, variables.init_value(v, seed=3)) and not np.array_equal(a, variables.init_value(v, seed=4))
    # get_variable's own default is what it was
    assert isinstance(tf.get_variable("plain", [2, 2]).initializer, G.random_normal_initializer)


def _op_types():
    return [op.type for op in G.get_default_graph().ops if op.type != "VariableV2"]


@pytest.mark.parametrize("depth_activation", [False, True])
def test_sepconv_bn_stride_1(depth_activation):
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 9, 11, 16])
    y = layers.SepConv_BN(x, 24, "blk", rate=2, depth_activation=depth_activation)
    assert tuple(y.shape) == (None, 9, 11, 24)
    mid = ["DepthwiseConv2D", "FusedBatchNorm"]
    want = ["Placeholder"] + (mid + ["Relu"] if depth_activation else ["Relu"] + mid) + ["Conv2D", "FusedBatchNorm",
                                                                                        "Relu"]
    assert _op_types() == want
    dw = next(op for op in G.get_default_graph().ops if op.type == "DepthwiseConv2D")
    assert dw.attrs == {"stride": 1, "rate": (2, 2), "padding": "SAME"} and dw.name.endswith("blk_depthwise")
    names = [v.var_name for v in tf.global_variables()]
    assert names == ["blk_filter", "batch_normalization/gamma", "batch_normalization/beta",
                     "batch_normalization/moving_mean", "batch_normalization/moving_variance",
                     "blk_pointwise_BN/weights", "batch_normalization_1/gamma", "batch_normalization_1/beta",
                     "batch_normalization_1/moving_mean", "batch_normalization_1/moving_variance"]
    g = G.get_default_graph().variables
    assert tuple(g["blk_filter"].shape) == (3, 3, 16, 1)
    assert isinstance(g["blk_filter"].initializer, G.glorot_uniform_initializer)
    assert tuple(g["blk_pointwise_BN/weights"].shape) == (1, 1, 16, 24)


@pytest.mark.parametrize("depth_activation", [False, True])
@pytest.mark.parametrize("k,rate,pads,hw", [(3, 1, (1, 1), (5, 6)), (4, 1, (1, 2), (5, 6)), (3, 2, (2, 2), (5, 6))])
def test_sepconv_bn_stride_2_pads_the_effective_kernel(depth_activation, k, rate, pads, hw):
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 9, 11, 16])
    if rate > 1:
        # the explicit padding is built first, then TF's rule refuses rate > 1 with stride 2
        with pytest.raises(ValueError):
            layers.SepConv_BN(x, 24, "blk", stride=2, kernel_size=k, rate=rate, depth_activation=depth_activation)
        pad = next(op for op in G.get_default_graph().ops if op.type == "Pad")
        assert pad.attrs["pads"] == pads + pads
        return
    y = layers.SepConv_BN(x, 24, "blk", stride=2, kernel_size=k, rate=rate, depth_activation=depth_activation)
    assert tuple(y.shape) == (None,) + hw + (24,)
    mid = ["DepthwiseConv2D", "FusedBatchNorm"]
    want = ["Placeholder", "Pad"] + (mid + ["Relu"] if depth_activation else ["Relu"] + mid) + [
        "Conv2D", "FusedBatchNorm", "Relu"]
    assert _op_types() == want
    ops_ = {op.type: op for op in G.get_default_graph().ops}
    assert ops_["Pad"].attrs["pads"] == pads + pads and ops_["Pad"].name.endswith("blkzero_paddings")
    assert ops_["DepthwiseConv2D"].attrs == {"stride": 2, "rate": (1, 1), "padding": "VALID"}


# ------------------------------------------------------------------ C-ABI, host half
def _init(N, H, W, C, cv, R, S, stride, dh, dw, padding, dtype=ops.BF16):
    d = _lib.SegDwconvDesc()
    for f, _ in d._fields_:
        setattr(d, f, -7)
    st = _lib.load().seg_dwconv_desc_init(ctypes.byref(d), N, H, W, C, cv, R, S, stride, dh, dw,
                                          0 if padding == "SAME" else 1, dtype)
    return st, d


def test_dwconv_desc_known_answers():
    st, d = _init(1, 8, 20, 8, 3, 3, 3, 1, 1, 18, "SAME")
    assert st == 0
    assert (d.OH, d.pad_top) == (8, 1) and (d.OW, d.pad_left) == (20, 18)       # rate 18 on 20 columns
    assert (d.N, d.H, d.W, d.C, d.c_valid, d.R, d.S, d.stride, d.dil_h, d.dil_w) == (1, 8, 20, 8, 3, 3, 3, 1, 1, 18)
    assert (d.ldx, d.ldy, d.dtype) == (8, 8, ops.BF16)
    for dtype in (ops.F32, ops.BF16, ops.F16):
        for (N, H, W, C, R, S, stride, rate, padding) in D.CASES:
            st, d = _init(N, H, W, C, C, R, S, stride, rate[0], rate[1], padding, dtype)
            gh, gw = D.geometry(H, R, stride, rate[0], padding), D.geometry(W, S, stride, rate[1], padding)
            assert st == 0 and (d.OH, d.OW, d.pad_top, d.pad_left) == (gh[0], gw[0], gh[1], gw[1])
    # the model's launches at 1x160x576: rates 6 / 12 / 18 on the 20x72 map, rate 1 on 40x144
    for r in (6, 12, 18):
        d = ops.dwconv_desc(1, 20, 72, 512, 512, 3, 3, 1, r, "SAME")
        assert (d.OH, d.OW, d.pad_top, d.pad_left) == (20, 72, r, r)
    d = ops.dwconv_desc(1, 40, 144, 256, 256, 3, 3, 1, 1, "SAME")
    assert (d.OH, d.OW, d.pad_top, d.pad_left) == (40, 144, 1, 1)
    # the filter-gradient workspace: whole fp32 partial rows [R S][C]
    ws = ops.dwconv_bwd_filter_workspace(d)
    assert ws > 0 and ws % (9 * 256 * 4) == 0


def test_dwconv_desc_refusals_leave_the_descriptor_alone():
    bad = [((0, 8, 8, 8, 8, 3, 3, 1, 1, 1, "SAME"), EINVAL), ((1, 8, -1, 8, 8, 3, 3, 1, 1, 1, "SAME"), EINVAL),
           ((1, 8, 8, 8, 8, 0, 3, 1, 1, 1, "SAME"), EINVAL), ((1, 8, 8, 8, 8, 3, 3, 0, 1, 1, "SAME"), EINVAL),
           ((1, 8, 8, 8, 8, 3, 3, 1, 0, 1, "SAME"), EINVAL), ((1, 8, 8, 8, 0, 3, 3, 1, 1, 1, "SAME"), EINVAL),
           ((1, 8, 8, 8, 8, 8, 3, 1, 1, 1, "SAME"), EINVAL),           # R > 7
           ((1, 8, 8, 8, 8, 3, 9, 1, 1, 1, "SAME"), EINVAL),
           ((1, 8, 8, 8, 8, 3, 3, 2, 2, 1, "SAME"), ESHAPE),           # stride 2 with rate 2: TF's rule
           ((1, 8, 8, 8, 8, 3, 3, 2, 1, 3, "SAME"), ESHAPE),
           ((1, 4, 8, 8, 8, 3, 3, 1, 2, 2, "VALID"), ESHAPE),          # effective window 5 on 4 rows: no output
           ((1, 8, 8, 12, 12, 3, 3, 1, 1, 1, "SAME"), EALIGN),         # C % 8
           ((1, 8, 8, 8, 9, 3, 3, 1, 1, 1, "SAME"), EALIGN),           # more real channels than padded ones
           ((1 << 15, 1 << 8, 1 << 8, 8, 8, 3, 3, 1, 1, 1, "SAME"), EINVAL)]     # 2^34 elements
    for args, code in bad:
        st, d = _init(*args)
        assert st == code, (args, st)
        assert all(getattr(d, f) == -7 for f, _ in d._fields_), args
    assert _init(1, 8, 8, 12, 12, 3, 3, 1, 1, 1, "SAME", ops.F32)[0] == EALIGN      # C % 8 in fp32 too
    assert _init(1, 8, 8, 8, 8, 7, 7, 1, 1, 1, "SAME")[0] == 0                      # 7 x 7 is the limit
    assert _init(1, 8, 8, 8, 8, 3, 3, 1, 1, 1, "SAME", 9)[0] == EINVAL              # unknown dtype
    lib = _lib.load()
    assert lib.seg_dwconv_desc_init(None, 1, 8, 8, 8, 8, 3, 3, 1, 1, 1, 0, ops.BF16) == EINVAL
    d = _lib.SegDwconvDesc()
    assert lib.seg_dwconv_desc_init(ctypes.byref(d), 1, 8, 8, 8, 8, 3, 3, 1, 1, 1, 2, ops.BF16) == EINVAL   # padding 2
    with pytest.raises(ValueError):
        ops.dwconv_desc(1, 8, 8, 8, 8, 3, 3, 2, 2)
    # a refused descriptor needs no workspace
    st, d = _init(1, 8, 8, 8, 8, 3, 3, 1, 1, 1, "SAME")
    d.R = 9
    assert lib.seg_dwconv_bwd_filter_workspace(ctypes.byref(d)) == 0
