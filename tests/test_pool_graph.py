"""General pooling and tf.pad at graph-construction time and in the host half of
the C-ABI (no GPU): shape inference of tf.nn.max_pool / avg_pool for any
window, stride and padding, tf.pad on H and W, layers.Zero_Padding, the 2x2
stride-2 VALID pool unchanged, and seg_pool_desc_init's geometry and refusals
through ctypes.  Kernels: tests/test_gpu_pool2d.py."""
import ctypes

import pytest

from semanticsegmentation_tensorflow_amd import _lib, layers, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import tf
from tests import pool_ref

# (N, H, W, C, kh, kw, sh, sw, padding): the kernel cases of tests/test_gpu_pool2d.py
CASES = [(2, 9, 11, 16, 3, 3, 2, 2, "VALID"), (1, 8, 8, 8, 3, 3, 2, 2, "SAME"), (2, 5, 18, 24, 5, 18, 5, 18, "VALID"),
         (1, 5, 18, 8, 3, 9, 3, 9, "VALID"), (1, 5, 18, 8, 2, 6, 2, 6, "VALID"), (1, 5, 18, 8, 1, 3, 1, 3, "VALID"),
         (2, 7, 9, 8, 1, 1, 2, 2, "VALID"), (1, 7, 7, 8, 2, 2, 3, 3, "VALID"), (1, 6, 6, 40, 2, 2, 2, 2, "VALID")]
# their output sizes, by hand: VALID (in - k) // s + 1, SAME ceil(in / s)
OUT = [(4, 5), (4, 4), (1, 1), (1, 2), (2, 3), (5, 6), (4, 5), (2, 2), (3, 3)]


@pytest.mark.parametrize("case,out", list(zip(CASES, OUT)))
@pytest.mark.parametrize("pool", [tf.nn.max_pool, tf.nn.avg_pool])
def test_pool_shape_inference(pool, case, out):
    N, H, W, C, kh, kw, sh, sw, padding = case
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, H, W, C])
    y = pool(x, ksize=[1, kh, kw, 1], strides=[1, sh, sw, 1], padding=padding, name="p")
    assert tuple(y.shape) == (None,) + out + (C,)
    assert out == pool_ref.out_shape((N, H, W, C), (kh, kw), (sh, sw), padding)[1:3]
    if (kh, kw, sh, sw, padding) != (2, 2, 2, 2, "VALID"):
        assert y.op.type == "Pool2D"
        assert y.op.attrs == {"kind": "max" if pool is tf.nn.max_pool else "avg", "ksize": (kh, kw),
                              "strides": (sh, sw), "padding": padding}


def test_pspnet_pool_shapes():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 82, 290, 64])
    assert tuple(layers.Max_Pooling(x, filter_height=3, filter_width=3, stride=2, name="pool1").shape) == \
        (None, 40, 144, 64)
    e = tf.placeholder(tf.float32, [None, 5, 18, 512])
    got = [tuple(layers.Avg_Pooling(e, filter_height=kh, filter_width=kw, stride_height=kh, stride_width=kw,
                                    name="p").shape[1:3]) for kh, kw in ((5, 18), (3, 9), (2, 6), (1, 3))]
    assert got == [(1, 1), (1, 2), (2, 3), (5, 6)]
    assert tuple(layers.Max_Pooling(e, "m", filter_height=3, filter_width=3, stride=2, padding="SAME").shape) == \
        (None, 3, 9, 512)


def test_2x2_stride2_valid_pool_is_the_op_it_was():
    """Type and attrs as before this op set grew: the fused-pool, switch-byte
    and unpool plans key on them."""
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 9, 10, 8])
    for fn, kind in ((tf.nn.max_pool, "MaxPool"), (tf.nn.avg_pool, "AvgPool")):
        for ks, st in (([1, 2, 2, 1], [1, 2, 2, 1]), ((2, 2), (2, 2)), (2, 2)):
            y = fn(x, ksize=ks, strides=st, padding="VALID", name="pool")
            assert y.op.type == kind and y.op.attrs == {} and len(y.op.inputs) == 1 and y.op.inputs[0] is x
            assert tuple(y.shape) == (None, 4, 5, 8)
    y = layers.max_pool(x, "pool1")
    assert y.op.type == "MaxPool" and y.op.attrs == {}
    assert layers.Avg_Pooling(x, "ap").op.type == "AvgPool"
    # the same window under SAME is not that op
    assert tf.nn.max_pool(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME").op.type == "Pool2D"


def test_pool_argument_errors():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 8, 8, 8])
    with pytest.raises(ValueError):
        tf.nn.max_pool(x, [1, 0, 3, 1], [1, 2, 2, 1], "VALID")
    with pytest.raises(ValueError):
        tf.nn.avg_pool(x, [1, 3, 3, 1], [1, 0, 2, 1], "VALID")
    with pytest.raises(ValueError):
        tf.nn.avg_pool(x, [1, 3, 3, 1], [1, 2, 2, 1], "FULL")


def test_tf_pad_on_h_and_w():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 5, 7, 16])
    y = tf.pad(x, paddings=[[0, 0], [0, 2], [1, 0], [0, 0]], name="padded")
    assert y.op.type == "Pad" and y.op.attrs == {"pads": (0, 2, 1, 0)} and tuple(y.shape) == (None, 7, 8, 16)
    import numpy as np
    y = tf.pad(x, paddings=np.array([[0, 0], [3, 3], [3, 3], [0, 0]]))
    assert tuple(y.shape) == (None, 11, 13, 16)
    for bad in ([[1, 0], [0, 0], [0, 0], [0, 0]], [[0, 0], [1, 1], [1, 1], [0, 1]]):
        with pytest.raises(ValueError):
            tf.pad(x, paddings=bad)
    with pytest.raises(ValueError):
        tf.pad(x, paddings=[[0, 0], [-1, 0], [0, 0], [0, 0]])
    with pytest.raises(NotImplementedError):
        tf.pad(x, paddings=[[0, 0], [1, 1], [1, 1], [0, 0]], mode="REFLECT")


def test_zero_padding_layer():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 160, 576, 4])
    y = layers.Zero_Padding(x, paddings=3, name="conv1")
    assert y.op.type == "Pad" and y.op.attrs["pads"] == (3, 3, 3, 3) and tuple(y.shape) == (None, 166, 582, 4)
    assert tuple(layers.Zero_Padding(y, 1, "conv1").shape) == (None, 168, 584, 4)
    assert not tf.global_variables()                     # the scope name is reused by conv1: no variable of its own


def test_conv2d_reads_dilation_true_as_one():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 16, 24, 4])
    y = layers.Conv2D_Block(x, 64, 7, 7, 2, "VALID", True, True, name="conv1")      # PSPNet.py:31's binding
    conv = next(op for op in G.get_default_graph().ops if op.type == "Conv2D")
    assert conv.attrs["dilation"] == 1 and conv.attrs["dilation_hw"] == (1, 1) and conv.attrs["stride"] == 2
    assert y.op.type == "FusedBatchNorm" and tuple(y.shape) == (None, 5, 9, 64)      # BN bound, no ReLU


# ------------------------------------------------------------------ C-ABI, host half
def _init(N, H, W, C, kh, kw, sh, sw, padding, kind=0, dtype=ops.BF16):
    d = _lib.SegPoolDesc()
    for f, _ in d._fields_:
        setattr(d, f, -7)
    st = _lib.load().seg_pool_desc_init(ctypes.byref(d), N, H, W, C, kh, kw, sh, sw, 0 if padding == "SAME" else 1,
                                        kind, dtype)
    return st, d


def test_pool_desc_known_answers():
    st, d = _init(1, 5, 4, 8, 3, 3, 2, 2, "SAME")
    assert st == 0
    assert (d.OH, d.pad_top) == (3, 1)                   # in 5: out 3, pads 1 / 1
    assert (d.OW, d.pad_left) == (2, 0)                  # in 4: out 2, pads 0 / 1
    assert (d.ldx, d.ldy, d.kind, d.dtype, d.N, d.H, d.W, d.C) == (8, 8, 0, ops.BF16, 1, 5, 4, 8)
    assert (d.kh, d.kw, d.sh, d.sw) == (3, 3, 2, 2)
    for (N, H, W, C, kh, kw, sh, sw, padding), out in zip(CASES, OUT):
        for kind in (0, 1):
            st, d = _init(N, H, W, C, kh, kw, sh, sw, padding, kind)
            assert st == 0 and (d.OH, d.OW) == out
            g = (pool_ref.geometry(H, kh, sh, padding), pool_ref.geometry(W, kw, sw, padding))
            assert (d.pad_top, d.pad_left) == (g[0][1], g[1][1])
    st, d = _init(1, 82, 290, 64, 3, 3, 2, 2, "VALID")
    assert st == 0 and (d.OH, d.OW) == (40, 144)
    st, d = _init(1, 80, 288, 256, 1, 1, 2, 2, "SAME", 1)
    assert st == 0 and (d.OH, d.OW, d.pad_top, d.pad_left) == (40, 144, 0, 0)
    assert ops.pool_desc(1, 5, 18, 512, (2, 6), (2, 6), "VALID", ops.POOL_AVG).OW == 3


def test_pool_desc_refusals_leave_the_descriptor_alone():
    EINVAL = 1
    bad = [(1, 17, 17, 8, 1, 257, 1, 1, "SAME"),         # area 257: the switch byte cannot hold the position
           (1, 20, 20, 8, 17, 16, 1, 1, "SAME"),         # 272
           (1, 8, 8, 8, 0, 3, 2, 2, "VALID"), (1, 8, 8, 8, 3, 3, 0, 2, "VALID"), (1, 8, 8, 8, 3, 3, 2, 0, "VALID"),
           (0, 8, 8, 8, 3, 3, 2, 2, "VALID"), (1, 8, 8, 0, 3, 3, 2, 2, "VALID"), (1, 8, -1, 8, 3, 3, 2, 2, "VALID"),
           (1, 8, 8, 12, 3, 3, 2, 2, "VALID"),           # 12 bf16 channels: one and a half chunks
           (1, 2, 8, 8, 3, 3, 2, 2, "VALID"),            # the window does not fit: no output
           (1 << 15, 1 << 8, 1 << 8, 8, 3, 3, 2, 2, "SAME")]   # 2^34 elements
    for args in bad:
        st, d = _init(*args)
        assert st == EINVAL, args
        assert all(getattr(d, f) == -7 for f, _ in d._fields_), args
    assert _init(1, 16, 16, 8, 16, 16, 1, 1, "SAME")[0] == 0            # area 256 is the limit
    assert _init(1, 8, 8, 12, 3, 3, 2, 2, "VALID", 0, ops.F32)[0] == 0  # 12 fp32 channels: three chunks
    assert _init(1, 8, 8, 8, 3, 3, 2, 2, "VALID", 2)[0] == EINVAL       # unknown kind
    with pytest.raises(ValueError):
        ops.pool_desc(1, 8, 8, 8, (0, 3), (2, 2))
