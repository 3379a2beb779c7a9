"""The reference's layer builders (L1 of SURVEY.md 1), same names, arguments
and semantics, building graph ops that the Session runs on MI355X kernels.

FCN helpers: Network/model/FCN.py:117-171.
Generic builders: Network/utils/utils.py:164-333.
"""
from __future__ import annotations

from . import tf

STDDEV = 1e-2


# ---------------------------------------------------------------------------
# Network/model/FCN.py:117-171
# ---------------------------------------------------------------------------
def conv_layer(x, num_filters, name, filter_height=3, filter_width=3, stride=1, padding="SAME"):
    """relu(conv2d(x, W, SAME) + b), W ~ N(0, 0.01), b = 0 (FCN.py:117-136)."""
    input_channels = int(x.get_shape()[-1].value)
    with tf.variable_scope(name, reuse=tf.AUTO_REUSE):
        W = tf.get_variable("weights", shape=[filter_height, filter_width, input_channels, num_filters],
                            initializer=tf.random_normal_initializer(mean=0.0, stddev=STDDEV))
        b = tf.get_variable("biases", shape=[num_filters], initializer=tf.constant_initializer(0.0))
        conv = tf.nn.conv2d(x, W, strides=[1, stride, stride, 1], padding=padding)
        z = tf.nn.bias_add(conv, b)
        return tf.nn.relu(z)


def deconv_layer(x, shape, num_filters, name, output_shape, filter_height=4, filter_width=4, stride=2,
                 padding="SAME"):
    """conv2d_transpose(x, W[kh,kw,shape[3],num_filters]) + b (FCN.py:138-159).
    Note: `num_filters` is the INPUT depth, output depth comes from shape[3]."""
    with tf.variable_scope(name, reuse=tf.AUTO_REUSE):
        W = tf.get_variable("weights", shape=[filter_height, filter_width, shape[3].value, num_filters],
                            initializer=tf.random_normal_initializer(mean=0.0, stddev=STDDEV))
        b = tf.get_variable("biases", shape=[shape[3].value], initializer=tf.constant_initializer(0.0))
        if output_shape is None:
            output_shape = x.get_shape().as_list()
            output_shape[1] *= 2
            output_shape[2] *= 2
            output_shape[3] = W.shape[2]
        deconv = tf.nn.conv2d_transpose(x, W, output_shape, strides=[1, stride, stride, 1], padding=padding)
        return tf.nn.bias_add(deconv, b)


def max_pool(x, name, filter_height=2, filter_width=2, stride=2, padding="VALID"):
    return tf.nn.max_pool(x, ksize=[1, filter_height, filter_width, 1], strides=[1, stride, stride, 1],
                          padding=padding, name=name)


def dropout(x, keep_prob):
    return tf.nn.dropout(x, keep_prob=keep_prob)


def fuse(x1, x2, name):
    return tf.add(x1, x2, name=name)


# ---------------------------------------------------------------------------
# Network/utils/utils.py:164-333
# ---------------------------------------------------------------------------
def Conv2D_Layer(x, num_filters, filter_height=3, filter_width=3, stride=1, padding="SAME", dilation=1,
                 name=None):
    """Bias-free conv with optional dilation (utils.py:164-184)."""
    input_channels = int(x.get_shape()[-1].value)
    with tf.variable_scope(name, reuse=tf.AUTO_REUSE):
        W = tf.get_variable("weights", shape=[filter_height, filter_width, input_channels, num_filters],
                            initializer=tf.random_normal_initializer(mean=0.0, stddev=STDDEV))
        return tf.nn.conv2d(x, W, strides=[1, stride, stride, 1], dilations=dilation, padding=padding)


def Conv2D_Block(x, num_filters, filter_height=3, filter_width=3, stride=1, padding="SAME", dilation=1,
                 batch_normalization=False, relu=False, name=None, activation=None):
    """utils.py:186-208 -- defaults: no BN, no ReLU.

    activation: None, 'relu', 'swish' or 'sigmoid', applied after the optional
    BatchNorm -- the keyword Network/model/EfficientNet.py passes (:190-193,
    :460, :496).  The module that defines it there (Utils_EfficientNet) is
    absent from the reference, so these are the semantics: the activation its
    name says, in the place `relu=True` has."""
    if activation not in (None, "relu", "swish", "sigmoid"):
        raise ValueError(f"Conv2D_Block: activation {activation!r}")
    conv = Conv2D_Layer(x, num_filters, filter_height=filter_height, filter_width=filter_width, stride=stride,
                        padding=padding, dilation=dilation, name=name)
    if batch_normalization is True:
        conv = Batch_Normalization(conv)
    if relu is True:
        conv = tf.nn.relu(conv)
    if activation == "relu":
        conv = tf.nn.relu(conv)
    elif activation == "swish":
        conv = tf.nn.swish(conv)
    elif activation == "sigmoid":
        conv = tf.nn.sigmoid(conv)
    return conv


def Atrous_Conv2D_Layer(x, num_filters, filter_height=3, filter_width=3, dilation=1, padding="SAME",
                        name=None):
    """tf.nn.atrous_conv2d == dilated conv2d (utils.py:210-229)."""
    input_channels = int(x.get_shape()[-1].value)
    with tf.variable_scope(name, reuse=tf.AUTO_REUSE):
        W = tf.get_variable("weights", shape=[filter_height, filter_width, input_channels, num_filters],
                            initializer=tf.random_normal_initializer(mean=0.0, stddev=STDDEV))
        return tf.nn.atrous_conv2d(x, W, dilation, padding=padding)


def Atrous_Conv2D_Block(x, num_filters, filter_height=3, filter_width=3, dilation=1, padding="SAME",
                        batch_normalization=False, relu=False, name=None):
    conv = Atrous_Conv2D_Layer(x, num_filters, filter_height=filter_height, filter_width=filter_width,
                               dilation=dilation, padding=padding, name=name)
    if batch_normalization is True:
        conv = Batch_Normalization(conv)
    if relu is True:
        conv = tf.nn.relu(conv)
    return conv


def Deconv2D_Layer(x, shape, num_filters, output_shape, filter_height=4, filter_width=4, stride=2,
                   padding="SAME", name=None):
    """Bias-free conv2d_transpose, W [kh,kw,shape[3],num_filters] (utils.py:255-274)."""
    with tf.variable_scope(name, reuse=tf.AUTO_REUSE):
        W = tf.get_variable("weights", shape=[filter_height, filter_width, shape[3].value, num_filters],
                            initializer=tf.random_normal_initializer(mean=0.0, stddev=STDDEV))
        if output_shape is None:
            output_shape = x.get_shape().as_list()
            output_shape[1] *= 2
            output_shape[2] *= 2
            output_shape[3] = W.shape[2]
        return tf.nn.conv2d_transpose(x, W, output_shape, strides=[1, stride, stride, 1], padding=padding)


def Deconv2D_Block(x, shape, num_filters, output_shape, filter_height=4, filter_width=4, stride=2,
                   padding="SAME", batch_normalization=False, relu=False, name=None):
    deconv = Deconv2D_Layer(x, shape, num_filters, output_shape, filter_height=filter_height,
                            filter_width=filter_width, stride=stride, padding=padding, name=name)
    if batch_normalization is True:
        deconv = Batch_Normalization(deconv)
    if relu is True:
        deconv = tf.nn.relu(deconv)
    return deconv


def Batch_Normalization(x, axis=3, name=None):
    """tf.layers.batch_normalization(x): training=False, frozen stats (utils.py:300-301).

    axis / name: the arguments Network/model/EfficientNet.py passes (:162, :175,
    :201); its Utils_EfficientNet module is absent from the reference, so these
    are the semantics: the channel axis of NHWC (the only one on the hot path)
    and the layer's variable scope, as tf.layers.batch_normalization(name=)."""
    if axis not in (3, -1):
        raise NotImplementedError("Batch_Normalization: only the channel axis of NHWC")
    return tf.layers.batch_normalization(x, name=name)


def ReLU(x):
    return tf.nn.relu(x)


def Max_Pooling(x, name, filter_height=2, filter_width=2, stride=2, padding="VALID"):
    return tf.nn.max_pool(x, ksize=[1, filter_height, filter_width, 1], strides=[1, stride, stride, 1],
                          padding=padding, name=name)


def Avg_Pooling(x, name, filter_height=2, filter_width=2, stride_height=2, stride_width=2, padding="VALID"):
    return tf.nn.avg_pool(x, ksize=[1, filter_height, filter_width, 1],
                          strides=[1, stride_height, stride_width, 1], padding=padding, name=name)


def Global_Avg_Pool(x, stride=1, name="global_avg_pooling"):
    """utils.py:312-313: tflearn global_avg_pool -> [N, C] (name=: EfficientNet.py:184, :493)."""
    return tf.nn.global_avg_pool(x, name=name)


def Dropout(x, keep_prob):
    return tf.nn.dropout(x, keep_prob=keep_prob)


def Softmax(x):
    return tf.nn.softmax(x)


def Zero_Padding(x, paddings, name):
    """utils.py:325-327: `paddings` zero rows / columns on every side of H and W."""
    pad_mat = [[0, 0], [paddings, paddings], [paddings, paddings], [0, 0]]
    return tf.pad(x, paddings=pad_mat, name=name)


def SepConv_BN(x, filters, prefix, stride=1, kernel_size=3, rate=1, depth_activation=False):
    """Depthwise k x k -> BN -> 1x1 conv + BN + ReLU (Network/model/EfficientNet.py
    :426-462, DeepLabv3Plus.py:23-58).  stride 1: SAME; otherwise explicit zero
    padding of the effective kernel (pad_beg, pad_end) and VALID, the "right SAME
    padding for even kernel sizes" of DeepLabv3Plus.py:37-43.  depth_activation:
    ReLU after the depthwise BN instead of before the depthwise conv."""
    if stride == 1:
        depth_padding = "SAME"
    else:
        k_eff = kernel_size + (kernel_size - 1) * (rate - 1)
        pad_beg = (k_eff - 1) // 2
        pad_end = k_eff - 1 - pad_beg
        x = tf.pad(x, paddings=[[0, 0], [pad_beg, pad_end], [pad_beg, pad_end], [0, 0]],
                   name=prefix + "zero_paddings")
        depth_padding = "VALID"
    if not depth_activation:
        x = ReLU(x)
    filter_shape = [kernel_size, kernel_size, int(x.get_shape()[-1].value), 1]
    filter = tf.get_variable(prefix + "_filter", shape=filter_shape, initializer=tf.glorot_uniform_initializer())
    x = tf.nn.depthwise_conv2d(x, filter=filter, strides=[1, stride, stride, 1], rate=[rate, rate],
                               padding=depth_padding, name=prefix + "_depthwise")
    x = Batch_Normalization(x)
    if depth_activation:
        x = ReLU(x)
    return Conv2D_Block(x, filters, filter_height=1, filter_width=1, stride=1, padding="SAME",
                        batch_normalization=True, relu=True, name=prefix + "_pointwise_BN")


def Resize_Bilinear(x, size, name):
    return tf.image.resize_bilinear(x, size=size, align_corners=True, name=name)


def Concat(x, axis, name):
    return tf.concat(x, axis=axis, name=name)
