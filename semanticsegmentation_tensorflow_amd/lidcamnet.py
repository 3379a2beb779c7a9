"""LidCamNet: the camera + LiDAR road-segmentation net (4 input channels at
160 x 576) -- same layer names, argument binding and quirks as the reference
(Network/model/LidCamNet.py:30-73), on this package's TF1-style graph.

* encoder         conv1 / conv3 / conv5 are 4x4 stride-2 convs (32, 64, 128),
                  conv2 / conv4 3x3                                   (:34-38)
* context module  conv6, conv7 3x3; conv8 ... conv12 3x3 with per-axis
                  dilations [1, dh, dw, 1] = (1,2) (2,4) (4,8) (8,16) (16,32);
                  conv13 3x3, conv14 1x1 VALID; dropout after each   (:41-58)
* decoder         three 4x4 stride-2 transposed convs that take only the
                  SHAPE of conv4 / conv2 / x (no skip tensors: conv19 has x's
                  4 channels), 3x3 convs between, conv21 the head    (:61-67)

Conv2D_Block's defaults hold throughout: no bias, no ReLU anywhere, frozen
batch normalization on every layer but conv21.
"""
from . import tf
from .layers import Conv2D_Block, Deconv2D_Block

KEEP_PROB = 0.8            # Network/model/LidCamNet.py:17
BATCH_SIZE = 4             # :22
IMAGE_SHAPE_KITTI = (160, 576)
CONTEXT_DILATIONS = ([1, 1, 2, 1], [1, 2, 4, 1], [1, 4, 8, 1], [1, 8, 16, 1], [1, 16, 32, 1])


def LidCamNet(x, keep_prob, num_classes, kernel=3, pool_size=(2, 2)):
    """Network/model/LidCamNet.py:30-73 -> (prediction [N,H,W,1], logits)."""
    # encoder
    conv1 = Conv2D_Block(x, 32, filter_height=4, filter_width=4, stride=2, batch_normalization=True, name="conv1")
    conv2 = Conv2D_Block(conv1, 32, batch_normalization=True, name="conv2")
    conv3 = Conv2D_Block(conv2, 64, filter_height=4, filter_width=4, stride=2, batch_normalization=True,
                         name="conv3")
    conv4 = Conv2D_Block(conv3, 64, batch_normalization=True, name="conv4")
    conv5 = Conv2D_Block(conv4, 128, filter_height=4, filter_width=4, stride=2, batch_normalization=True,
                         name="conv5")

    # context module
    h = conv5
    for i in (6, 7):
        h = tf.nn.dropout(Conv2D_Block(h, 128, batch_normalization=True, name=f"conv{i}"), keep_prob)
    for i, d in enumerate(CONTEXT_DILATIONS):
        h = tf.nn.dropout(Conv2D_Block(h, 128, dilation=d, batch_normalization=True, name=f"conv{8 + i}"),
                          keep_prob)
    h = tf.nn.dropout(Conv2D_Block(h, 128, batch_normalization=True, name="conv13"), keep_prob)
    conv14 = tf.nn.dropout(Conv2D_Block(h, 128, filter_height=1, filter_width=1, padding="VALID",
                                        batch_normalization=True, name="conv14"), keep_prob)

    # decoder
    conv15 = Deconv2D_Block(conv14, conv4.get_shape(), 128, tf.shape(conv4), batch_normalization=True,
                            name="conv15")
    conv16 = Conv2D_Block(conv15, 64, batch_normalization=True, name="conv16")
    conv17 = Deconv2D_Block(conv16, conv2.get_shape(), 64, tf.shape(conv2), batch_normalization=True,
                            name="conv17")
    conv18 = Conv2D_Block(conv17, 32, batch_normalization=True, name="conv18")
    conv19 = Deconv2D_Block(conv18, x.get_shape(), 32, tf.shape(x), batch_normalization=True, name="conv19")
    conv20 = Conv2D_Block(conv19, 8, batch_normalization=True, name="conv20")
    conv21 = Conv2D_Block(conv20, num_classes, name="conv21")

    outputs = tf.argmax(conv21, dimension=3, name="prediction")
    return tf.expand_dims(outputs, dim=3), conv21
