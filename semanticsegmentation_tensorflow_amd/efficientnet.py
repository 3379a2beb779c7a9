"""EfficientSeg: the reference's EfficientNet encoder under its separable-ASPP
decoder (Network/model/EfficientNet.py:61-85, :136-299, :464-529), with the
reference's call surface and argument order, built from the layer builders of
layers.py so that the Session runs it on the MI355X kernels.

MBConvBlock is: 1x1 expand conv + BatchNorm + swish (expand_ratio != 1), a
depthwise k x k conv + BatchNorm + swish, squeeze-excite (global average pool,
a 1x1 reduce conv + swish, a 1x1 expand conv + sigmoid, the channel multiply),
a 1x1 project conv + BatchNorm, and the identity add at stride 1 with equal
widths.  Kept as the reference has them:

* each stage's first block is prefixed 'bock{}a_' (sic), the repeats
  'block{}{}_';
* the depthwise filter is `prefix + '_filter'` (so 'bock1a__filter'), created
  with tf.get_variable's default initializer (glorot uniform);
* the squeeze-excite width is max(1, int(input_filters * se_ratio));
* stem and top have no activation (the reference comments them out);
* drop_rate / keep_prob are accepted and unused in the encoder, and the B*
  wrappers pass their resolution and dropout rate (224, 0.2, ...) into the
  dropout_rate / drop_connect_rate slots of EfficientNet, positionally.
"""
import collections
import math
import string

from . import tf
from .deeplab import ASPP_RATES, sep_aspp_head
from .layers import Batch_Normalization, Conv2D_Block, Global_Avg_Pool

BlockArgs = collections.namedtuple("BlockArgs", ["kernel_size", "num_repeat", "input_filters", "output_filters",
                                                 "expand_ratio", "id_skip", "strides", "se_ratio"])
BlockArgs.__new__.__defaults__ = (None,) * len(BlockArgs._fields)

# (kernel, repeats, in, out, expand, stride) of EfficientNet-B0's seven stages
_B0_STAGES = ((3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 2, 40, 80, 6, 2),
              (5, 3, 80, 112, 6, 1), (5, 4, 112, 192, 7, 2), (3, 1, 192, 320, 6, 1))
# the reference's table (its sixth stage expands by 7, not the paper's 6)
DEFAULT_BLOCK_ARGS = [BlockArgs(kernel_size=k, num_repeat=r, input_filters=i, output_filters=o, expand_ratio=e,
                                id_skip=True, strides=[s, s], se_ratio=0.25) for k, r, i, o, e, s in _B0_STAGES]


def round_filters(filters, width_coefficient, depth_divisor):
    """Width scaling: to the nearest multiple of depth_divisor, never more than 10 % down."""
    filters *= width_coefficient
    new_filters = max(depth_divisor, int(filters + depth_divisor / 2) // depth_divisor * depth_divisor)
    if new_filters < 0.9 * filters:
        new_filters += depth_divisor
    return int(new_filters)


def round_repeats(repeats, depth_coefficient):
    """Depth scaling: ceil."""
    return int(math.ceil(depth_coefficient * repeats))


def _activate(x, activation):
    if activation == "relu":
        return tf.nn.relu(x)
    if activation == "swish":
        return tf.nn.swish(x)
    return x


def MBConvBlock(inputs, block_args, activation, drop_rate=None, prefix=""):
    """Mobile inverted residual bottleneck (EfficientNet.py:153-210)."""
    has_se = block_args.se_ratio is not None and 0 < block_args.se_ratio <= 1
    filters = block_args.input_filters * block_args.expand_ratio
    x = inputs
    if block_args.expand_ratio != 1:
        x = Conv2D_Block(x, filters, filter_height=1, filter_width=1, stride=1, padding="SAME",
                         name=prefix + "expand_conv")
        x = _activate(Batch_Normalization(x, axis=3, name=prefix + "expand_bn"), activation)

    k = block_args.kernel_size
    filt = tf.get_variable(prefix + "_filter", shape=[k, k, int(x.get_shape()[-1].value), 1],
                           initializer=tf.glorot_uniform_initializer())
    x = tf.nn.depthwise_conv2d(x, filter=filt, strides=[1, block_args.strides[0], block_args.strides[1], 1],
                               padding="SAME", name=prefix + "dwconv")
    x = _activate(Batch_Normalization(x, axis=3, name=prefix + "bn"), activation)

    if has_se:
        reduced = max(1, int(block_args.input_filters * block_args.se_ratio))
        se = Global_Avg_Pool(x, name=prefix + "se_squeeze")
        se = tf.expand_dims(se, dim=1)
        se = tf.expand_dims(se, dim=1)
        se = Conv2D_Block(se, reduced, filter_height=1, filter_width=1, stride=1, padding="SAME",
                          activation=activation, name=prefix + "se_reduce")
        se = Conv2D_Block(se, filters, filter_height=1, filter_width=1, padding="SAME", activation="sigmoid",
                          name=prefix + "se_expand")
        x = tf.math.multiply(x, se, name=prefix + "se_excite")

    x = Conv2D_Block(x, block_args.output_filters, filter_height=1, filter_width=1, padding="SAME",
                     name=prefix + "project_conv")
    x = Batch_Normalization(x, axis=3, name=prefix + "project_bn")
    if (block_args.id_skip and all(s == 1 for s in block_args.strides)
            and block_args.input_filters == block_args.output_filters):
        x = tf.math.add(x, inputs, name=prefix + "add")
    return x


def EfficientNet(inputs, keep_prob, width_coefficient, depth_coefficient, dropout_rate=0.2, drop_connect_rate=0.2,
                 depth_divisor=8, blocks_args=DEFAULT_BLOCK_ARGS, include_top=True, pooling=None, classes=2):
    """The encoder (EfficientNet.py:213-299): stem conv + BN, the MBConv stages,
    top conv + BN -- no classifier; returns the [N, H/32, W/32, 1280 w] feature map."""
    activation = "swish"
    x = Conv2D_Block(inputs, round_filters(32, width_coefficient, depth_divisor), filter_height=3, filter_width=3,
                     stride=2, padding="SAME", name="stem_conv")
    x = Batch_Normalization(x, axis=3, name="stem_bn")

    total = sum(a.num_repeat for a in blocks_args)
    block_num = 0
    for idx, args in enumerate(blocks_args):
        assert args.num_repeat > 0
        args = args._replace(input_filters=round_filters(args.input_filters, width_coefficient, depth_divisor),
                             output_filters=round_filters(args.output_filters, width_coefficient, depth_divisor),
                             num_repeat=round_repeats(args.num_repeat, depth_coefficient))
        x = MBConvBlock(x, args, activation=activation, drop_rate=drop_connect_rate * float(block_num) / total,
                        prefix="bock{}a_".format(idx + 1))
        block_num += 1
        if args.num_repeat > 1:
            args = args._replace(input_filters=args.output_filters, strides=[1, 1])
            for bidx in range(args.num_repeat - 1):
                x = MBConvBlock(x, args, activation=activation,
                                drop_rate=drop_connect_rate * float(block_num) / total,
                                prefix="block{}{}_".format(idx + 1, string.ascii_lowercase[bidx + 1]))
                block_num += 1

    x = Conv2D_Block(x, round_filters(1280, width_coefficient, depth_divisor), filter_height=1, filter_width=1,
                     padding="SAME", name="top_conv")
    return Batch_Normalization(x, axis=3, name="top_bn")


def _variant(width, depth, resolution, rate):
    def build(inputs, keep_prob, include_top=True, classes=2):
        return EfficientNet(inputs, keep_prob, width, depth, resolution, rate, include_top=include_top,
                            classes=classes)
    return build


EfficientNetB0 = _variant(1.0, 1.0, 224, 0.2)
EfficientNetB1 = _variant(1.0, 1.1, 240, 0.2)
EfficientNetB2 = _variant(1.1, 1.2, 260, 0.3)
EfficientNetB3 = _variant(1.2, 1.4, 300, 0.3)
EfficientNetB4 = _variant(1.4, 1.8, 380, 0.4)
EfficientNetB5 = _variant(1.6, 2.2, 456, 0.4)
EfficientNetB6 = _variant(1.8, 2.6, 528, 0.5)
EfficientNetB7 = _variant(2.0, 3.1, 600, 0.5)
EfficientNetL2 = _variant(4.3, 5.3, 800, 0.5)

_ENCODERS = {"b0": EfficientNetB0, "b1": EfficientNetB1, "b2": EfficientNetB2, "b3": EfficientNetB3,
             "b4": EfficientNetB4, "b5": EfficientNetB5, "b6": EfficientNetB6}


def EfficientSeg(inputs, keep_prob, phi, num_classes, aspp_rates=ASPP_RATES):
    """EfficientNet-`phi` + the separable-ASPP decoder (EfficientNet.py:464-529);
    any phi outside 'b0'..'b6' selects B7, as there.  Returns the logits at the
    input size.  aspp_rates= lets small inputs be tested."""
    H, W = int(inputs.get_shape()[1].value), int(inputs.get_shape()[2].value)
    feature = _ENCODERS.get(phi, EfficientNetB7)(inputs, keep_prob)
    return sep_aspp_head(feature, keep_prob, num_classes, (H, W), aspp_rates=aspp_rates, pool_name="b4")
