"""FC-DenseNet with TransNet camera + LiDAR fusion -- same builder functions,
names, call order and quirks as the reference
(Network/model/FCDenseNet_TransNet.py:27-238), on this package's TF1-style
graph (`semanticsegmentation_tensorflow_amd.tf`).

* bottleneck_layer / Transition_Layer: fcdensenet.py's (the same source text,
  :27-51).
* DenseBlock loops `range(num_bottleneck_layers - 2)` here (:60), unlike
  FCDenseNet.py: a block of n has n - 1 bottleneck layers.
* TransNet (:70-86): alpha, beta = 1x1 convs of [x_img, x_lid]; lid_feat = 1x1
  conv of x_lid (all VALID); relu((alpha + 1) * lid_feat + beta) -> 3x3 conv ->
  relu(x_img + lamda * fuse).  The Session runs the two elementwise forms as
  one launch each (csrc/transnet.hip).
* FCDenseNet (:107-238): two encoders (3-channel image, 1-channel ADI -- the
  LiDAR image), TransNet after transitions 2..5, the sixth block commented out,
  the decoder on the image stream with the transposed-conv input widths
  hard-coded (143 / 572 / 440 / 304 / 224), two auxiliary heads (Dropout ->
  Resize_Bilinear to the input size -> 1x1 conv).  Returns
  (expand_dims(argmax), final_conv, lid_aux_classifier, aux_classifier).

All convolutions are bias-free (utils_transnet.py:207 has the bias commented
out); batch normalization is tf.layers.batch_normalization's inference form.
"""
from . import tf
from .fcdensenet import GROWTH_RATE, N_FILTERS_FIRST_CONV, THETA, Transition_Layer, bottleneck_layer
from .layers import Concat, Conv2D_Block, Deconv2D_Block, Dropout, ReLU, Resize_Bilinear

N_LAYERS_PER_BLOCKS = [4, 5, 7, 10, 12, 15]
KEEP_PROB = 0.2            # Network/model/FCDenseNet_TransNet.py:14
LOSS_WEIGHTS = (1.0, 0.4, 1.6)      # logits, lid_logits, aux_logits (:268-271)


def DenseBlock(x, num_bottleneck_layers, growth_rate, keep_prob, name):
    """Network/model/FCDenseNet_TransNet.py:54-68."""
    layers_concat = [x]
    x = bottleneck_layer(x, growth_rate=growth_rate, keep_prob=keep_prob, name=name + "bottleneck_layer_0")
    layers_concat.append(x)
    for i in range(num_bottleneck_layers - 2):
        x = Concat(layers_concat, axis=-1, name=name + "bottleneck_layer_concatenate_" + str(i + 1))
        x = bottleneck_layer(x, growth_rate=growth_rate, keep_prob=keep_prob,
                             name=name + "bottleneck_layer_" + str(i + 1))
        layers_concat.append(x)
    return Concat(layers_concat, axis=-1, name=name + "bottleneck_layer_concatenate_final")


def TransNet(x_img, x_lid, out_ch, lamda=0.1, name=None):
    """Network/model/FCDenseNet_TransNet.py:70-86."""
    out_ch = int(out_ch)
    concat = Concat([x_img, x_lid], axis=-1, name=name + "_concat")

    alpha = Conv2D_Block(concat, out_ch, filter_height=1, filter_width=1, stride=1, padding="VALID",
                         name=name + "_alpha") + 1
    beta = Conv2D_Block(concat, out_ch, filter_height=1, filter_width=1, stride=1, padding="VALID",
                        name=name + "_beta")
    lid_feat = Conv2D_Block(x_lid, out_ch, filter_height=1, filter_width=1, stride=1, padding="VALID",
                            name=name + "_lid_feat")

    lid_feat = alpha * lid_feat + beta
    lid_feat = ReLU(lid_feat)

    fuse = Conv2D_Block(lid_feat, out_ch, name=name + "_fuse")

    fuse = x_img + lamda * fuse
    fuse = ReLU(fuse)
    return fuse


def FCDenseNet(x_img, x_lid, keep_prob, num_classes, n_layers_per_blocks=None):
    """Network/model/FCDenseNet_TransNet.py:107-238 -> (prediction [N,H,W,1],
    final_conv, lid_aux_classifier, aux_classifier)."""
    n_layers = N_LAYERS_PER_BLOCKS if n_layers_per_blocks is None else list(n_layers_per_blocks)
    shape = tf.shape(x_img)[1:3]

    def block(x, i, stream):
        return DenseBlock(x, n_layers[i - 1], growth_rate=GROWTH_RATE, keep_prob=keep_prob,
                          name=f"denseblock{i}_{stream}")

    def down(x, i, stream):
        return Transition_Layer(x, theta=THETA, name=f"transition_layer{i}_{stream}")

    dense_init_img = Conv2D_Block(x_img, N_FILTERS_FIRST_CONV, name="dense_init_img")
    dense_init_lid = Conv2D_Block(x_lid, N_FILTERS_FIRST_CONV, name="dense_init_lid")

    dense_block1_img = block(dense_init_img, 1, "img")
    transition_down1_img = down(dense_block1_img, 1, "img")
    dense_block1_lid = block(dense_init_lid, 1, "lid")
    transition_down1_lid = down(dense_block1_lid, 1, "lid")

    dense_block2_img = block(transition_down1_img, 2, "img")
    transition_down2_img = down(dense_block2_img, 2, "img")
    dense_block2_lid = block(transition_down1_lid, 2, "lid")
    transition_down2_lid = down(dense_block2_lid, 2, "lid")
    trans1 = TransNet(transition_down2_img, transition_down2_lid, transition_down2_img.get_shape()[-1], name="trans1")

    dense_block3_img = block(trans1, 3, "img")
    transition_down3_img = down(dense_block3_img, 3, "img")
    dense_block3_lid = block(transition_down2_lid, 3, "lid")
    transition_down3_lid = down(dense_block3_lid, 3, "lid")
    trans2 = TransNet(transition_down3_img, transition_down3_lid, transition_down3_img.get_shape()[-1], name="trans2")

    dense_block4_img = block(trans2, 4, "img")
    transition_down4_img = down(dense_block4_img, 4, "img")
    dense_block4_lid = block(transition_down3_lid, 4, "lid")
    transition_down4_lid = down(dense_block4_lid, 4, "lid")
    trans3 = TransNet(transition_down4_img, transition_down4_lid, transition_down4_img.get_shape()[-1], name="trans3")

    # the auxiliary head: dropout, resize to the input size, then the 1x1 conv -- in this order
    aux_loss = Dropout(trans3, keep_prob=keep_prob)
    aux_loss_interp = Resize_Bilinear(aux_loss, shape, name="aux_loss_interp")
    aux_classifier = Conv2D_Block(aux_loss_interp, num_classes, filter_height=1, filter_width=1, stride=1,
                                  name="aux_classifier")

    dense_block5_img = block(trans3, 5, "img")
    transition_down5_img = down(dense_block5_img, 5, "img")
    dense_block5_lid = block(transition_down4_lid, 5, "lid")
    transition_down5_lid = down(dense_block5_lid, 5, "lid")
    trans4 = TransNet(transition_down5_img, transition_down5_lid, transition_down5_img.get_shape()[-1], name="trans4")

    # (the sixth block is commented out in the reference, :189-193)
    lid_aux_classifier = Dropout(trans4, keep_prob=keep_prob)
    lid_aux_classifier = Resize_Bilinear(lid_aux_classifier, shape, name="lid_aux_classifier_interp")
    lid_aux_classifier = Conv2D_Block(lid_aux_classifier, num_classes, filter_height=1, filter_width=1, stride=1,
                                      name="lid_aux_loss")

    # decoder: the reference hard-codes the transposed-conv input widths
    transition_up1 = Deconv2D_Block(trans4, dense_block5_img.get_shape(), 143, tf.shape(dense_block5_img),
                                    name="transition_up1")
    tu_db_concat1 = Concat([transition_up1, dense_block5_img], axis=-1, name="tu_db_concat1")
    transition_up2 = Deconv2D_Block(tu_db_concat1, dense_block4_img.get_shape(), 572, tf.shape(dense_block4_img),
                                    name="transition_up2")
    tu_db_concat2 = Concat([transition_up2, dense_block4_img], axis=-1, name="tu_db_concat2")
    transition_up3 = Deconv2D_Block(tu_db_concat2, dense_block3_img.get_shape(), 440, tf.shape(dense_block3_img),
                                    name="transition_up3")
    tu_db_concat3 = Concat([transition_up3, dense_block3_img], axis=-1, name="tu_db_concat3")
    transition_up4 = Deconv2D_Block(tu_db_concat3, dense_block2_img.get_shape(), 304, tf.shape(dense_block2_img),
                                    name="transition_up4")
    tu_db_concat4 = Concat([transition_up4, dense_block2_img], axis=-1, name="tu_db_concat4")
    transition_up5 = Deconv2D_Block(tu_db_concat4, dense_block1_img.get_shape(), 224, tf.shape(dense_block1_img),
                                    name="transition_up5")
    tu_db_concat5 = Concat([transition_up5, dense_block1_img], axis=-1, name="tu_db_concat5")

    final_conv = Conv2D_Block(tu_db_concat5, num_classes, filter_height=1, filter_width=1, name="final_conv")
    prediction = tf.argmax(final_conv, dimension=3, name="prediction")
    return tf.expand_dims(prediction, dim=3), final_conv, lid_aux_classifier, aux_classifier


def training_loss(logits, lid_logits, aux_logits, labels):
    """(loss, training_loss) of the reference driver (:267-271): the main head's
    loss for the summary, and the weighted three-head loss that is minimised."""
    xent = tf.nn.softmax_cross_entropy_with_logits
    loss = tf.reduce_mean(xent(logits=logits, labels=labels))
    total = tf.reduce_mean(xent(logits=logits, labels=labels) + 0.4 * xent(logits=lid_logits, labels=labels)
                           + 1.6 * xent(logits=aux_logits, labels=labels))
    return loss, total
