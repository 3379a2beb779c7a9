"""PSPNet50: a ResNet-50-shaped encoder and a pyramid pooling head for the
4-channel 160 x 576 KITTI road input -- same layer names, argument binding and
quirks as the reference (Network/model/PSPNet.py:26-181), on this package's
TF1-style graph.

* stem      Zero_Padding(3) -> 7x7 stride-2 VALID conv (64) -> Zero_Padding(1)
            -> 3x3 stride-2 VALID max pool: 160 x 576 -> 80 x 288 -> 40 x 144
                                                                      (:30-34)
* stages    3 + 4 + 6 + 3 bottlenecks (1x1 -> 3x3 -> 1x1, widths 64 / 128 /
            256 / 512, expansions 256 ... 2048); stages 3, 4 and 5 open with
            two 1x1 stride-2 convs (the reducing conv and the shortcut):
            20 x 72, 10 x 36, 5 x 18                                (:37-139)
* head      encoder_output 1x1 (512); four average pools with stride = window
            (PYRAMID_WINDOWS), each followed by a 1x1 conv (128) + BN + ReLU;
            all five resized to the input size, concatenated (1024), then
            conv5_4 3x3 (128) + BN + ReLU and conv6 1x1         (:141-176)

The reference's quirks are kept:

* Conv2D_Block's arguments are passed by position one slot early.  The calls
  ending `'VALID', True, True` bind dilation=True (TF reads it as 1),
  batch_normalization=True and leave relu=False; those ending `'VALID', True`
  bind dilation=True alone.  So in the encoder only the reducing and the 3x3
  convs are batch-normalised, the expanding and shortcut convs are bare, and
  the only ReLUs are the ones after each tf.add.  The head's convs and conv5_4
  are called with keywords and do get BN + ReLU.
* The scope name "conv1" is also the name of both paddings; the first block of
  stage 3 uses the scopes conv3_1 / conv3_2 / conv3_3.
* The residuals of conv3_3, conv3_4 and conv5_3 add conv3_1, conv3_1 and
  conv5_1, not the block before them.
"""
from . import tf
from .layers import Avg_Pooling, Concat, Conv2D_Block, Max_Pooling, Resize_Bilinear, Zero_Padding

KEEP_PROB = 0.8                    # Network/model/PSPNet.py:13
NUM_OF_CLASSESS = 2                # :15
IMAGE_SHAPE_KITTI = (160, 576)     # :16
BATCH_SIZE = 1                     # :20
EPOCHS = 50                        # :21
LEARNING_RATE = 1e-4               # :22
# the pools' (height, width) windows = strides, written out in the reference
# for the 5 x 18 encoder map of a 160 x 576 input (:147-166)
PYRAMID_WINDOWS = ((5, 18), (3, 9), (2, 6), (1, 3))


def _bottleneck(x, width, tag, names=None, stride=1, last_padding="VALID"):
    """1x1 (BN) -> 3x3 (BN) -> 1x1 expanding to 4 * width (bare): the three
    convs before a block's tf.add; `names` overrides the scopes `tag`_1.._3."""
    n1, n2, n3 = names or (f"{tag}_1", f"{tag}_2", f"{tag}_3")
    h = Conv2D_Block(x, width, 1, 1, stride, "VALID", True, True, name=n1)
    h = Conv2D_Block(h, width, 3, 3, 1, "SAME", True, True, name=n2)
    return Conv2D_Block(h, 4 * width, 1, 1, 1, last_padding, True, name=n3)


def PSPNet50(x, num_classes, pyramid_windows=PYRAMID_WINDOWS):
    """Network/model/PSPNet.py:26-181 -> (prediction [N,H,W,1], logits).
    pyramid_windows: the four average pools' windows, for inputs whose
    encoder map is not 5 x 18."""
    # stage 1
    conv1 = Zero_Padding(x, paddings=3, name="conv1")
    conv1 = Conv2D_Block(conv1, 64, 7, 7, 2, "VALID", True, True, name="conv1")
    conv1 = Zero_Padding(conv1, paddings=1, name="conv1")
    pool1 = Max_Pooling(conv1, filter_height=3, filter_width=3, stride=2, name="pool1")

    # stage 2
    conv2_1_3 = _bottleneck(pool1, 64, "conv2_1")
    shortcut1 = Conv2D_Block(pool1, 256, 1, 1, 1, "VALID", True, name="shortcut1")
    conv2_1 = tf.nn.relu(tf.add(conv2_1_3, shortcut1, name="conv2_1"))
    conv2_2 = tf.nn.relu(tf.add(_bottleneck(conv2_1, 64, "conv2_2"), conv2_1, name="conv2_2"))
    conv2_3 = tf.nn.relu(tf.add(_bottleneck(conv2_2, 64, "conv2_3", last_padding="SAME"), conv2_2, name="conv2_3"))

    # stage 3
    conv3_1_3 = _bottleneck(conv2_3, 128, None, names=("conv3_1", "conv3_2", "conv3_3"), stride=2)
    shortcut2 = Conv2D_Block(conv2_3, 512, 1, 1, 2, "VALID", True, name="shortcut2")
    conv3_1 = tf.nn.relu(tf.add(conv3_1_3, shortcut2, name="conv3_1"))
    conv3_2 = tf.nn.relu(tf.add(_bottleneck(conv3_1, 128, "conv3_2"), conv3_1, name="conv3_2"))
    conv3_3 = tf.nn.relu(tf.add(_bottleneck(conv3_2, 128, "conv3_3"), conv3_1, name="conv3_3"))
    conv3_4 = tf.nn.relu(tf.add(_bottleneck(conv3_3, 128, "conv3_4"), conv3_1, name="conv3_4"))

    # stage 4
    conv4_1_3 = _bottleneck(conv3_4, 256, "conv4_1", stride=2)
    shortcut3 = Conv2D_Block(conv3_4, 1024, 1, 1, 2, "VALID", True, name="shortcut3")
    conv4_1 = tf.nn.relu(tf.add(conv4_1_3, shortcut3, name="conv4_1"))
    conv4_2 = tf.nn.relu(tf.add(_bottleneck(conv4_1, 256, "conv4_2"), conv4_1, name="conv4_2"))
    h = conv4_2
    for i in (3, 4, 5, 6):
        h = tf.nn.relu(tf.add(_bottleneck(h, 256, f"conv4_{i}"), h, name=f"conv4_{i}"))
    conv4_6 = h

    # stage 5
    conv5_1_3 = _bottleneck(conv4_6, 512, "conv5_1", stride=2)
    shortcut4 = Conv2D_Block(conv4_6, 2048, 1, 1, 2, "VALID", True, name="shortcut4")
    conv5_1 = tf.nn.relu(tf.add(conv5_1_3, shortcut4, name="conv5_1"))
    conv5_2 = tf.nn.relu(tf.add(_bottleneck(conv5_1, 512, "conv5_2"), conv5_1, name="conv5_2"))
    conv5_3 = tf.nn.relu(tf.add(_bottleneck(conv5_2, 512, "conv5_3"), conv5_1, name="conv5_3"))

    encoder_output = Conv2D_Block(conv5_3, 512, 1, 1, 1, "SAME", name="encoder_output")

    # pyramid pooling head
    shape = tf.shape(x)[1:3]
    branches = [Resize_Bilinear(encoder_output, shape, name="conv5_3_interp")]
    for tag, (kh, kw) in zip(("pool1", "pool2", "pool3", "pool6"), pyramid_windows):
        pooled = Avg_Pooling(encoder_output, filter_height=kh, filter_width=kw, stride_height=kh, stride_width=kw,
                             name=f"conv5_3_{tag}")
        pooled = Conv2D_Block(pooled, 128, filter_height=1, filter_width=1, stride=1, batch_normalization=True,
                              relu=True, name=f"conv5_3_{tag}_conv")
        branches.append(Resize_Bilinear(pooled, shape, name=f"conv5_3_{tag}_interp"))
    concatenation = Concat(branches, axis=-1, name="concatenation")

    conv5_4 = Conv2D_Block(concatenation, 128, batch_normalization=True, relu=True, name="conv5_4")
    conv6 = Conv2D_Block(conv5_4, num_classes, filter_height=1, filter_width=1, stride=1, name="conv6")

    prediction = tf.argmax(conv6, dimension=3, name="prediction")
    return tf.expand_dims(prediction, dim=3), conv6


def build_train_graph(image_shape=IMAGE_SHAPE_KITTI, num_classes=NUM_OF_CLASSESS, batch_size=BATCH_SIZE,
                      learning_rate=LEARNING_RATE, pyramid_windows=PYRAMID_WINDOWS):
    """The graph of the reference driver (Network/model/PSPNet.py:599-636):
    placeholders, PSPNet50, the loss, and the accumulate-then-apply train
    step -- zero the accumulators, add 3 / batch_size times each batch's
    gradient, then Adam on the accumulators.  Returns a dict of its handles."""
    H, W = image_shape
    keep_probability = tf.placeholder(tf.float32, name="keep_probability")
    image = tf.placeholder(tf.float32, shape=[None, H, W, 4], name="input_image")
    prediction = tf.placeholder(tf.float32, shape=[None, H, W, num_classes], name="prediction")
    pred_annotation, logits = PSPNet50(image, num_classes, pyramid_windows=pyramid_windows)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=prediction))
    optimizer = tf.train.AdamOptimizer(learning_rate)
    const = tf.constant(1 / batch_size * 3)
    t_vars = tf.trainable_variables()
    accum_tvars = [tf.Variable(tf.zeros_like(t_var.initialized_value()), trainable=False) for t_var in t_vars]
    zero_ops = [tv.assign(tf.zeros_like(tv)) for tv in accum_tvars]
    batch_grads_vars = optimizer.compute_gradients(loss, t_vars)
    accum_ops = [accum_tvars[i].assign_add(tf.scalar_mul(const, gv[0])) for i, gv in enumerate(batch_grads_vars)]
    train_step = optimizer.apply_gradients([(accum_tvars[i], gv[1]) for i, gv in enumerate(batch_grads_vars)])
    return {"image": image, "prediction": prediction, "keep_probability": keep_probability,
            "pred_annotation": pred_annotation, "logits": logits, "loss": loss, "zero_ops": zero_ops,
            "accum_ops": accum_ops, "train_step": train_step}


def run(get_batches_fn, epochs=EPOCHS, batch_size=BATCH_SIZE, image_shape=IMAGE_SHAPE_KITTI, checkpoint_dir=None,
        compute_dtype="bf16", pyramid_windows=PYRAMID_WINDOWS):
    """The reference's training loop (Network/model/PSPNet.py:585-702) on a
    batch source: `get_batches_fn(batch_size)` yields (images [B,H,W,4],
    one-hot labels [B,H,W,2]).  Per batch: zero the accumulators, run the
    accumulation once per image of the batch, then one Adam step (:685-690).
    Restores from and saves to `checkpoint_dir` when given; returns the
    Session."""
    import os

    tf.reset_default_graph()
    g = build_train_graph(image_shape, NUM_OF_CLASSESS, batch_size, LEARNING_RATE, pyramid_windows)
    sess = tf.Session(compute_dtype=compute_dtype)
    global_step = tf.Variable(0, trainable=False, name="global_step")
    saver = tf.train.Saver(tf.global_variables())
    sess.run(tf.global_variables_initializer())
    ckpt = tf.train.get_checkpoint_state(checkpoint_dir) if checkpoint_dir else None
    if ckpt and ckpt.model_checkpoint_path:
        saver.restore(sess, ckpt.model_checkpoint_path)
    for _ in range(epochs):
        for images, labels in get_batches_fn(batch_size):
            feed_dict = {g["image"]: images, g["prediction"]: labels, g["keep_probability"]: KEEP_PROB}
            sess.run(g["zero_ops"])
            for _i in range(len(images)):
                sess.run(g["accum_ops"], feed_dict=feed_dict)
            sess.run(g["train_step"], feed_dict=feed_dict)
    if checkpoint_dir:
        saver.save(sess, os.path.join(checkpoint_dir, "PSPNet.ckpt"), global_step=global_step)
    return sess
