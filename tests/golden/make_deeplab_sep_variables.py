"""Writes deeplab_sep_variables.txt: the variables `tf.global_variables()` lists
after DeepLabSepASPP(x [N,H,W,3], keep_prob, 2), "name d0,d1,..." per line in
creation order.

The table below is read off the sources, not off this package's builder: the
VGG atrous backbone's conv_layer scopes (Network/model/FCN.py:55-83: weights
then biases), then the head in the call order of EfficientSeg
(Network/model/EfficientNet.py:492-529) with SepConv_BN (:426-462) spelled out:
its depthwise filter `prefix_filter` [3,3,C,1] at the root scope, a
batch_normalization of C channels, then the `prefix_pointwise_BN` 1x1 weights
and their batch_normalization.  tf.layers.batch_normalization names its scopes
batch_normalization, batch_normalization_1, ... in call order."""
import os

NUM_CLASSES = 2


def lines():
    out, bn = [], [0]

    def norm(c):
        base = "batch_normalization" if bn[0] == 0 else f"batch_normalization_{bn[0]}"
        bn[0] += 1
        return [f"{base}/{v} {c}" for v in ("gamma", "beta", "moving_mean", "moving_variance")]

    def block(scope, cin, cout, bn_=True):
        return [f"{scope}/weights 1,1,{cin},{cout}"] + (norm(cout) if bn_ else [])

    def sepconv(prefix, cin, cout):
        return [f"{prefix}_filter 3,3,{cin},1"] + norm(cin) + block(f"{prefix}_pointwise_BN", cin, cout)

    cin = 3
    for scope, cout in (("conv1_1", 64), ("conv1_2", 64), ("conv2_1", 128), ("conv2_2", 128), ("conv3_1", 256),
                        ("conv3_2", 256), ("conv3_3", 256), ("conv4_1", 512), ("conv4_2", 512), ("conv4_3", 512),
                        ("conv5_1", 512), ("conv5_2", 512), ("conv5_3", 512)):
        out += [f"{scope}/weights 3,3,{cin},{cout}", f"{scope}/biases {cout}"]
        cin = cout
    out += block("image_pooling", 512, 256)
    out += block("aspp0", 512, 256)
    for i in (1, 2, 3):
        out += sepconv(f"aspp{i}", 512, 256)
    out += block("concatenation_conv", 5 * 256, 256)
    out += sepconv("decoder_conv0", 256, 256)
    out += sepconv("decoder_conv1", 256, 256)
    out += block("last_layer", 256, NUM_CLASSES, bn_=False)
    return out


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "deeplab_sep_variables.txt"), "w") as f:
        f.write("\n".join(lines()) + "\n")
