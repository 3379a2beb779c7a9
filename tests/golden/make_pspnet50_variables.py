"""Writes pspnet50_variables.txt: the variables `tf.global_variables()` lists
after PSPNet50(x [N,H,W,4], 2), "name d0,d1,..." per line in creation order.

The table below is read off the reference source (Network/model/PSPNet.py:26-181
with Conv2D_Block's signature, Network/utils/utils.py:186-208), not off this
package's builder: one row per Conv2D_Block call in source order -- scope,
filter height, filter width, input depth, output depth, and whether the call
binds batch_normalization=True.  Under the positional misbinding only calls
ending `True, True` do (the reducing and the 3x3 conv of every bottleneck, and
conv1); the expanding and shortcut convs do not; the keyword calls of the head
do.  tf.layers.batch_normalization names its scopes batch_normalization,
batch_normalization_1, ... in call order."""
import os


def bottleneck(names, cin, width):
    n1, n2, n3 = names
    return [(n1, 1, 1, cin, width, True), (n2, 3, 3, width, width, True), (n3, 1, 1, width, 4 * width, False)]


def table():
    rows = [("conv1", 7, 7, 4, 64, True)]
    # (first block's scopes, the other blocks' prefixes, shortcut, stage input depth, width)
    stages = [(("conv2_1_1", "conv2_1_2", "conv2_1_3"), ["conv2_2", "conv2_3"], "shortcut1", 64, 64),
              (("conv3_1", "conv3_2", "conv3_3"), ["conv3_2", "conv3_3", "conv3_4"], "shortcut2", 256, 128),
              (("conv4_1_1", "conv4_1_2", "conv4_1_3"), [f"conv4_{i}" for i in range(2, 7)], "shortcut3", 512, 256),
              (("conv5_1_1", "conv5_1_2", "conv5_1_3"), ["conv5_2", "conv5_3"], "shortcut4", 1024, 512)]
    for first, rest, shortcut, cin, width in stages:
        rows += bottleneck(first, cin, width)
        rows.append((shortcut, 1, 1, cin, 4 * width, False))
        for tag in rest:
            rows += bottleneck((f"{tag}_1", f"{tag}_2", f"{tag}_3"), 4 * width, width)
    rows.append(("encoder_output", 1, 1, 2048, 512, False))
    for tag in ("pool1", "pool2", "pool3", "pool6"):
        rows.append((f"conv5_3_{tag}_conv", 1, 1, 512, 128, True))
    rows.append(("conv5_4", 3, 3, 512 + 4 * 128, 128, True))
    rows.append(("conv6", 1, 1, 128, 2, False))
    return rows


def lines():
    out, bn = [], 0
    for scope, kh, kw, cin, cout, norm in table():
        out.append(f"{scope}/weights {kh},{kw},{cin},{cout}")
        if norm:
            base = "batch_normalization" if bn == 0 else f"batch_normalization_{bn}"
            bn += 1
            out += [f"{base}/{v} {cout}" for v in ("gamma", "beta", "moving_mean", "moving_variance")]
    return out


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "pspnet50_variables.txt"), "w") as f:
        f.write("\n".join(lines()) + "\n")
