"""Writes fcdensenet_transnet_variables.txt: the variables `tf.global_variables()`
lists after FCDenseNet(image [N,H,W,3], adi [N,H,W,1], keep_prob, 2) of
Network/model/FCDenseNet_TransNet.py, "name d0,d1,..." per line in creation
order.

The table below is read off the reference source, not off this package's
builder: the two stems (:121-122); per stage the image DenseBlock and
Transition_Layer, then the LiDAR ones (:126-140, :147-152, :159-164, :177-182);
TransNet after transitions 2..5 (:143, :155, :167, :185) with its four convs
in call order alpha, beta, lid_feat, fuse (:73-81); the auxiliary classifier
after trans3 (:174) and the LiDAR one after trans4 (:197); five transposed convs
[4,4,out,in] with the hard-coded input widths (:211-227); final_conv (:233).

DenseBlock(n) (:54-68) has 1 + (n - 2) bottleneck layers; a bottleneck layer
(:27-39) is BatchNorm(c), `<name>_conv1` [1,1,c,64], BatchNorm(64), `<name>_conv2`
[3,3,64,16]; Transition_Layer (:42-51) is BatchNorm(c), `<name>_conv`
[1,1,c,c // 2].  Convs are bias-free (utils_transnet.py:207).  Every BatchNorm is
anonymous: batch_normalization, batch_normalization_1, ... in creation order,
each with gamma, beta, moving_mean, moving_variance."""
import os

NUM_CLASSES = 2
FIRST, GROWTH = 48, 16
N_LAYERS = [4, 5, 7, 10, 12, 15]
TCONV_IN = (143, 572, 440, 304, 224)


def lines():
    out, bn = [], [0]

    def norm(c):
        name = "batch_normalization" if bn[0] == 0 else f"batch_normalization_{bn[0]}"
        bn[0] += 1
        return [f"{name}/{v} {c}" for v in ("gamma", "beta", "moving_mean", "moving_variance")]

    def conv(scope, k, cin, cout):
        return [f"{scope}/weights {k},{k},{cin},{cout}"]

    def bottleneck(name, c):
        return (norm(c) + conv(name + "_conv1", 1, c, 4 * GROWTH) + norm(4 * GROWTH)
                + conv(name + "_conv2", 3, 4 * GROWTH, GROWTH))

    def dense_block(name, c, n):
        rows = []
        for i in range(n - 1):
            rows += bottleneck(f"{name}bottleneck_layer_{i}", c)
            c += GROWTH
        return rows, c

    def transition(name, c):
        return norm(c) + conv(name + "_conv", 1, c, c // 2), c // 2

    def transnet(name, c):
        return (conv(name + "_alpha", 1, 2 * c, c) + conv(name + "_beta", 1, 2 * c, c)
                + conv(name + "_lid_feat", 1, c, c) + conv(name + "_fuse", 3, c, c))

    out += conv("dense_init_img", 3, 3, FIRST) + conv("dense_init_lid", 3, 1, FIRST)
    c_img = c_lid = FIRST
    skips = []
    for stage in range(1, 6):
        rows, c_img = dense_block(f"denseblock{stage}_img", c_img, N_LAYERS[stage - 1])
        out += rows
        skips.append(c_img)
        rows, c_img = transition(f"transition_layer{stage}_img", c_img)
        out += rows
        rows, c_lid = dense_block(f"denseblock{stage}_lid", c_lid, N_LAYERS[stage - 1])
        out += rows
        rows, c_lid = transition(f"transition_layer{stage}_lid", c_lid)
        out += rows
        if stage >= 2:
            assert c_img == c_lid
            out += transnet(f"trans{stage - 1}", c_img)
        if stage == 4:
            out += conv("aux_classifier", 1, c_img, NUM_CLASSES)
    out += conv("lid_aux_loss", 1, c_img, NUM_CLASSES)
    c = c_img
    for i, (skip, cin) in enumerate(zip(reversed(skips), TCONV_IN), 1):
        assert c == cin, (i, c, cin)
        out.append(f"transition_up{i}/weights 4,4,{skip},{cin}")
        c = 2 * skip
    out += conv("final_conv", 1, c, NUM_CLASSES)
    return out


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fcdensenet_transnet_variables.txt"), "w") as f:
        f.write("\n".join(lines()) + "\n")
