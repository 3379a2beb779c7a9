"""Writes efficientseg_b0_variables.txt: the variables `tf.global_variables()`
lists after EfficientSeg(x [N,H,W,3], keep_prob, 'b0', 2), "name d0,d1,..." per
line in creation order.

The table below is read off the reference source, not off this package's
builder (Network/model/EfficientNet.py): the stem (:260-262), the seven stages
of DEFAULT_BLOCK_ARGS (:70-85) at width and depth 1.0 with MBConvBlock
(:153-210) spelled out, the top (:295-296) and the decoder in EfficientSeg's
call order (:492-529) with SepConv_BN (:426-462) as in
make_deeplab_sep_variables.py.

MBConvBlock with prefix p, input width i, output width o, expand ratio e,
kernel k: `p expand_conv` [1,1,i,i e] and the BatchNorm named `p expand_bn`
(only when e != 1), the depthwise filter `p _filter` [k,k,i e,1] at the root
scope, the BatchNorm `p bn`, `p se_reduce` [1,1,i e,max(1,int(i/4))],
`p se_expand` back, `p project_conv` [1,1,i e,o] and the BatchNorm
`p project_bn`.  A stage's first block is prefixed 'bock{n}a_' (the source's
spelling), its repeats 'block{n}b_', 'block{n}c_', ... with i = o.  The named
BatchNorms take no default-name index (TF1), so the decoder's anonymous ones
are batch_normalization, batch_normalization_1, ... from zero."""
import os

NUM_CLASSES = 2
# kernel, repeats, input width, output width, expand ratio -- EfficientNet.py:70-85
STAGES = ((3, 1, 32, 16, 1), (3, 2, 16, 24, 6), (5, 2, 24, 40, 6), (3, 2, 40, 80, 6), (5, 3, 80, 112, 6),
          (5, 4, 112, 192, 7), (3, 1, 192, 320, 6))


def lines():
    out, bn = [], [0]

    def norm(c, name=None):
        if name is None:
            name = "batch_normalization" if bn[0] == 0 else f"batch_normalization_{bn[0]}"
            bn[0] += 1
        return [f"{name}/{v} {c}" for v in ("gamma", "beta", "moving_mean", "moving_variance")]

    def conv(scope, k, cin, cout):
        return [f"{scope}/weights {k},{k},{cin},{cout}"]

    def mbconv(p, k, i, o, e):
        f = i * e
        rows = []
        if e != 1:
            rows += conv(p + "expand_conv", 1, i, f) + norm(f, p + "expand_bn")
        rows += [f"{p}_filter {k},{k},{f},1"] + norm(f, p + "bn")
        r = max(1, int(i * 0.25))
        rows += conv(p + "se_reduce", 1, f, r) + conv(p + "se_expand", 1, r, f)
        return rows + conv(p + "project_conv", 1, f, o) + norm(o, p + "project_bn")

    def sepconv(prefix, cin, cout):
        return [f"{prefix}_filter 3,3,{cin},1"] + norm(cin) + conv(f"{prefix}_pointwise_BN", 1, cin, cout) + norm(cout)

    out += conv("stem_conv", 3, 3, 32) + norm(32, "stem_bn")
    for n, (k, reps, i, o, e) in enumerate(STAGES, 1):
        out += mbconv(f"bock{n}a_", k, i, o, e)
        for letter in "bcdefgh"[:reps - 1]:
            out += mbconv(f"block{n}{letter}_", k, o, o, e)
    out += conv("top_conv", 1, 320, 1280) + norm(1280, "top_bn")
    out += conv("image_pooling", 1, 1280, 256) + norm(256)
    out += conv("aspp0", 1, 1280, 256) + norm(256)
    for i in (1, 2, 3):
        out += sepconv(f"aspp{i}", 1280, 256)
    out += conv("concatenation_conv", 1, 5 * 256, 256) + norm(256)
    out += sepconv("decoder_conv0", 256, 256)
    out += sepconv("decoder_conv1", 256, 256)
    out += conv("last_layer", 1, 256, NUM_CLASSES)
    return out


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "efficientseg_b0_variables.txt"), "w") as f:
        f.write("\n".join(lines()) + "\n")
