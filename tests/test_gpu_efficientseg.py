"""EfficientSeg (efficientnet.py: Network/model/EfficientNet.py:153-299, :464-529)
on the Session vs a float64 restatement written here from oracle.tf1_ops +
tests/dwconv_ref.py + torch.sigmoid, on identical inputs and weights.

* The whole EfficientSeg('b0') in fp32 at 1 x 64 x 96 x 3 (feature map 2 x 3,
  decoder map 4 x 6) with aspp_rates (1, 2, 3): logits and loss within 1e-4,
  every gradient within 2e-3 of its max, one TF1 Adam step within 1e-6 + 1e-5
  max -- the project's fp32 model bounds.  In fp32 the 1344- / 1152-channel
  squeezes and the decoder's 1280-channel pool run on seg_se_squeeze.
* bf16 / f16: EfficientNet with two stages (k3 r1 32->16 e1 s1, k5 r2 16->24 e6
  s2: a 5x5 stride-2 depthwise conv, an identity add, squeeze-excite widths 8,
  4 and 6), a 1x1 conv to the classes and a resize to the input, at
  1 x 32 x 48 x 3.  The reference is rounded (q) at the device's storage
  points; the longest path has 26 of them, DeepLabSepASPP's count, so the
  BOUNDS of tests/test_gpu_lidcamnet.py apply unchanged.

Weights: dense filters ~ N(0, GAIN^2 / fan_in), depthwise filters ~ N(0, GAIN_DW^2
/ (k k)), gamma ~ 1, beta small, with both gains He's sqrt(2) as in the other
model tests.  Checked on the float64 reference alone (and asserted there): at
sqrt(2) the 15-block model has max |logit| 0.44 and no zero gradient although
every sigmoid gate halves the signal (the linear stem, project and top layers
make up for it); a gain of 2 already blows the logits up to 1e7.

A Saver round trip (save, overwrite, restore) gives back the same logits."""
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import ops, tf
from semanticsegmentation_tensorflow_amd.efficientnet import DEFAULT_BLOCK_ARGS, BlockArgs, EfficientNet, EfficientSeg
from semanticsegmentation_tensorflow_amd.layers import Conv2D_Block, Resize_Bilinear
from tests import dwconv_ref
from tests.test_gpu_lidcamnet import BOUNDS

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
RATES = (1, 2, 3)
LR = 1e-4
CLASSES = 2
GAIN = GAIN_DW = math.sqrt(2.0)
TWO_STAGES = [BlockArgs(kernel_size=3, num_repeat=1, input_filters=32, output_filters=16, expand_ratio=1,
                        id_skip=True, strides=[1, 1], se_ratio=0.25),
              BlockArgs(kernel_size=5, num_repeat=2, input_filters=16, output_filters=24, expand_ratio=6,
                        id_skip=True, strides=[2, 2], se_ratio=0.25)]

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
b0 f32 (1x64x96): logits max-rel 3.5e-7 (max |logit| 0.436), loss 0.649003 vs 0.649003, worst gradient 3.4e-6 of
       its max (bock3a_se_reduce/weights), median rel-L2 7.4e-7
two stages bf16 (1x32x48): logits max-rel 3.3e-3 (max |logit| 2.34), loss 0.707180 vs 0.706981, worst cosine 0.99995
       (stem_bn/beta), median rel-L2 5.1e-3, worst max-rel 9.5e-3 (bock2a_expand_bn/beta)
two stages f16: logits max-rel 4.2e-4, loss 0.707190 vs 0.707193, worst cosine 0.999999 (bock1a_bn/beta),
       median rel-L2 6.7e-4
"""


def build(kind, h, w):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, h, w, 3], name="input")
    labels = tf.placeholder(tf.uint8, shape=[None, h, w], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    if kind == "b0":
        logits = EfficientSeg(image, keep, "b0", CLASSES, aspp_rates=RATES)
    else:
        feat = EfficientNet(image, keep, 1.0, 1.0, blocks_args=TWO_STAGES)
        last = Conv2D_Block(feat, CLASSES, filter_height=1, filter_width=1, stride=1, padding="SAME",
                            name="last_layer")
        logits = Resize_Bilinear(last, [h, w], name="output")
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    return image, labels, keep, logits, loss


def make_weights(seed):
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        s = tuple(v.shape)
        if v.var_name.endswith("_filter"):
            out[v.var_name] = (rng.standard_normal(s) * GAIN_DW / math.sqrt(s[0] * s[1])).astype(np.float32)
        elif len(s) == 4:
            out[v.var_name] = (rng.standard_normal(s) * GAIN / math.sqrt(s[0] * s[1] * s[2])).astype(np.float32)
        elif v.var_name.endswith("gamma"):
            out[v.var_name] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        else:
            out[v.var_name] = (0.05 * rng.standard_normal(s)).astype(np.float32)
    return out


def batch(seed, h, w):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((1, h, w, 3)).astype(np.float32)
    lab = np.zeros((1, h, w), np.uint8)
    lab[:, h // 2:, w // 4: 3 * w // 4] = 1
    lab = np.where(rng.random((1, h, w)) < 0.05, 1 - lab, lab).astype(np.uint8)
    return img, lab


def _stages(blocks_args):
    """(prefix, kernel, stride, input width, output width, expand ratio) per block, width / depth 1.0."""
    out = []
    for n, a in enumerate(blocks_args, 1):
        out.append((f"bock{n}a_", a.kernel_size, a.strides[0], a.input_filters, a.output_filters, a.expand_ratio))
        for letter in "bcdefgh"[:a.num_repeat - 1]:
            out.append((f"block{n}{letter}_", a.kernel_size, 1, a.output_filters, a.output_filters, a.expand_ratio))
    return out


def reference(p, x, q, kind):
    """float64 model; q rounds a stored activation through the compute dtype."""
    anon = [0]

    def swish(t):
        return t * torch.sigmoid(t)

    def BN(h, name=None, act=None):
        if name is None:
            name = "batch_normalization" if anon[0] == 0 else f"batch_normalization_{anon[0]}"
            anon[0] += 1
        y = T.batch_norm_frozen(h, p[name + "/gamma"], p[name + "/beta"])
        return q(swish(y) if act == "swish" else T.relu(y) if act == "relu" else y)

    def conv(h, name, stride=1):
        return q(T.conv2d(h, p[name + "/weights"], stride, "SAME"))

    def mbconv(h, prefix, k, stride, i, o, e):
        t = h
        if e != 1:
            t = BN(conv(t, prefix + "expand_conv"), prefix + "expand_bn", "swish")
        t = q(dwconv_ref.depthwise_ad(t, p[prefix + "_filter"], stride, (1, 1), "SAME"))
        t = BN(t, prefix + "bn", "swish")
        se = q(t.mean(dim=(1, 2), keepdim=True))
        se = q(swish(conv(se, prefix + "se_reduce")))
        se = q(torch.sigmoid(conv(se, prefix + "se_expand")))
        t = q(t * se)
        t = BN(conv(t, prefix + "project_conv"), prefix + "project_bn")
        return q(t + h) if (stride == 1 and i == o) else t

    def block(h, name):
        return BN(conv(h, name), act="relu")

    def sepconv(h, prefix, rate=1):
        y = BN(q(dwconv_ref.depthwise_ad(h, p[prefix + "_filter"], 1, (rate, rate), "SAME")), act="relu")
        return block(y, prefix + "_pointwise_BN")

    h = BN(conv(x, "stem_conv", 2), "stem_bn")
    for args in _stages(DEFAULT_BLOCK_ARGS if kind == "b0" else TWO_STAGES):
        h = mbconv(h, *args)
    feat = BN(conv(h, "top_conv"), "top_bn")
    if kind != "b0":
        return q(T.resize_bilinear(conv(feat, "last_layer"), (x.shape[1], x.shape[2])))
    fh, fw = feat.shape[1:3]
    b4 = block(q(feat.mean(dim=(1, 2), keepdim=True)), "image_pooling")
    parts = [q(T.resize_bilinear(b4, (fh, fw))), block(feat, "aspp0")]
    for i, r in enumerate(RATES):
        parts.append(sepconv(feat, f"aspp{i + 1}", r))
    h = block(T.concat(parts), "concatenation_conv")               # keep_prob 1: the Dropout is a copy
    h = q(T.resize_bilinear(h, (2 * fh, 2 * fw)))
    h = sepconv(sepconv(h, "decoder_conv0"), "decoder_conv1")
    assert anon[0] == 13
    return q(T.resize_bilinear(conv(h, "last_layer"), (x.shape[1], x.shape[2])))


def oracle_step(weights, img, lab, dt, kind):
    tdt = TDT[dt]

    class _Q(torch.autograd.Function):        # storage rounding, straight-through gradient
        @staticmethod
        def forward(ctx, t):
            return t.to(tdt).double()

        @staticmethod
        def backward(ctx, g):
            return g
    q = (lambda t: t) if dt == "f32" else _Q.apply
    p = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    # dense filters are read from a packed copy in the compute dtype; depthwise filters as fp32
    p = {k: (q(v) if v.dim() == 4 and not k.endswith("_filter") else v).detach().requires_grad_(True)
         for k, v in p.items()}
    logits = reference(p, q(torch.from_numpy(img).double()), q, kind)
    loss = T.mean_softmax_xent(logits, T.one_hot(torch.from_numpy(lab), CLASSES))
    loss.backward()
    return logits.detach().numpy(), loss.item(), {k: v.grad.numpy() for k, v in p.items()}


def session(dt, weights):
    sess = tf.Session(compute_dtype=dt)
    sess.store_fused_grads = True
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    return sess


def test_weight_draw_keeps_the_signal_in_the_reference():
    """(host) the draw's gains on the float64 reference alone: max |logit| > 0.1
    and no gradient is zero, for both models."""
    torch.set_num_threads(16)
    for kind, h, w in (("b0", 64, 96), ("two", 32, 48)):
        build(kind, h, w)
        weights = make_weights(71)
        img, lab = batch(72, h, w)
        logits, loss, grads = oracle_step(weights, img, lab, "f32", kind)
        assert np.isfinite(logits).all() and np.abs(logits).max() > 0.1, (kind, np.abs(logits).max())
        assert np.abs(logits).max() < 1e3, (kind, np.abs(logits).max())
        zero = [k for k, g in grads.items() if not np.abs(g).max() > 0]
        assert not zero, (kind, zero)


def _run(kind, h, w, dt):
    torch.set_num_threads(16)
    image, labels, keep, logits, loss = build(kind, h, w)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(71)
    img, lab = batch(72, h, w)
    r_logits, r_loss, r_grads = oracle_step(weights, img, lab, dt, kind)
    sess = session(dt, weights)
    scale = sess.loss_scale if dt == "f16" else 1.0
    out_logits, out_loss, _ = sess.run([logits, loss, train], feed_dict={image: img, labels: lab, keep: 1.0})
    torch.cuda.synchronize()
    assert np.abs(r_logits).max() > 0.1
    e_log = np.abs(out_logits - r_logits).max() / np.abs(r_logits).max()
    stats = []
    for k, gr in r_grads.items():
        g = sess.store.grad(k).cpu().numpy().reshape(-1).astype(np.float64) / scale
        r = gr.reshape(-1)
        assert np.linalg.norm(r) > 0, k
        stats.append((g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300),
                      np.linalg.norm(g - r) / np.linalg.norm(r), np.abs(g - r).max() / np.abs(r).max(), k))
    assert len(stats) == len(tf.trainable_variables())
    print(f"EFFICIENTSEG {kind} {dt}: logits max-rel {e_log:.3e} (max |logit| {np.abs(r_logits).max():.3e}), "
          f"loss {float(out_loss):.6f} vs {r_loss:.6f}, worst cosines {sorted(stats)[:3]}, "
          f"median rel-L2 {np.median([s[1] for s in stats]):.3e}, worst max-rel {max(stats, key=lambda s: s[2])[2:]}")
    return sess, weights, out_logits, out_loss, r_logits, r_loss, e_log, stats


def test_efficientseg_b0_fp32_logits_grads_adam(dev):
    sess, weights, out_logits, out_loss, r_logits, r_loss, e_log, stats = _run("b0", 64, 96, "f32")
    plan = list(sess.plans.values())[-1]
    kinds = [n.kind for n in plan.nodes]
    assert kinds.count("se_excite") == 15 and kinds.count("act") == 30 and kinds.count("dwconv") == 20
    # fp32: block6b-d (1344), bock7a (1152) and the decoder's pool (1280) are wider than seg_spatial_reduce takes
    wide = [n for n in plan.nodes if n.kind == "GlobalAvgPool"
            and not ops.spatial_reduce_fits(plan.shapes[id(n.inputs[0])][3], ops.F32)]
    assert len(wide) == 5
    assert e_log < 1e-4, f"logits rel err {e_log:.3e}"
    assert abs(float(out_loss) - r_loss) <= 1e-4 * max(1.0, abs(r_loss)), (out_loss, r_loss)
    for _, _, e, k in stats:
        assert e < 2e-3, f"grad {k} max-rel err {e:.3e}"
    upd = T.AdamTF1(lr=LR).apply({k: torch.from_numpy(v).double() for k, v in weights.items()},
                                 {k: sess.store.grad(k).double().cpu().view(weights[k].shape) for k in weights})
    for k in weights:
        got, ref = sess.variable_value(k), upd[k].numpy()
        assert np.abs(got - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), k
    for k in ("bock1a__filter", "block6d_se_reduce/weights", "bock7a_se_expand/weights", "bock3a_expand_bn/gamma"):
        assert np.abs(sess.variable_value(k) - weights[k]).max() > 0, k


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_two_stage_efficientnet_in_the_compute_dtypes(dev, dt):
    sess, weights, out_logits, out_loss, r_logits, r_loss, e_log, stats = _run("two", 32, 48, dt)
    plan = list(sess.plans.values())[-1]
    dws = [n.desc for n in plan.nodes if n.kind == "dwconv"]
    assert [(d.R, d.stride, d.c_valid) for d in dws] == [(3, 1, 32), (5, 2, 96), (5, 1, 144)]
    assert [n.kind for n in plan.nodes].count("Add") == 1
    tl = BOUNDS[dt]
    assert e_log < tl[0], f"logits rel err {e_log:.3e}"
    assert abs(float(out_loss) - r_loss) <= tl[1] * max(1.0, abs(r_loss)), (out_loss, r_loss)
    assert min(s[0] for s in stats) >= tl[2], sorted(stats)[:3]
    assert np.median([s[1] for s in stats]) <= tl[3]


def test_saver_round_trip_gives_the_same_logits(dev, tmp_path):
    image, labels, keep, logits, loss = build("two", 32, 48)
    weights = make_weights(73)
    img, lab = batch(74, 32, 48)
    sess = session("bf16", weights)
    feed = {image: img, labels: lab, keep: 1.0}
    before = sess.run(logits, feed_dict=feed).copy()
    saver = tf.train.Saver(tf.global_variables())
    path = saver.save(sess, str(tmp_path / "EfficientNet.ckpt"))
    names = ["bock1a__filter", "bock2a_se_reduce/weights", "block2b_expand_bn/gamma", "last_layer/weights"]
    for k in names:
        sess.assign(k, np.zeros_like(weights[k]))
    assert not np.array_equal(sess.run(logits, feed_dict=feed), before)
    saver.restore(sess, path)
    assert np.array_equal(sess.run(logits, feed_dict=feed), before)
    for k in names:
        assert np.array_equal(sess.variable_value(k), weights[k]), k
