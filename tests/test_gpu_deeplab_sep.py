"""DeepLabSepASPP (deeplab.py: the reference's EfficientSeg head,
Network/model/EfficientNet.py:492-529, on the VGG atrous backbone) on the
Session vs a float64 restatement written here from oracle.tf1_ops +
tests/dwconv_ref.py, on identical inputs and weights.

Small model: 1 x 32 x 48 x 3 (feature map 4 x 6, decoder map 8 x 12) with
aspp_rates (1, 2, 3), and one fp32 run with the default rates 6 / 12 / 18,
where on the 4 x 6 map every off-centre tap of the ASPP depthwise convs lies in
the padding (their filter gradients are exact zeros).  Weights are drawn at
sqrt(2 / fan_in) and assigned, gamma ~ 1 and beta randomised, as the other
model tests do.

fp32: logits 1e-4 of max, loss 1e-4, every gradient 2e-3 of its max, one TF1
Adam step 1e-6 + 1e-5 max (tests/test_gpu_pspnet.py's fp32 bounds).  bf16 /
f16: the reference rounded at the device's storage points, BOUNDS of
tests/test_gpu_lidcamnet.py (26 storage points on the longest path here,
against LidCamNet's 21).  Measured values: see MEASURED below.

A Saver round trip (save, overwrite, restore) gives back the same logits."""
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.deeplab import ASPP_RATES, DeepLabSepASPP
from tests import dwconv_ref
from tests.test_gpu_lidcamnet import BOUNDS

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SMALL_RATES = (1, 2, 3)
LR = 1e-4
N, H, W, CLASSES = 1, 32, 48, 2
FILTERS = [f"aspp{i}_filter" for i in (1, 2, 3)] + ["decoder_conv0_filter", "decoder_conv1_filter"]

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
(1, 2, 3) f32: logits max-rel 8.8e-7, worst gradient 1.1e-6 of its max (conv1_1/biases)
(6, 12, 18) f32: logits max-rel 9.3e-7, worst gradient 1.8e-6 of its max (batch_normalization_12/gamma)
(1, 2, 3) bf16: logits max-rel 9.2e-3, loss 0.564959 vs 0.564685, worst cosine 0.9916 (conv1_1/weights),
               median rel-L2 4.6e-2
(1, 2, 3) f16: logits max-rel 1.7e-3, loss 0.564658 vs 0.564637, worst cosine 0.9979 (conv1_1/weights),
              median rel-L2 9.4e-3
"""


def build(rates):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 3], name="input_image")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    pred, logits = DeepLabSepASPP(image, keep, CLASSES, aspp_rates=rates)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    return image, labels, keep, pred, logits, loss


def make_weights(seed):
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        s = tuple(v.shape)
        if v.var_name.endswith("_filter"):
            out[v.var_name] = (rng.standard_normal(s) * math.sqrt(2.0 / (s[0] * s[1]))).astype(np.float32)
        elif len(s) == 4:
            out[v.var_name] = (rng.standard_normal(s) * math.sqrt(2.0 / (s[0] * s[1] * s[2]))).astype(np.float32)
        elif v.var_name.endswith("gamma"):
            out[v.var_name] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        else:
            out[v.var_name] = (0.05 * rng.standard_normal(s)).astype(np.float32)
    return out


def batch(seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((N, H, W, 3)).astype(np.float32)
    lab = np.zeros((N, H, W), np.uint8)
    lab[:, H // 2:, W // 4: 3 * W // 4] = 1
    lab = np.where(rng.random((N, H, W)) < 0.05, 1 - lab, lab).astype(np.uint8)
    return img, lab


def reference(p, x, q, rates):
    """float64 DeepLabSepASPP; q rounds a stored activation through the compute
    dtype.  Batch-normalised layers take their scope in call order, as TF."""
    count = [0]

    def BN(h, relu=True):
        i = count[0]
        count[0] += 1
        base = "batch_normalization" if i == 0 else f"batch_normalization_{i}"
        y = T.batch_norm_frozen(h, p[base + "/gamma"], p[base + "/beta"])
        return q(T.relu(y)) if relu else q(y)

    def cl(h, name, rate=1):
        return q(T.relu(T.conv2d(h, p[name + "/weights"], 1, "SAME", rate) + p[name + "/biases"]))

    def block(h, name, norm=True):
        y = q(T.conv2d(h, p[name + "/weights"], 1, "SAME"))
        return BN(y) if norm else y

    def sepconv(h, prefix, rate=1):             # depth_activation=True: ReLU after the depthwise BN
        y = BN(q(dwconv_ref.depthwise_ad(h, p[prefix + "_filter"], 1, (rate, rate), "SAME")))
        return block(y, prefix + "_pointwise_BN")

    h = cl(cl(x, "conv1_1"), "conv1_2")
    h = T.max_pool2x2(h)
    h = cl(cl(h, "conv2_1"), "conv2_2")
    h = T.max_pool2x2(h)
    h = cl(cl(cl(h, "conv3_1"), "conv3_2"), "conv3_3")
    h = T.max_pool2x2(h)
    h = cl(cl(cl(h, "conv4_1"), "conv4_2"), "conv4_3")
    feat = cl(cl(cl(h, "conv5_1", 2), "conv5_2", 2), "conv5_3", 2)
    fh, fw = feat.shape[1:3]
    b4 = block(q(feat.mean(dim=(1, 2), keepdim=True)), "image_pooling")
    parts = [q(T.resize_bilinear(b4, (fh, fw))), block(feat, "aspp0")]
    for i, r in enumerate(rates):
        parts.append(sepconv(feat, f"aspp{i + 1}", r))
    h = block(T.concat(parts), "concatenation_conv")             # keep_prob 1: the Dropout is a copy
    h = q(T.resize_bilinear(h, (2 * fh, 2 * fw)))
    h = sepconv(sepconv(h, "decoder_conv0"), "decoder_conv1")
    last = block(h, "last_layer", norm=False)
    assert count[0] == 13
    return q(T.resize_bilinear(last, (x.shape[1], x.shape[2])))


def oracle_step(weights, img, lab, dt, rates):
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
    logits = reference(p, q(torch.from_numpy(img).double()), q, rates)
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


@pytest.mark.parametrize("rates,dt", [(SMALL_RATES, "f32"), (SMALL_RATES, "bf16"), (SMALL_RATES, "f16"),
                                      (ASPP_RATES, "f32")])
def test_deeplab_sep_logits_grads_adam(dev, rates, dt):
    torch.set_num_threads(16)
    image, labels, keep, pred, logits, loss = build(rates)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(61)
    img, lab = batch(62)
    r_logits, r_loss, r_grads = oracle_step(weights, img, lab, dt, rates)
    sess = session(dt, weights)
    scale = sess.loss_scale if dt == "f16" else 1.0
    out_logits, out_loss, _ = sess.run([logits, loss, train], feed_dict={image: img, labels: lab, keep: 1.0})
    torch.cuda.synchronize()
    plan = list(sess.plans.values())[-1]
    dws = [n for n in plan.nodes if n.kind == "dwconv"]
    assert [n.w.var_name for n in dws] == FILTERS
    assert [(n.desc.H, n.desc.W, n.desc.C, n.desc.dil_h) for n in dws] == \
        [(4, 6, 512, r) for r in rates] + [(8, 12, 256, 1)] * 2
    assert np.abs(r_logits).max() > 0.1                    # the signal survives the depth
    e_log = np.abs(out_logits - r_logits).max() / np.abs(r_logits).max()
    stats = []
    for k, gr in r_grads.items():
        g = sess.store.grad(k).cpu().numpy().reshape(-1).astype(np.float64) / scale
        r = gr.reshape(-1)
        assert np.linalg.norm(r) > 0, k
        stats.append((g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300),
                      np.linalg.norm(g - r) / np.linalg.norm(r), np.abs(g - r).max() / np.abs(r).max(), k))
    assert len(stats) == 13 * 2 + 9 + 5 + 13 * 2
    print(f"DEEPLABSEP {rates} {dt}: logits max-rel {e_log:.3e} (max |logit| {np.abs(r_logits).max():.3e}), "
          f"loss {float(out_loss):.6f} vs {r_loss:.6f}, worst cosines {sorted(stats)[:3]}, "
          f"median rel-L2 {np.median([s[1] for s in stats]):.3e}, worst max-rel {max(stats, key=lambda s: s[2])[2:]}")
    if dt == "f32":
        assert e_log < 1e-4, f"logits rel err {e_log:.3e}"
        assert abs(float(out_loss) - r_loss) <= 1e-4 * max(1.0, abs(r_loss)), (out_loss, r_loss)
        for _, _, e, k in stats:
            assert e < 2e-3, f"grad {k} max-rel err {e:.3e}"
    else:
        tl = BOUNDS[dt]
        assert e_log < tl[0], f"logits rel err {e_log:.3e}"
        assert abs(float(out_loss) - r_loss) <= tl[1] * max(1.0, abs(r_loss)), (out_loss, r_loss)
        assert min(s[0] for s in stats) >= tl[2], sorted(stats)[:3]
        assert np.median([s[1] for s in stats]) <= tl[3]
    if rates == ASPP_RATES:
        # every off-centre tap of the ASPP depthwise convs lies in the padding of the 4 x 6 map
        for k in FILTERS[:3]:
            g = sess.store.grad(k).cpu().view(3, 3, 512)
            centre = torch.zeros(3, 3, dtype=torch.bool)
            centre[1, 1] = True
            assert bool((g[~centre] == 0).all()) and g[1, 1].abs().max().item() > 0, k
            assert np.all(r_grads[k].reshape(3, 3, 512)[~centre.numpy()] == 0)
    if dt != "f16":
        # one TF1 Adam step of the step's own gradient on every variable, the depthwise filters among them
        upd = T.AdamTF1(lr=LR).apply({k: torch.from_numpy(v).double() for k, v in weights.items()},
                                     {k: sess.store.grad(k).double().cpu().view(weights[k].shape) for k in weights})
        for k in weights:
            got, ref = sess.variable_value(k), upd[k].numpy()
            assert np.abs(got - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), k
        assert all(np.abs(sess.variable_value(k) - weights[k]).max() > 0 for k in FILTERS)


def test_saver_round_trip_gives_the_same_logits(dev, tmp_path):
    image, labels, keep, pred, logits, loss = build(SMALL_RATES)
    weights = make_weights(63)
    img, lab = batch(64)
    sess = session("bf16", weights)
    feed = {image: img, labels: lab, keep: 1.0}
    before = sess.run(logits, feed_dict=feed).copy()
    saver = tf.train.Saver(tf.global_variables())
    path = saver.save(sess, str(tmp_path / "DeepLabSep.ckpt"))
    for k in FILTERS + ["aspp1_pointwise_BN/weights", "last_layer/weights"]:
        sess.assign(k, np.zeros_like(weights[k]))
    assert not np.array_equal(sess.run(logits, feed_dict=feed), before)
    saver.restore(sess, path)
    assert np.array_equal(sess.run(logits, feed_dict=feed), before)
    for k in FILTERS:
        assert np.array_equal(sess.variable_value(k), weights[k]), k
