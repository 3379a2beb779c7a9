"""FC-DenseNet + TransNet (fcdensenet_transnet.py:
Network/model/FCDenseNet_TransNet.py:27-238, :267-271) on the Session vs a
float64 restatement written here from oracle.tf1_ops + tests/transnet_ref.py, on
identical inputs and weights.

* The full-depth model in fp32 at 1 x 64 x 96 (image 3 channels, ADI 1 channel;
  the TransNet maps are 16x24x56, 8x12x76, 4x6x110 and 2x3x143), uint8 labels,
  keep_prob 1 as in tests/test_gpu_fcdensenet.py: the logits of the three heads
  and the weighted loss mean(xent + 0.4 xent_lid + 1.6 xent_aux) within 1e-4,
  every gradient within 2e-3 of its max, one TF1 Adam step within 1e-6 + 1e-5
  max -- the project's fp32 model bounds.
* bf16 / f16 at 1 x 32 x 48 on a short two-stream model: a 3x3 stem (44 wide)
  on the image and on the ADI, one Transition_Layer each (22 channels at
  16 x 24: the kernels see C = 24, c_valid = 22), one TransNet, and two heads on
  its output -- Resize_Bilinear -> 1x1 conv, and Dropout -> Resize_Bilinear ->
  1x1 conv -- under mean(xent + 1.6 xent_aux).  The reference is rounded (q) at
  the device's storage points; the longest path has 11 of them (input, stem,
  BN + ReLU, 1x1 conv, pool, alpha conv, modulation, fuse conv, fusion, resize,
  classifier), within the 26 the BOUNDS of tests/test_gpu_lidcamnet.py were
  set for, so they apply unchanged.

Weights: filters ~ N(0, 2 / fan_in) (He; transposed convs with fan_in =
(k / stride)^2 C_in), gamma ~ 1, beta small, as in the other model tests -- not
the reference's stddev 0.01, under which every head is ~0.  Asserted on the
float64 reference alone (no GPU): every head's max |logit| > 0.1 and no
gradient is all zero.

A second loss fetched beside the train step leaves every gradient bit for bit
as it was; a Saver round trip gives back the same logits."""
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.fcdensenet import Transition_Layer
from semanticsegmentation_tensorflow_amd.fcdensenet_transnet import (N_LAYERS_PER_BLOCKS, FCDenseNet, TransNet,
                                                                     training_loss)
from semanticsegmentation_tensorflow_amd.layers import Conv2D_Block, Dropout, Resize_Bilinear
from tests import transnet_ref as R
from tests.test_gpu_lidcamnet import BOUNDS

gpu = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LR = 1e-4
CLASSES = 2
STEM = 44
TCONV_IN = (143, 572, 440, 304, 224)

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
full f32 (1x64x96): logits max-rel 1.2e-6 / 9.5e-7 / 1.2e-6 (max |logit| 8.41 / 1.28 / 0.762), weighted loss
       2.805498 vs 2.805497, worst gradient 4.1e-4 of its max (denseblock1_lidbottleneck_layer_2_conv1/weights),
       worst cosine 0.99999999 (batch_normalization_11/gamma), median rel-L2 5.4e-7
short bf16 (1x32x48): logits max-rel 1.6e-3 / 1.7e-8 (max |logit| 2.45 / 3.48), weighted loss 3.441415 vs
       3.441417, worst cosine 0.999999 (dense_init_lid/weights), median rel-L2 5.7e-4, worst max-rel 1.7e-3
short f16: logits max-rel 4.0e-4 / 5.6e-4, weighted loss 3.438425 vs 3.438421, worst cosine 0.99999998
       (dense_init_lid/weights), median rel-L2 6.6e-5, worst max-rel 1.3e-4
"""


def build(kind, h, w):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, h, w, 3], name="input_image")
    adi = tf.placeholder(tf.float32, shape=[None, h, w, 1], name="input_adi")
    labels = tf.placeholder(tf.uint8, shape=[None, h, w], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    if kind == "full":
        _, logits, lid_logits, aux_logits = FCDenseNet(image, adi, keep, CLASSES)
        loss, total = training_loss(logits, lid_logits, aux_logits, labels)
        heads = [logits, lid_logits, aux_logits]
    else:
        si = Conv2D_Block(image, STEM, name="dense_init_img")
        sl = Conv2D_Block(adi, STEM, name="dense_init_lid")
        ti = Transition_Layer(si, theta=0.5, name="transition_layer1_img")
        tl = Transition_Layer(sl, theta=0.5, name="transition_layer1_lid")
        trans = TransNet(ti, tl, ti.get_shape()[-1], name="trans1")
        size = tf.shape(image)[1:3]
        logits = Conv2D_Block(Resize_Bilinear(trans, size, name="interp"), CLASSES, filter_height=1, filter_width=1,
                              stride=1, name="final_conv")
        aux = Resize_Bilinear(Dropout(trans, keep_prob=keep), size, name="aux_loss_interp")
        aux_logits = Conv2D_Block(aux, CLASSES, filter_height=1, filter_width=1, stride=1, name="aux_classifier")
        xent = tf.nn.softmax_cross_entropy_with_logits
        loss = tf.reduce_mean(xent(logits=logits, labels=labels))
        total = tf.reduce_mean(xent(logits=logits, labels=labels) + 1.6 * xent(logits=aux_logits, labels=labels))
        heads = [logits, aux_logits]
    return image, adi, labels, keep, heads, loss, total


def make_weights(seed):
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        s = tuple(v.shape)
        if len(s) == 4:
            fan = (s[0] // 2) * (s[1] // 2) * s[3] if v.var_name.startswith("transition_up") else s[0] * s[1] * s[2]
            out[v.var_name] = (rng.standard_normal(s) * math.sqrt(2.0 / fan)).astype(np.float32)
        elif v.var_name.endswith("gamma"):
            out[v.var_name] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        else:
            out[v.var_name] = (0.05 * rng.standard_normal(s)).astype(np.float32)
    return out


def batch(seed, h, w):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((1, h, w, 3)).astype(np.float32)
    adi = rng.standard_normal((1, h, w, 1)).astype(np.float32)
    lab = np.zeros((1, h, w), np.uint8)
    lab[:, h // 2:, w // 4: 3 * w // 4] = 1
    lab = np.where(rng.random((1, h, w)) < 0.05, 1 - lab, lab).astype(np.uint8)
    return img, adi, lab


def reference(p, x_img, x_lid, q, kind):
    """float64 model -> the heads' logits; q rounds a stored activation through
    the compute dtype.  keep_prob 1: every Dropout is a copy."""
    anon = [0]

    def BN_relu(h):
        name = "batch_normalization" if anon[0] == 0 else f"batch_normalization_{anon[0]}"
        anon[0] += 1
        return q(T.relu(T.batch_norm_frozen(h, p[name + "/gamma"], p[name + "/beta"])))

    def conv(h, name):
        return q(T.conv2d(h, p[name + "/weights"], 1, "SAME"))

    def bottleneck(h, name):
        h = conv(BN_relu(h), name + "_conv1")
        return conv(BN_relu(h), name + "_conv2")

    def dense_block(h, n, name):
        feats = [h, bottleneck(h, name + "bottleneck_layer_0")]
        for i in range(n - 2):
            feats.append(bottleneck(T.concat(feats), f"{name}bottleneck_layer_{i + 1}"))
        return T.concat(feats)

    def transition(h, name):
        return q(T.avg_pool2x2(conv(BN_relu(h), name + "_conv")))

    def head(h, name):
        return conv(q(T.resize_bilinear(h, (x_img.shape[1], x_img.shape[2]))), name)

    def transnet(a, b, name):
        return R.transnet(a, b, p, name, 0.1, q)

    hi, hl = conv(x_img, "dense_init_img"), conv(x_lid, "dense_init_lid")
    if kind != "full":
        trans = transnet(transition(hi, "transition_layer1_img"), transition(hl, "transition_layer1_lid"), "trans1")
        return [head(trans, "final_conv"), head(trans, "aux_classifier")]
    skips = []
    aux = None
    for s in range(1, 6):
        db = dense_block(hi, N_LAYERS_PER_BLOCKS[s - 1], f"denseblock{s}_img")
        skips.append(db)
        hi = transition(db, f"transition_layer{s}_img")
        hl = transition(dense_block(hl, N_LAYERS_PER_BLOCKS[s - 1], f"denseblock{s}_lid"), f"transition_layer{s}_lid")
        if s >= 2:
            hi = transnet(hi, hl, f"trans{s - 1}")
        if s == 4:
            aux = head(hi, "aux_classifier")
    lid = head(hi, "lid_aux_loss")
    h = hi
    for u, skip in enumerate(reversed(skips), 1):
        assert h.shape[3] == TCONV_IN[u - 1]
        t = q(T.conv2d_transpose(h, p[f"transition_up{u}/weights"], tuple(skip.shape), 2))
        h = T.concat([t, skip])
    return [conv(h, "final_conv"), lid, aux]


def weights_of(kind):
    return (1.0, 0.4, 1.6) if kind == "full" else (1.0, 1.6)


def oracle_step(weights, img, adi, lab, dt, kind):
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
    # filters are read from a packed copy in the compute dtype
    p = {k: (q(v) if v.dim() == 4 else v).detach().requires_grad_(True) for k, v in p.items()}
    heads = reference(p, q(torch.from_numpy(img).double()), q(torch.from_numpy(adi).double()), q, kind)
    onehot = T.one_hot(torch.from_numpy(lab), CLASSES)
    losses = [T.mean_softmax_xent(h, onehot) for h in heads]
    total = sum(w * l for w, l in zip(weights_of(kind), losses))
    total.backward()
    return ([h.detach().numpy() for h in heads], losses[0].item(), total.item(),
            {k: v.grad.numpy() for k, v in p.items()})


def session(dt, weights):
    sess = tf.Session(compute_dtype=dt)
    sess.store_fused_grads = True
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    return sess


def test_weight_draw_keeps_the_signal_in_the_reference():
    """(host) on the float64 reference alone: every head's max |logit| > 0.1 and
    no gradient is all zero, for both models."""
    torch.set_num_threads(16)
    for kind, h, w in (("full", 64, 96), ("short", 32, 48)):
        build(kind, h, w)
        weights = make_weights(81)
        img, adi, lab = batch(82, h, w)
        heads, loss, total, grads = oracle_step(weights, img, adi, lab, "f32", kind)
        for i, lg in enumerate(heads):
            assert np.isfinite(lg).all() and 0.1 < np.abs(lg).max() < 1e3, (kind, i, np.abs(lg).max())
        assert set(grads) == {v.var_name for v in tf.trainable_variables()}
        zero = [k for k, g in grads.items() if not np.abs(g).max() > 0]
        assert not zero, (kind, zero)
        assert total > loss > 0


def _run(kind, h, w, dt):
    torch.set_num_threads(16)
    image, adi_t, labels, keep, heads, loss, total = build(kind, h, w)
    train = tf.train.AdamOptimizer(LR).minimize(total)
    weights = make_weights(81)
    img, adi, lab = batch(82, h, w)
    r_heads, r_loss, r_total, r_grads = oracle_step(weights, img, adi, lab, dt, kind)
    sess = session(dt, weights)
    scale = sess.loss_scale if dt == "f16" else 1.0
    out = sess.run(heads + [total, train], feed_dict={image: img, adi_t: adi, labels: lab, keep: 1.0})
    torch.cuda.synchronize()
    out_heads, out_total = out[:len(heads)], float(out[len(heads)])
    e_log = []
    for o, r in zip(out_heads, r_heads):
        assert np.abs(r).max() > 0.1
        e_log.append(np.abs(o - r).max() / np.abs(r).max())
    stats = []
    for k, gr in r_grads.items():
        g = sess.store.grad(k).cpu().numpy().reshape(-1).astype(np.float64) / scale
        r = gr.reshape(-1)
        assert np.linalg.norm(r) > 0, k
        stats.append((g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300),
                      np.linalg.norm(g - r) / np.linalg.norm(r), np.abs(g - r).max() / np.abs(r).max(), k))
    assert len(stats) == len(tf.trainable_variables())
    print(f"FCDENSENET_TRANSNET {kind} {dt}: logits max-rel {['%.3e' % e for e in e_log]} "
          f"(max |logit| {['%.3g' % np.abs(r).max() for r in r_heads]}), weighted loss {out_total:.6f} vs "
          f"{r_total:.6f}, worst cosines {sorted(stats)[:2]}, median rel-L2 "
          f"{np.median([s[1] for s in stats]):.3e}, worst max-rel {max(stats, key=lambda s: s[2])[2:]}")
    return sess, weights, out_total, r_total, e_log, stats


@gpu
def test_full_depth_fp32_logits_loss_grads_adam(dev):
    sess, weights, out_total, r_total, e_log, stats = _run("full", 64, 96, "f32")
    plan = list(sess.plans.values())[-1]
    kinds = [n.kind for n in plan.nodes]
    assert kinds.count("film") == 4 and kinds.count("axpy") == 4 and kinds.count("xent") == 3
    assert [plan.shapes[id(n.output)] for n in plan.nodes if n.kind == "axpy"] == \
        [(1, 16, 24, 56), (1, 8, 12, 76), (1, 4, 6, 110), (1, 2, 3, 143)]
    for e in e_log:
        assert e < 1e-4, f"logits rel err {e:.3e}"
    assert abs(out_total - r_total) <= 1e-4 * max(1.0, abs(r_total)), (out_total, r_total)
    for _, _, e, k in stats:
        assert e < 2e-3, f"grad {k} max-rel err {e:.3e}"
    upd = T.AdamTF1(lr=LR).apply({k: torch.from_numpy(v).double() for k, v in weights.items()},
                                 {k: sess.store.grad(k).double().cpu().view(weights[k].shape) for k in weights})
    for k in weights:
        got, ref = sess.variable_value(k), upd[k].numpy()
        assert np.abs(got - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), k
    for k in ("dense_init_lid/weights", "trans1_alpha/weights", "trans4_fuse/weights", "lid_aux_loss/weights"):
        assert np.abs(sess.variable_value(k) - weights[k]).max() > 0, k


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_short_two_stream_model_in_the_compute_dtypes(dev, dt):
    sess, weights, out_total, r_total, e_log, stats = _run("short", 32, 48, dt)
    plan = list(sess.plans.values())[-1]
    film = [n for n in plan.nodes if n.kind == "film"]
    assert len(film) == 1 and plan.shapes[id(film[0].output)] == (1, 16, 24, 22)
    assert plan.buf[id(film[0].output)].shape[3] == 24
    tl = BOUNDS[dt]
    assert max(e_log) < tl[0], f"logits rel err {max(e_log):.3e}"
    assert abs(out_total - r_total) <= tl[1] * max(1.0, abs(r_total)), (out_total, r_total)
    assert min(s[0] for s in stats) >= tl[2], sorted(stats)[:3]
    assert np.median([s[1] for s in stats]) <= tl[3]


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_second_loss_beside_the_step_leaves_the_gradients_unchanged(dev, dt):
    """The summary loss of the main head fetched with the step
    (FCDenseNet_TransNet.py:361) must not add that head's gradient again."""
    image, adi_t, labels, keep, heads, loss, total = build("short", 32, 48)
    train = tf.train.AdamOptimizer(LR).minimize(total)
    weights = make_weights(83)
    img, adi, lab = batch(84, 32, 48)
    feed = {image: img, adi_t: adi, labels: lab, keep: 1.0}
    grads = []
    for fetches in ([train], [train, loss, total], [train, loss]):
        sess = session(dt, weights)
        out = sess.run(fetches, feed_dict=feed)
        torch.cuda.synchronize()
        grads.append({k: sess.store.grad(k).cpu().clone() for k in weights})
        if len(fetches) == 3:
            # both fetched losses against each other: total = loss + 1.6 * aux, aux > 0
            assert float(out[2]) > float(out[1]) > 0
    for other in grads[1:]:
        for k in weights:
            assert torch.equal(grads[0][k], other[k]), k
    assert all(float(g.abs().max()) > 0 for g in grads[0].values())


@gpu
def test_saver_round_trip_gives_the_same_logits(dev, tmp_path):
    image, adi_t, labels, keep, heads, loss, total = build("short", 32, 48)
    weights = make_weights(85)
    img, adi, lab = batch(86, 32, 48)
    sess = session("bf16", weights)
    feed = {image: img, adi_t: adi, labels: lab, keep: 1.0}
    before = [a.copy() for a in sess.run(heads, feed_dict=feed)]
    saver = tf.train.Saver(tf.global_variables())
    path = saver.save(sess, str(tmp_path / "FCDenseNet_TransNet.ckpt"))
    names = ["dense_init_lid/weights", "trans1_alpha/weights", "trans1_fuse/weights", "batch_normalization_1/gamma"]
    for k in names:
        sess.assign(k, np.zeros_like(weights[k]))
    assert not np.array_equal(sess.run(heads[0], feed_dict=feed), before[0])
    saver.restore(sess, path)
    after = sess.run(heads, feed_dict=feed)
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    for k in names:
        assert np.array_equal(sess.variable_value(k), weights[k]), k
