"""PSPNet50 (Network/model/PSPNet.py:26-181) on the Session vs a float64
restatement written here from oracle.tf1_ops + tests/pool_ref.py, on identical
inputs and weights.

Small model: 1 x 64 x 96 x 4 with pyramid_windows ((2, 3), (1, 3), (2, 1),
(1, 1)) on the 2 x 3 encoder map (pyramid maps 1x1, 2x1, 1x3, 2x3).  The
weights are drawn at 1/sqrt(fan_in) and assigned, and the frozen BatchNorm's
gamma ~ 1 and beta are randomised, as tests/test_gpu_lidcamnet.py does and for
its reason: the reference's N(0, 0.01) init through 60 layers leaves no signal
to compare.

fp32: logits 1e-4 of max, every gradient 2e-3 of its max, one TF1 Adam step
1e-6 + 1e-5 max (tests/test_gpu_fcn.py's fp32 bounds).  bf16 / f16: the
reference rounded at the device's storage points, BOUNDS of
tests/test_gpu_lidcamnet.py.  Measured on an MI355X: fp32 logits 1.2e-6,
worst gradient 2.5e-6 of its max; bf16 logits 9.1e-3, loss 9.6401 vs 9.6464,
worst cosine 0.985, median rel-L2 9.5e-2 (bound 0.1: 60 layers of bf16
storage, against LidCamNet's 21); f16 logits 1.1e-3, worst cosine 0.9989,
median rel-L2 2.5e-2.

Full size: one bf16 train step at 1 x 160 x 576 with the default windows --
finite loss, and the pyramid head (four pools, their 1x1 conv + BN + ReLU, the
resizes) layer by layer against float64 on the device's own buffers."""
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import ops, tf
from semanticsegmentation_tensorflow_amd.pspnet import PYRAMID_WINDOWS, PSPNet50
from tests import pool_ref
from tests.gpu_utils import assert_close
from tests.test_gpu_lidcamnet import BOUNDS

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SMALL_WINDOWS = ((2, 3), (1, 3), (2, 1), (1, 1))
LR = 1e-4
POOL_TAGS = ("pool1", "pool2", "pool3", "pool6")


def build(H, W, windows):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 4], name="input_image")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    pred, logits = PSPNet50(image, 2, pyramid_windows=windows)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    return image, labels, pred, logits, loss


def make_weights(seed):
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        s = tuple(v.shape)
        if len(s) == 4:
            out[v.var_name] = (rng.standard_normal(s) / math.sqrt(s[0] * s[1] * s[2])).astype(np.float32)
        elif v.var_name.endswith("gamma"):
            out[v.var_name] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        else:
            out[v.var_name] = (0.1 * rng.standard_normal(s)).astype(np.float32)
    return out


def batch(N, H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((N, H, W, 4)).astype(np.float32)
    lab = np.zeros((N, H, W), np.uint8)
    lab[:, H // 2:, W // 4: 3 * W // 4] = 1
    lab = np.where(rng.random((N, H, W)) < 0.05, 1 - lab, lab).astype(np.uint8)
    return img, lab


def reference(p, x, q, windows):
    """float64 PSPNet50; q rounds a stored activation through the compute
    dtype.  Batch-normalised layers take their scope in call order, as TF."""
    count = [0]

    def conv(h, name, k=1, stride=1, pad="VALID", norm=False, relu=False):
        w = p[name + "/weights"]
        assert w.shape[0] == w.shape[1] == k
        y = q(T.conv2d(h, w, stride, pad))
        if norm:
            i = count[0]
            count[0] += 1
            bn = "batch_normalization" if i == 0 else f"batch_normalization_{i}"
            y = T.batch_norm_frozen(y, p[bn + "/gamma"], p[bn + "/beta"])
            y = q(T.relu(y)) if relu else q(y)
        return y

    def block(h, names, stride=1, last_pad="VALID"):
        a = conv(h, names[0], 1, stride, "VALID", norm=True)
        b = conv(a, names[1], 3, 1, "SAME", norm=True)
        return conv(b, names[2], 1, 1, last_pad)

    def three(tag):
        return tag + "_1", tag + "_2", tag + "_3"

    def join(a, b):
        return q(T.relu(q(a + b)))

    H, W = x.shape[1:3]
    h = conv(q(pool_ref.pad_ad(x, (3, 3, 3, 3))), "conv1", 7, 2, "VALID", norm=True)
    h = q(pool_ref.max_pool_ad(q(pool_ref.pad_ad(h, (1, 1, 1, 1))), (3, 3), (2, 2), "VALID"))
    # stage 2
    b = block(h, three("conv2_1"))
    c2_1 = join(b, conv(h, "shortcut1"))
    c2_2 = join(block(c2_1, three("conv2_2")), c2_1)
    c2_3 = join(block(c2_2, three("conv2_3"), last_pad="SAME"), c2_2)
    # stage 3: the residuals of the third and fourth block add the first block's output
    b = block(c2_3, ("conv3_1", "conv3_2", "conv3_3"), stride=2)
    c3_1 = join(b, conv(c2_3, "shortcut2", 1, 2))
    c3_2 = join(block(c3_1, three("conv3_2")), c3_1)
    c3_3 = join(block(c3_2, three("conv3_3")), c3_1)
    c3_4 = join(block(c3_3, three("conv3_4")), c3_1)
    # stage 4
    b = block(c3_4, three("conv4_1"), stride=2)
    h = join(b, conv(c3_4, "shortcut3", 1, 2))
    for i in range(2, 7):
        h = join(block(h, three(f"conv4_{i}")), h)
    # stage 5: the third block adds the first block's output
    b = block(h, three("conv5_1"), stride=2)
    c5_1 = join(b, conv(h, "shortcut4", 1, 2))
    c5_2 = join(block(c5_1, three("conv5_2")), c5_1)
    c5_3 = join(block(c5_2, three("conv5_3")), c5_1)
    enc = conv(c5_3, "encoder_output", 1, 1, "SAME")
    parts = [q(T.resize_bilinear(enc, (H, W)))]
    for tag, k in zip(POOL_TAGS, windows):
        pooled = q(pool_ref.avg_pool_ad(enc, k, k, "VALID"))
        parts.append(q(T.resize_bilinear(conv(pooled, f"conv5_3_{tag}_conv", 1, 1, "SAME", norm=True, relu=True), (H, W))))
    h = conv(T.concat(parts), "conv5_4", 3, 1, "SAME", norm=True, relu=True)
    out = conv(h, "conv6", 1, 1, "SAME")
    assert count[0] == 38
    return out


def oracle_step(weights, img, lab, dt, windows):
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
    p = {k: (q(v) if v.dim() == 4 else v).detach().requires_grad_(True) for k, v in p.items()}
    logits = reference(p, q(torch.from_numpy(img).double()), q, windows)
    loss = T.mean_softmax_xent(logits, T.one_hot(torch.from_numpy(lab), 2))
    loss.backward()
    return logits.detach().numpy(), loss.item(), {k: v.grad.numpy() for k, v in p.items()}


def session(dt, weights):
    sess = tf.Session(compute_dtype=dt)
    sess.store_fused_grads = True
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    return sess


_ORACLE = {}


def small_oracle(dt):
    """The float64 step of the small model, computed once per dtype."""
    if dt not in _ORACLE:
        torch.set_num_threads(16)
        build(64, 96, SMALL_WINDOWS)
        weights = make_weights(51)
        img, lab = batch(1, 64, 96, 52)
        _ORACLE[dt] = (weights, img, lab) + oracle_step(weights, img, lab, dt, SMALL_WINDOWS)
    return _ORACLE[dt]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_pspnet50_small_logits_grads_adam(dev, dt):
    N, H, W = 1, 64, 96
    weights, img, lab, r_logits, r_loss, r_grads = small_oracle(dt)
    image, labels, pred, logits, loss = build(H, W, SMALL_WINDOWS)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    sess = session(dt, weights)
    scale = sess.loss_scale if dt == "f16" else 1.0
    out_logits, out_loss, _ = sess.run([logits, loss, train], feed_dict={image: img, labels: lab})
    torch.cuda.synchronize()
    plan = list(sess.plans.values())[-1]
    enc = next(n for n in plan.nodes if n.kind == "conv" and n.w.var_name == "encoder_output/weights")
    assert plan.shapes[id(enc.output)] == (N, 2, 3, 512)
    pools = [n for n in plan.nodes if n.kind == "Pool2D" and n.desc.kind == ops.POOL_AVG]
    assert [tuple(plan.shapes[id(n.output)][1:3]) for n in pools] == [(1, 1), (2, 1), (1, 3), (2, 3)]
    assert len([n for n in plan.nodes if n.kind == "Subsample"]) == 3
    assert np.abs(r_logits).max() > 0.1                    # the signal survives 60 layers
    e_log = np.abs(out_logits - r_logits).max() / np.abs(r_logits).max()
    print(f"PSPNET {dt}: logits max-rel {e_log:.3e} (max |logit| {np.abs(r_logits).max():.3e}), "
          f"loss {float(out_loss):.6f} vs {r_loss:.6f}")
    stats = []
    for k, gr in r_grads.items():
        g = sess.store.grad(k).cpu().numpy().reshape(-1).astype(np.float64) / scale
        r = gr.reshape(-1)
        assert np.linalg.norm(r) > 0, k
        stats.append((g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300),
                      np.linalg.norm(g - r) / np.linalg.norm(r), np.abs(g - r).max() / np.abs(r).max(), k))
    assert len(stats) == 60 + 76
    print(f"PSPNET {dt}: worst cosines {sorted(stats)[:3]}, median rel-L2 {np.median([s[1] for s in stats]):.3e}, "
          f"worst max-rel {max(stats, key=lambda s: s[2])[2:]}")
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
    if dt != "f16":
        # one TF1 Adam step of the step's own gradient on every variable
        upd = T.AdamTF1(lr=LR).apply({k: torch.from_numpy(v).double() for k, v in weights.items()},
                                     {k: sess.store.grad(k).double().cpu().view(weights[k].shape) for k in weights})
        for k in weights:
            got, ref = sess.variable_value(k), upd[k].numpy()
            assert np.abs(got - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), k


def test_pspnet50_full_size_step_and_pyramid_head(dev):
    torch.set_num_threads(16)
    N, H, W = 1, 160, 576
    tdt = torch.bfloat16
    image, labels, pred, logits, loss = build(H, W, PYRAMID_WINDOWS)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(53)
    img, lab = batch(N, H, W, 54)
    sess = session("bf16", weights)
    out_loss, _ = sess.run([loss, train], feed_dict={image: img, labels: lab})
    torch.cuda.synchronize()
    assert np.isfinite(float(out_loss)), out_loss
    assert all(bool(torch.isfinite(sess.store.grad(k)).all()) for k in weights)
    plan = list(sess.plans.values())[-1]
    enc_node = next(n for n in plan.nodes if n.kind == "conv" and n.w.var_name == "encoder_output/weights")
    assert plan.shapes[id(enc_node.output)] == (N, 5, 18, 512)
    enc = plan.buf[id(enc_node.output)][..., :512].double().cpu()
    assert enc.abs().max().item() > 0
    pools = [n for n in plan.nodes if n.kind == "Pool2D" and n.desc.kind == ops.POOL_AVG]
    convs = {n.w.var_name: n for n in plan.nodes if n.kind == "conv"}
    bns = {id(n.inputs[0]): n for n in plan.nodes if n.kind == "bn"}
    resizes = {id(n.inputs[0]): n for n in plan.nodes if n.kind == "ResizeBilinear"}
    assert [tuple(plan.shapes[id(n.output)][1:3]) for n in pools] == [(1, 1), (1, 2), (2, 3), (5, 6)]
    for tag, k, pool in zip(POOL_TAGS, PYRAMID_WINDOWS, pools):
        assert pool.inputs[0] is enc_node.output
        got_pool = plan.buf[id(pool.output)].double().cpu()
        assert_close(got_pool, pool_ref.avg_pool(enc, k, k, "VALID"), tdt, f"{tag} {k} average pool")
        c = convs[f"conv5_3_{tag}_conv/weights"]
        assert c.inputs[0] is pool.output
        b = bns[id(c.output)]
        assert b.relu
        w = torch.from_numpy(weights[c.w.var_name]).to(tdt).double()
        y = T.conv2d(got_pool, w, 1, "SAME")
        assert_close(plan.buf[id(c.output)][..., :128].double().cpu(), y, tdt, f"{tag} 1x1 conv")
        z = T.relu(T.batch_norm_frozen(plan.buf[id(c.output)][..., :128].double().cpu(),
                                       torch.from_numpy(weights[b.gamma.var_name]).double(),
                                       torch.from_numpy(weights[b.beta.var_name]).double()))
        got_bn = plan.buf[id(b.output)][..., :128].double().cpu()
        assert_close(got_bn, z, tdt, f"{tag} BN + ReLU")
        r = resizes[id(b.output)]
        assert_close(plan.buf[id(r.output)][..., :128].double().cpu(), T.resize_bilinear(got_bn, (H, W)), tdt,
                     f"{tag} resize {tuple(got_bn.shape[1:3])} -> {(H, W)}")
    # the encoder map's own resize, on a channel range (the CPU side stays small)
    r = resizes[id(enc_node.output)]
    assert_close(plan.buf[id(r.output)][..., 64:128].double().cpu(), T.resize_bilinear(enc[..., 64:128], (H, W)), tdt,
                 "encoder_output resize 5x18 -> 160x576")
    cat = next(n for n in plan.nodes if n.kind == "ConcatV2")
    assert plan.shapes[id(cat.output)] == (N, H, W, 1024)
