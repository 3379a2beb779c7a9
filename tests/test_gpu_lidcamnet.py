"""LidCamNet (Network/model/LidCamNet.py:30-73) on the Session vs a float64
restatement built here from oracle.tf1_ops + tests/aniso_ref.py (the per-axis
dilated convs), on identical inputs and weights, in bf16 and f16.

The weights are drawn at 1/sqrt(fan_in) and assigned: the reference's
N(0, 0.01) init with no ReLU anywhere shrinks the signal of 21 layers to
~1e-10 and would prove nothing.  The BatchNorm is the reference's frozen form
(moving mean 0, variance 1); gamma ~ 1 and beta are randomised.

Criteria: the project's 16-bit end-to-end bounds, with the reference rounded
at the device's storage points -- bf16 as tests/test_gpu_fcn.py (logits 3e-2
of max, loss 1e-2, gradient cosine >= 0.95, median rel-L2 <= 0.1), f16 as
tests/test_gpu_fp16.py (1e-2, 5e-3, 0.98, 0.05); layer-local checks at the
per-dtype tolerances of tests/gpu_utils.py."""
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import ops, tf
from semanticsegmentation_tensorflow_amd.lidcamnet import CONTEXT_DILATIONS, LidCamNet
from tests import aniso_ref
from tests.gpu_utils import assert_close
from tests.test_gpu_ops import _np_uniform

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
# logits max-rel, loss rel, min gradient cosine, median gradient rel-L2
BOUNDS = {"bf16": (3e-2, 1e-2, 0.95, 0.1), "f16": (1e-2, 5e-3, 0.98, 0.05)}
LR = 1e-4


def bn_name(i):
    return "batch_normalization" if i == 1 else f"batch_normalization_{i - 1}"


def build(H, W):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 4], name="input_image")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    pred, logits = LidCamNet(image, keep, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    return image, labels, keep, pred, logits, loss


def make_weights(seed):
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        s = tuple(v.shape)
        if len(s) == 4:
            R, S_, A, B = s
            tconv = v.var_name.split("/")[0] in ("conv15", "conv17", "conv19")
            fan = (R // 2) * (S_ // 2) * B if tconv else R * S_ * A
            out[v.var_name] = (rng.standard_normal(s) / math.sqrt(fan)).astype(np.float32)
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


def reference(p, x, q, kp=1.0, masks=None):
    """float64 LidCamNet; q rounds a stored activation through the compute
    dtype; masks: the nine dropout masks (conv6 ... conv14) when kp < 1."""
    def bn(h, i):
        return q(T.batch_norm_frozen(h, p[bn_name(i) + "/gamma"], p[bn_name(i) + "/beta"]))

    def conv(h, i, stride=1, pad="SAME", dil=(1, 1), norm=True):
        y = q(aniso_ref.conv2d(h, p[f"conv{i}/weights"], stride, pad, dil))
        return bn(y, i) if norm else y

    def tconv(h, i, like):
        w = p[f"conv{i}/weights"]
        return bn(q(T.conv2d_transpose(h, w, (h.shape[0], like.shape[1], like.shape[2], w.shape[2]), 2, "SAME")), i)

    def drop(h, j):
        return h if masks is None else q(h / kp * masks[j])

    c1 = conv(x, 1, 2)
    c2 = conv(c1, 2)
    c3 = conv(c2, 3, 2)
    c4 = conv(c3, 4)
    h = conv(c4, 5, 2)
    j = 0
    for i in (6, 7):
        h = drop(conv(h, i), j)
        j += 1
    for i, d in enumerate(CONTEXT_DILATIONS):
        h = drop(conv(h, 8 + i, dil=(d[1], d[2])), j)
        j += 1
    h = drop(conv(h, 13), j)
    h = drop(conv(h, 14, pad="VALID"), j + 1)
    h = conv(tconv(h, 15, c4), 16)
    h = conv(tconv(h, 17, c2), 18)
    h = conv(tconv(h, 19, x), 20)
    return conv(h, 21, norm=False)


def oracle_step(weights, img, lab, dtype, kp=1.0, masks=None):
    tdt = TDT[dtype]

    class _Q(torch.autograd.Function):        # storage rounding, straight-through gradient
        @staticmethod
        def forward(ctx, t):
            return t.to(tdt).double()

        @staticmethod
        def backward(ctx, g):
            return g
    p = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    p = {k: (v.to(tdt).double() if v.dim() == 4 else v).requires_grad_(True) for k, v in p.items()}
    logits = reference(p, _Q.apply(torch.from_numpy(img).double()), _Q.apply, kp, masks)
    loss = T.mean_softmax_xent(logits, T.one_hot(torch.from_numpy(lab), 2))
    loss.backward()
    return logits.detach().numpy(), loss.item(), {k: v.grad.numpy() for k, v in p.items()}


def session(dtype, weights, seed=0):
    sess = tf.Session(compute_dtype=dtype, seed=seed)
    sess.store_fused_grads = True
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    return sess


def check_step(sess, dtype, out_logits, out_loss, r_logits, r_loss, r_grads, scale, what):
    tl = BOUNDS[dtype]
    e_log = np.abs(out_logits - r_logits).max() / np.abs(r_logits).max()
    print(f"{what} {dtype}: logits max-rel {e_log:.3e}, loss {float(out_loss):.6f} vs {r_loss:.6f}")
    assert np.abs(r_logits).max() > 0.1                  # the signal survives 21 layers
    assert e_log < tl[0], f"{what}: logits rel err {e_log:.3e}"
    assert abs(float(out_loss) - r_loss) <= tl[1] * max(1.0, abs(r_loss)), (what, out_loss, r_loss)
    stats = []
    for k, gr in r_grads.items():
        g = sess.store.grad(k).cpu().numpy().reshape(-1).astype(np.float64) / scale
        r = gr.reshape(-1)
        assert np.linalg.norm(r) > 0, k
        cos = g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300)
        stats.append((cos, np.linalg.norm(g - r) / np.linalg.norm(r), k))
    print(f"{what} {dtype}: worst cosines {sorted(stats)[:3]}, median rel-L2 {np.median([s[1] for s in stats]):.3e}")
    assert len(stats) == 21 + 40
    assert min(s[0] for s in stats) >= tl[2], sorted(stats)[:3]
    assert np.median([s[1] for s in stats]) <= tl[3]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_lidcamnet_logits_loss_grads(dev, dtype):
    torch.set_num_threads(16)
    N, H, W = 2, 48, 96                                   # context map 6 x 12
    image, labels, keep, pred, logits, loss = build(H, W)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(31)
    img, lab = batch(N, H, W, 32)
    sess = session(dtype, weights)
    scale = sess.loss_scale if dtype == "f16" else 1.0
    out_logits, out_loss, _ = sess.run([logits, loss, train], feed_dict={image: img, labels: lab, keep: 1.0})
    torch.cuda.synchronize()
    plan = list(sess.plans.values())[-1]
    convs = {n.w.var_name: n for n in plan.nodes if n.kind == "conv"}
    assert [(convs[f"conv{i}/weights"].desc.dil_h, convs[f"conv{i}/weights"].desc.dil_w) for i in range(8, 13)] == \
        [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32)]
    r_logits, r_loss, r_grads = oracle_step(weights, img, lab, dtype)
    check_step(sess, dtype, out_logits, out_loss, r_logits, r_loss, r_grads, scale, "keep_prob 1.0")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_lidcamnet_dropout_masks_redrawn_on_the_host(dev, dtype):
    torch.set_num_threads(16)
    N, H, W, kp = 2, 48, 96, 0.8
    image, labels, keep, pred, logits, loss = build(H, W)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(33)
    img, lab = batch(N, H, W, 34)
    sess = session(dtype, weights, seed=5)
    scale = sess.loss_scale if dtype == "f16" else 1.0
    out_logits, out_loss, _ = sess.run([logits, loss, train], feed_dict={image: img, labels: lab, keep: kp})
    torch.cuda.synchronize()
    plan = list(sess.plans.values())[-1]
    drops = [n for n in plan.nodes if n.kind == "Dropout"]
    assert len(drops) == 9 and all(n.kp_val == np.float32(kp) or abs(n.kp_val - kp) < 1e-6 for n in drops)
    P, C = N * (H // 8) * (W // 8), 128                   # flat counter p * C + c of the dropout pass
    masks = []
    for n in drops:
        u = np.array([_np_uniform(n.seed_val, i) for i in range(P * C)], np.float32)
        m = np.floor(np.float32(kp) + u).astype(np.float64).reshape(N, H // 8, W // 8, C)
        assert 0.7 < m.mean() < 0.9
        masks.append(torch.from_numpy(m))
    r_logits, r_loss, r_grads = oracle_step(weights, img, lab, dtype, kp, masks)
    check_step(sess, dtype, out_logits, out_loss, r_logits, r_loss, r_grads, scale, f"keep_prob {kp}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_lidcamnet_accumulate_template_is_adam_on_its_own_gradient(dev, dtype):
    """The reference driver's step (Network/model/LidCamNet.py:106-125) with
    B = 2: two accumulations of 1.5 g, then TF1 Adam on the accumulators."""
    N, H, W, B = 2, 48, 96, 2
    image, labels, keep, pred, logits, loss = build(H, W)
    opt = tf.train.AdamOptimizer(LR)
    const = tf.constant(1 / B * 3)
    t_vars = tf.trainable_variables()
    accum = [tf.Variable(tf.zeros_like(t.initialized_value()), trainable=False) for t in t_vars]
    zero_ops = [a.assign(tf.zeros_like(a)) for a in accum]
    gvs = opt.compute_gradients(loss, t_vars)
    accum_ops = [accum[i].assign_add(tf.scalar_mul(const, gv[0])) for i, gv in enumerate(gvs)]
    train_step = opt.apply_gradients([(accum[i], gv[1]) for i, gv in enumerate(gvs)])
    weights = make_weights(35)
    img, lab = batch(N, H, W, 36)
    feed = {image: img, labels: lab, keep: 1.0}
    sess = session(dtype, weights)
    sess.run(zero_ops)
    for _ in range(B):
        sess.run(accum_ops, feed_dict=feed)
    acc = {t.var_name: sess.store.aux[a.var_name].cpu().numpy().astype(np.float64) for t, a in zip(t_vars, accum)}
    sess.run(train_step, feed_dict=feed)
    assert sess.store.step == 1
    # the accumulators hold 3 g: against the float64 gradient at the project's bounds
    _, _, r_grads = oracle_step(weights, img, lab, dtype)
    tl = BOUNDS[dtype]
    stats = []
    for k, gr in r_grads.items():
        g, r = acc[k].reshape(-1), 3.0 * gr.reshape(-1)
        stats.append((g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-300),
                      np.linalg.norm(g - r) / np.linalg.norm(r), k))
    assert min(s[0] for s in stats) >= tl[2], sorted(stats)[:3]
    assert np.median([s[1] for s in stats]) <= tl[3]
    # and the update is float64 TF1 Adam of the step's own (accumulated) gradient
    upd = T.AdamTF1(lr=LR).apply({k: torch.from_numpy(v).double() for k, v in weights.items()},
                                 {k: torch.from_numpy(acc[k]).double().view(weights[k].shape) for k in weights})
    for k in weights:
        got, ref = sess.variable_value(k), upd[k].numpy()
        assert np.abs(got - ref).max() <= 1e-6 + 1e-5 * np.abs(ref).max(), k


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_lidcamnet_full_size_layer_local(dev, dtype):
    """One step at the shape users run, 1 x 160 x 576 x 4: the five per-axis
    dilated convs (forward) and the two strided input gradients, each against
    float64 on the buffers its own launch read."""
    torch.set_num_threads(16)
    N, H, W = 1, 160, 576
    tdt = TDT[dtype]
    image, labels, keep, pred, logits, loss = build(H, W)
    train = tf.train.AdamOptimizer(LR).minimize(loss)
    weights = make_weights(37)
    img, lab = batch(N, H, W, 38)
    sess = session(dtype, weights)
    sess.capture = []
    sess.run([loss, train], feed_dict={image: img, labels: lab, keep: 1.0})
    torch.cuda.synchronize()
    rec = {r["name"]: r for r in sess.capture if r["kind"] == "conv"}
    sess.capture = None
    wq = {k: torch.from_numpy(v).to(tdt).double() for k, v in weights.items() if v.ndim == 4}
    for i, d in enumerate(CONTEXT_DILATIONS):
        r = rec[f"conv{8 + i}/weights"]
        assert (r["desc"].dil_h, r["desc"].dil_w) == (d[1], d[2]) and r["dilation_hw"] == (d[1], d[2])
        assert tuple(r["x"].shape) == (N, 20, 72, 128)
        ref = aniso_ref.conv2d(r["x"].double().cpu(), wq[r["name"]], 1, "SAME", (d[1], d[2]))
        fam = ops.conv_kernel_info(r["desc"], ops.OP_FWD)[0]
        assert ref.abs().max().item() > 0
        assert_close(r["y"][..., :128].double().cpu(), ref, tdt, f"conv{8 + i} fwd {d} on {fam}")
    for name, (h, w, c, k) in (("conv3/weights", (80, 288, 32, 64)), ("conv5/weights", (40, 144, 64, 128))):
        r = rec[name]
        assert r["stride"] == 2 and ops.conv2d_bwd_data_s2_ok(r["desc"])
        fam = ops.conv_kernel_info(r["desc"], ops.OP_BWD_DATA)[0]
        assert fam.startswith("dgrad_s2<"), fam
        assert tuple(r["dx"].shape) == (N, h, w, c)
        x = torch.zeros(N, h, w, c, dtype=torch.float64, requires_grad=True)
        dz = r["dz"][..., :k].double().cpu()
        (T.conv2d(x, wq[name], 2, "SAME", 1) * dz).sum().backward()
        assert x.grad.abs().max().item() > 0
        assert_close(r["dx"].double().cpu(), x.grad, tdt, f"{name} strided dgrad on {fam}")
