"""The op forms PSPNet50 adds to the Session, each in a small trained graph
against oracle.tf1_ops autograd at the op suite's per-dtype tolerances
(tests/gpu_utils.py):

* a 1x1 conv with stride 2 and 3 (Network/model/PSPNet.py:57, :60 ...), which
  the planner lowers to a subsample + the stride-1 conv: logits, filter
  gradient and the input gradient scattered back into the full map;
* the 7x7 stride-2 VALID stem after Zero_Padding(3) (:30-31): forward and
  filter gradient;
* the pyramid's align_corners resizes from 1x2, 2x3 and 1x1 to the input size
  (:151-170): forward and gradient."""
import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import ops, tf
from semanticsegmentation_tensorflow_amd.layers import Conv2D_Block, Zero_Padding
from tests import pool_ref
from tests.gpu_utils import assert_close, rnd

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CLASSES = 8


def _quant(tdt):
    class _Q(torch.autograd.Function):        # storage rounding, straight-through gradient
        @staticmethod
        def forward(ctx, t):
            return t.to(tdt).double()

        @staticmethod
        def backward(ctx, g):
            return g
    return _Q.apply


def _weights(seed, tdt):
    """1/sqrt(fan_in) filters already on the compute dtype's grid (the packed copy is then exact)."""
    rng = np.random.default_rng(seed)
    out = {}
    for v in tf.trainable_variables():
        R, S, A, B = v.shape
        w = torch.from_numpy(rng.standard_normal((R, S, A, B)) / np.sqrt(R * S * A))
        out[v.var_name] = rnd(w, tdt).numpy().astype(np.float32)
    return out


def _session(dt, weights):
    sess = tf.Session(compute_dtype=dt)
    sess.store_fused_grads = True
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    return sess


def _labels(shape, classes, seed):
    return np.random.default_rng(seed).integers(0, classes, shape).astype(np.uint8)


@pytest.mark.parametrize("dt", list(TDT))
@pytest.mark.parametrize("padding", ["VALID", "SAME"])
@pytest.mark.parametrize("stride", [2, 3])
def test_strided_1x1_conv_in_a_trained_graph(dev, stride, padding, dt):
    N, H, W, C, K = 2, 9, 11, 16, 32
    tdt = TDT[dt]
    q = _quant(tdt)
    OH, OW = -(-H // stride), -(-W // stride)
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, C], name="input_image")
    labels = tf.placeholder(tf.uint8, [None, OH, OW], name="annotation")
    pre = Conv2D_Block(image, C, 1, 1, 1, "VALID", name="pre")
    logits = Conv2D_Block(pre, K, 1, 1, stride, padding, name="strided")
    sibling = Conv2D_Block(pre, K, 1, 1, stride, padding, name="sibling")       # shares the compact copy
    total = tf.add(logits, sibling)
    assert tuple(total.shape) == (None, OH, OW, K)
    head = Conv2D_Block(total, CLASSES, 1, 1, 1, "VALID", name="head")          # the loss kernel takes <= 16 classes
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=head, labels=labels))
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    weights = _weights(5 + stride, tdt)
    x = rnd(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(stride), dtype=torch.float64), tdt)
    lab = _labels((N, OH, OW), CLASSES, 9)
    sess = _session(dt, weights)
    out, out_head, _ = sess.run([total, head, train], feed_dict={image: x.numpy().astype(np.float32), labels: lab})
    torch.cuda.synchronize()
    plan = list(sess.plans.values())[-1]
    scale = sess.loss_scale if dt == "f16" else 1.0
    # the plan: one shared subsample, both convs at stride 1 on it, no strided input gradient
    subs = [n for n in plan.nodes if n.kind == "Subsample"]
    assert len(subs) == 1 and subs[0].stride == stride and plan.shapes[id(subs[0].output)] == (N, OH, OW, C)
    convs = {n.w.var_name: n for n in plan.nodes if n.kind == "conv"}
    for nm in ("strided/weights", "sibling/weights"):
        assert convs[nm].inputs[0] is subs[0].output and convs[nm].desc.stride_h == 1 and convs[nm].desc.H == OH
    # float64 reference, rounded where the device stores
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in weights.items()}
    a = q(T.conv2d(x, p["pre/weights"], 1, "VALID"))
    a.retain_grad()
    r_total = q(q(T.conv2d(a, p["strided/weights"], stride, padding)) + q(T.conv2d(a, p["sibling/weights"], stride, padding)))
    assert r_total.shape == (N, OH, OW, K)
    r_head = q(T.conv2d(r_total, p["head/weights"], 1, "VALID"))
    T.mean_softmax_xent(r_head, T.one_hot(torch.from_numpy(lab), CLASSES)).backward()
    assert_close(torch.from_numpy(out).double(), r_total.detach(), tdt, f"strided conv outputs s{stride} {padding}")
    assert_close(torch.from_numpy(out_head).double(), r_head.detach(), tdt, f"logits s{stride} {padding}")
    for k, v in p.items():
        got = sess.store.grad(k).double().cpu().view(v.shape) / scale
        assert v.grad.abs().max().item() > 0
        assert_close(got, v.grad, tdt, f"{k} gradient s{stride} {padding}")
    # the input gradient in the full map: the sum of both convs', every skipped pixel 0
    dfull = plan.tmp[("g", id(pre))][..., :C].double().cpu() / scale
    assert_close(dfull, a.grad, tdt, f"input gradient s{stride} {padding}")
    skipped = torch.ones(H, W, dtype=torch.bool)
    skipped[::stride, ::stride] = False
    assert bool((dfull[:, skipped] == 0).all()) and bool((a.grad[:, skipped] == 0).all())
    dsub = plan.tmp[("g", id(subs[0].output))][..., :C].double().cpu() / scale
    assert torch.equal(dfull[:, ::stride, ::stride], dsub)


@pytest.mark.parametrize("dt", list(TDT))
def test_7x7_stride2_valid_stem_after_zero_padding(dev, dt):
    N, H, W, C, K = 1, 16, 24, 4, 8
    tdt = TDT[dt]
    q = _quant(tdt)
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, C], name="input_image")
    padded = Zero_Padding(image, paddings=3, name="conv1")
    logits = Conv2D_Block(padded, K, 7, 7, 2, "VALID", True, name="conv1")        # dilation=True: PSPNet.py:31
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    assert tuple(logits.shape) == (None, OH, OW, K) == (None, 8, 12, K)
    labels = tf.placeholder(tf.uint8, [None, OH, OW], name="annotation")
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    weights = _weights(21, tdt)
    x = rnd(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(22), dtype=torch.float64), tdt)
    lab = _labels((N, OH, OW), K, 23)
    sess = _session(dt, weights)
    out, _ = sess.run([logits, train], feed_dict={image: x.numpy().astype(np.float32), labels: lab})
    torch.cuda.synchronize()
    scale = sess.loss_scale if dt == "f16" else 1.0
    plan = list(sess.plans.values())[-1]
    pad_node, = [n for n in plan.nodes if n.kind == "Pad"]
    got_pad = plan.buf[id(pad_node.output)][..., :C].double().cpu()
    assert torch.equal(got_pad, pool_ref.pad(x, (3, 3, 3, 3)))
    w = torch.from_numpy(weights["conv1/weights"]).double().requires_grad_(True)
    r = q(T.conv2d(pool_ref.pad_ad(x, (3, 3, 3, 3)), w, 2, "VALID"))
    T.mean_softmax_xent(r, T.one_hot(torch.from_numpy(lab), K)).backward()
    assert_close(torch.from_numpy(out).double(), r.detach(), tdt, "7x7 / 2 VALID forward")
    got = sess.store.grad("conv1/weights").double().cpu().view(w.shape) / scale
    assert_close(got, w.grad, tdt, "7x7 / 2 VALID filter gradient")


@pytest.mark.parametrize("dt", list(TDT))
@pytest.mark.parametrize("src", [(1, 2), (2, 3), (1, 1)])
def test_resize_from_the_pyramid_maps(dev, src, dt):
    """The kernels, and for 1x1 the broadcast / spatial sum the Session takes."""
    N, C, OH, OW = 2, 8, 16, 24
    h, w = src
    tdt = TDT[dt]
    g = torch.Generator().manual_seed(31 + h * 3 + w)
    x = rnd(torch.randn(N, h, w, C, generator=g, dtype=torch.float64), tdt).requires_grad_(True)
    dy = rnd(torch.randn(N, OH, OW, C, generator=g, dtype=torch.float64), tdt)
    y = T.resize_bilinear(x, (OH, OW))
    (y * dy).sum().backward()
    xd, dyd = x.detach().to(tdt).to(dev), dy.to(tdt).to(dev)
    yd = torch.full((N, OH, OW, C), float("nan"), dtype=tdt, device=dev)
    dxd = torch.full((N, h, w, C), float("nan"), dtype=torch.float32, device=dev)
    ops.resize_bilinear_fwd(xd, yd)
    ops.resize_bilinear_bwd(dyd, dxd)
    torch.cuda.synchronize()
    assert_close(yd.double().cpu(), y.detach(), tdt, f"resize {src} forward")
    assert_close(dxd.double().cpu(), x.grad, torch.float32, f"resize {src} gradient", 1e-5 if dt == "f32" else None)
    if src == (1, 1):
        yb = torch.full((N, OH, OW, C), float("nan"), dtype=tdt, device=dev)
        dxb = torch.full((N, 1, 1, C), float("nan"), dtype=tdt, device=dev)
        ws = ops.Workspace(dev)
        ops.spatial_broadcast(xd, yb, 1.0)
        ops.spatial_reduce(dyd, dxb, 1.0, ws)
        torch.cuda.synchronize()
        assert torch.equal(yb.double().cpu(), y.detach())
        assert_close(dxb.double().cpu(), x.grad, tdt, "1x1 resize gradient as a spatial sum")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pyramid_branch_in_a_trained_graph(dev, dt):
    """avg pool (window = stride) -> 1x1 conv -> resize to the input size, the
    three non-trivial pyramid map sizes on a 2 x 3 map with channels to spare."""
    N, H, W, C, K = 1, 4, 9, 8, 8
    tdt = TDT[dt]
    q = _quant(tdt)
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, C], name="input_image")
    labels = tf.placeholder(tf.uint8, [None, H, W], name="annotation")
    enc = Conv2D_Block(image, C, 1, 1, 1, "SAME", name="enc")
    outs = []
    for i, k in enumerate(((4, 9), (2, 3), (4, 3))):              # maps 1x1, 2x3, 1x3
        pooled = tf.nn.avg_pool(enc, [1, k[0], k[1], 1], [1, k[0], k[1], 1], "VALID", name=f"p{i}")
        outs.append(tf.image.resize_bilinear(Conv2D_Block(pooled, K, 1, 1, 1, name=f"c{i}"), tf.shape(image)[1:3],
                                             align_corners=True))
    logits = tf.add(tf.add(outs[0], outs[1]), outs[2])
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    weights = _weights(41, tdt)
    x = rnd(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(42), dtype=torch.float64), tdt)
    lab = _labels((N, H, W), K, 43)
    sess = _session(dt, weights)
    out, _ = sess.run([logits, train], feed_dict={image: x.numpy().astype(np.float32), labels: lab})
    torch.cuda.synchronize()
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in weights.items()}
    e = q(T.conv2d(x, p["enc/weights"], 1, "SAME"))
    rs = []
    for i, k in enumerate(((4, 9), (2, 3), (4, 3))):
        pooled = q(pool_ref.avg_pool_ad(e, k, k, "VALID"))
        rs.append(q(T.resize_bilinear(q(T.conv2d(pooled, p[f"c{i}/weights"], 1, "SAME")), (H, W))))
    r = q(q(rs[0] + rs[1]) + rs[2])
    T.mean_softmax_xent(r, T.one_hot(torch.from_numpy(lab), K)).backward()
    assert_close(torch.from_numpy(out).double(), r.detach(), tdt, "pyramid branch logits")
    for k, v in p.items():
        got = sess.store.grad(k).double().cpu().view(v.shape)
        # bf16: dlogits and three stored gradients in a row -- the end-to-end
        # bound of the 16-bit model tests (cosine), not the single-op tolerance
        if dt == "f32":
            assert_close(got, v.grad, tdt, f"{k} gradient")
        else:
            cos = (got.reshape(-1) @ v.grad.reshape(-1)) / (got.norm() * v.grad.norm())
            assert cos.item() >= 0.95, (k, cos.item())
