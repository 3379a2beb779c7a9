"""FC-DenseNet + TransNet on the Session compiler, host logic only (no GPU): the
C-ABI is replaced by the recording stub of tests/test_lidcamnet_dryrun.py (here
also keeping each launch's arguments), so the checkpoint variable names, the
TransNet maps at 1 x 160 x 576, the launch census of one training step, the
weighted three-head loss and the graph operators behind them can be checked on
the CPU.  Numerics: tests/test_gpu_fcdensenet_transnet.py,
tests/test_gpu_transnet_kernels.py."""
import os

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import session as S
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.fcdensenet_transnet import (LOSS_WEIGHTS, DenseBlock, FCDenseNet, TransNet,
                                                                     training_loss)
from tests.test_lidcamnet_dryrun import _Rec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcdensenet_transnet_variables.txt")
N, H, W, CLASSES = 1, 160, 576, 2
XENT = ("seg_softmax_xent_fwd_bwd", "seg_softmax_xent_soft_fwd_bwd")
NEW = ("seg_film_fwd", "seg_film_bwd", "seg_axpy_relu_fwd", "seg_axpy_relu_bwd")


class _ArgRec(_Rec):
    def __init__(self, real):
        super().__init__(real)
        self.args = []         # (symbol, arguments) of every recorded launch

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def call(*a):
            before = len(self.calls)
            r = fn(*a)
            if len(self.calls) > before:
                self.args.append((name, a))
            return r
        return call


@pytest.fixture
def dry(monkeypatch):
    rec = _ArgRec(_lib.load())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return rec


def _model():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 3], name="input_image")
    adi = tf.placeholder(tf.float32, [None, H, W, 1], name="input_adi")
    labels = tf.placeholder(tf.uint8, [None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    pred, logits, lid_logits, aux_logits = FCDenseNet(image, adi, keep, CLASSES)
    loss, total = training_loss(logits, lid_logits, aux_logits, labels)
    feed = {image: np.zeros((N, H, W, 3), np.float32), adi: np.zeros((N, H, W, 1), np.float32),
            labels: np.zeros((N, H, W), np.uint8), keep: 0.8}
    return (pred, logits, lid_logits, aux_logits), loss, total, feed


def _golden():
    with open(GOLDEN) as f:
        rows = [line.split() for line in f.read().splitlines() if line]
    return [(name, tuple(int(v) for v in shape.split(","))) for name, shape in rows]


def _session():
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    return sess


def _xent_scales(rec):
    return [a[9] for name, a in rec.args if name in XENT]


def test_variable_names_and_shapes_follow_tf():
    _model()
    want = _golden()
    assert [(v.var_name, tuple(v.shape)) for v in tf.global_variables()] == want
    names = [n for n, _ in want]
    assert names[:2] == ["dense_init_img/weights", "dense_init_lid/weights"] and want[1][1] == (3, 3, 1, 48)
    assert "denseblock1_imgbottleneck_layer_2_conv1/weights" in names        # a block of 4 has layers 0..2
    assert "denseblock1_imgbottleneck_layer_3_conv1/weights" not in names
    assert not any(n.startswith("denseblock6") or n.endswith("/biases") for n in names)
    shapes = dict(want)
    assert [shapes[f"transition_up{i}/weights"][3] for i in range(1, 6)] == [143, 572, 440, 304, 224]
    assert shapes["trans4_alpha/weights"] == (1, 1, 286, 143) and shapes["trans4_fuse/weights"] == (3, 3, 143, 143)
    anon = [n for n in names if n.startswith("batch_normalization") and n.endswith("/gamma")]
    assert anon[0] == "batch_normalization/gamma" and anon[-1] == f"batch_normalization_{len(anon) - 1}/gamma"


def test_transnet_is_importable_on_its_own_and_denseblock_is_this_files():
    G.reset_default_graph()
    a = tf.placeholder(tf.float32, [None, 6, 8, 16])
    b = tf.placeholder(tf.float32, [None, 6, 8, 16])
    y = TransNet(a, b, 16, name="t")
    assert y.op.type == "Relu" and y.shape == a.shape
    assert [v.var_name for v in tf.global_variables()] == ["t_alpha/weights", "t_beta/weights", "t_lid_feat/weights",
                                                           "t_fuse/weights"]
    types = [op.type for op in G.get_default_graph().ops]
    assert types.count("AddScalar") == 1 and types.count("MulFull") == 1 and types.count("ScalarMul") == 1
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 6, 8, 48])
    assert DenseBlock(x, 4, 16, 0.8, "d").shape[3] == 48 + 3 * 16


def test_transnet_maps_at_160x576(dry):
    outs, loss, total, feed = _model()
    sess = _session()
    sess.run(list(outs), feed_dict=feed)
    plan, = sess.plans.values()
    maps = [(40, 144, 56), (20, 72, 76), (10, 36, 110), (5, 18, 143)]
    for kind in ("film", "axpy"):
        nodes = [n for n in plan.nodes if n.kind == kind]
        assert [plan.shapes[id(n.output)] for n in nodes] == [(N, h, w, c) for h, w, c in maps]
        assert all(n.relu for n in nodes)
        # the kernels see C = 56 / 80 / 112 / 144
        assert [plan.buf[id(n.inputs[0])].shape[3] for n in nodes] == [56, 80, 112, 144]
    assert all(n.alpha_bias == 1.0 for n in plan.nodes if n.kind == "film")
    assert all(n.lam == 0.1 for n in plan.nodes if n.kind == "axpy")
    assert not any(n.kind in ("AddScalar", "MulFull", "ScalarMul") for n in plan.nodes)
    for t, c in zip(outs[1:], (CLASSES,) * 3):
        assert plan.shapes[id(t)] == (N, H, W, c)
    # the auxiliary heads resize before their 1x1 conv: the convs run at full resolution on 143 / 110 channels
    convs = {n.w.var_name.split("/")[0]: n for n in plan.nodes if n.kind == "conv"}
    assert (convs["lid_aux_loss"].desc.H, convs["lid_aux_loss"].desc.c_valid) == (H, 143)
    assert (convs["aux_classifier"].desc.H, convs["aux_classifier"].desc.c_valid) == (H, 110)
    assert (convs["dense_init_lid"].desc.c_valid, convs["dense_init_lid"].desc.C) == (1, 8)
    assert all(convs[f"trans{i}_{w}"].padding == "VALID" for i in range(1, 5) for w in ("alpha", "beta", "lid_feat"))


def _step(dry, sess, fetches, feed):
    sess.run(fetches, feed_dict=feed)          # the first run of a plan also packs the filters
    dry.calls.clear()
    dry.args.clear()
    sess.run(fetches, feed_dict=feed)
    return list(dry.calls), _xent_scales(dry)


def test_minimize_step_census_and_loss_weights(dry):
    outs, loss, total, feed = _model()
    train = tf.train.AdamOptimizer(1e-4).minimize(total)
    sess = _session()
    calls, scales = _step(dry, sess, [train], feed)
    assert [calls.count(s) for s in NEW] == [4, 4, 4, 4]
    assert sum(calls.count(s) for s in XENT) == 3
    count = N * H * W
    assert scales == pytest.approx([w / count for w in LOSS_WEIGHTS], rel=1e-6)
    assert [s / scales[0] for s in scales] == pytest.approx([1.0, 0.4, 1.6], rel=1e-6)
    plan = sess.plans[next(iter(sess.plans))]
    assert not plan.uncovered and len(plan.adam_names) == len(tf.trainable_variables())
    heads = [n for n in plan.nodes if n.kind == "xent"]
    assert [n.weight for n in heads] == [1.0, 0.4, 1.6] and all(n.in_loss for n in heads)
    assert [n.inputs[0] for n in heads] == list(outs[1:])

    # a second loss fetched beside the step: the same launches behind the forward, the same three scales
    calls2, scales2 = _step(dry, sess, [train, loss, total], feed)
    assert scales2 == scales
    extra = ["seg_fill"] + ["seg_axpy"] * 3            # the fetched weighted sum, nothing else
    assert sorted(calls2) == sorted(calls + extra)
    bwd = lambda c: c[max(i for i, s in enumerate(c) if s in XENT) + 1:]     # noqa: E731
    assert [s for s in bwd(calls2) if s not in ("seg_fill", "seg_axpy")] == bwd(calls)
    plan2 = [p for p in sess.plans.values() if p is not plan][0]
    solo = [n for n in plan2.nodes if n.kind == "xent" and not n.in_loss]
    assert len(solo) == 1 and solo[0].twin is not None and solo[0].twin.in_loss and solo[0].twin.weight == 1.0


def test_a_forward_only_loss_on_other_logits_launches_but_gives_no_gradient(dry):
    """The main-head loss minimised, the weighted loss only fetched: four
    launches, one gradient source."""
    outs, loss, total, feed = _model()
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    sess = _session()
    calls, scales = _step(dry, sess, [train, total], feed)
    plan, = sess.plans.values()
    xs = [n for n in plan.nodes if n.kind == "xent"]
    assert [n.in_loss for n in xs] == [True, False, False, False]
    assert xs[1].twin is xs[0] and xs[2].twin is None and xs[3].twin is None
    assert sum(calls.count(s) for s in XENT) == 3
    # the TransNet blocks behind the auxiliary heads still train through the main head only
    assert calls.count("seg_film_bwd") == 4


def test_accumulate_template_builds_and_plans(dry):
    """The reference driver's own loop (FCDenseNet_TransNet.py:279-297)."""
    outs, loss, total, feed = _model()
    optimizer = tf.train.AdamOptimizer(1e-4)
    const = tf.constant(1 / 1 * 3)
    t_vars = tf.trainable_variables()
    accum = [tf.Variable(tf.zeros_like(v.initialized_value()), trainable=False) for v in t_vars]
    zero_ops = [tv.assign(tf.zeros_like(tv)) for tv in accum]
    gv = optimizer.compute_gradients(total, t_vars)
    accum_ops = [accum[i].assign_add(tf.scalar_mul(const, g[0])) for i, g in enumerate(gv)]
    train_step = optimizer.apply_gradients([(accum[i], g[1]) for i, g in enumerate(gv)])
    sess = _session()
    sess.run(zero_ops)
    dry.calls.clear()
    dry.args.clear()
    sess.run(accum_ops, feed_dict=feed)
    assert [dry.calls.count(s) for s in NEW] == [4, 4, 4, 4]
    scales = _xent_scales(dry)
    assert [s / scales[0] for s in scales] == pytest.approx([1.0, 0.4, 1.6], rel=1e-6)
    sess.run([train_step, loss], feed_dict=feed)


def test_tensor_operators_build_the_ops():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 4, 6, 8])
    y = tf.placeholder(tf.float32, [None, 4, 6, 8])
    s = tf.placeholder(tf.float32, [None, 1, 1, 8])
    assert (x + 1).op.type == (1 + x).op.type == "AddScalar" and (x + 1).op.attrs["scalar"] == 1.0
    assert (x + y).op.type == "Add"
    assert (x * y).op.type == tf.multiply(x, y).op.type == "MulFull" and (x * y).shape == x.shape
    assert (0.1 * x).op.type == (x * 0.1).op.type == "ScalarMul" and (0.1 * x).op.attrs["scalar"] == 0.1
    assert (x * s).op.type == tf.multiply(s, x).op.type == "Mul"            # the squeeze-excite gate, as before
    for bad in (tf.placeholder(tf.float32, [None, 4, 6, 16]), tf.placeholder(tf.float32, [None, 4, 3, 8]), x):
        with pytest.raises(NotImplementedError):
            x * bad


def test_the_new_ops_outside_their_chains_are_refused(dry):
    def run(build):
        G.reset_default_graph()
        x = tf.placeholder(tf.float32, [None, 4, 6, 8])
        y = tf.placeholder(tf.float32, [None, 4, 6, 8])
        out = build(x, y)
        feed = {x: np.zeros((1, 4, 6, 8), np.float32), y: np.zeros((1, 4, 6, 8), np.float32)}
        sess = _session()
        sess.run([out], feed_dict=feed)
        return [n.kind for n in next(iter(sess.plans.values())).nodes]

    for build in (lambda x, y: x * y, lambda x, y: x + 1, lambda x, y: 0.5 * x, lambda x, y: (x + 1) * y,
                  lambda x, y: tf.nn.relu(x * y + x), lambda x, y: 0.5 * x + 0.5 * y):
        with pytest.raises(NotImplementedError, match="hot path"):
            run(build)
    assert run(lambda x, y: tf.nn.relu((x + 1) * y + x)) == ["input", "input", "film"]
    assert run(lambda x, y: (x + 0) * y + x) == ["input", "input", "film"]
    assert run(lambda x, y: tf.nn.relu(x + 0.1 * y)) == ["input", "input", "axpy"]
    assert run(lambda x, y: 2 * y + x) == ["input", "input", "axpy"]
    # a plain tf.add followed by a ReLU lowers as before (PSPNet's residual sums)
    assert run(lambda x, y: tf.nn.relu(tf.add(x, y))) == ["input", "input", "Add", "Relu"]


def test_loss_forms(dry):
    def build(weights_tree):
        G.reset_default_graph()
        lg = [tf.placeholder(tf.float32, [None, 4, 6, 2]) for _ in range(3)]
        lab = tf.placeholder(tf.uint8, [None, 4, 6])
        xe = [tf.nn.softmax_cross_entropy_with_logits(logits=t, labels=lab) for t in lg]
        loss = tf.reduce_mean(weights_tree(xe))
        feed = {t: np.zeros((1, 4, 6, 2), np.float32) for t in lg}
        feed[lab] = np.zeros((1, 4, 6), np.uint8)
        sess = _session()
        sess.run([loss], feed_dict=feed)
        plan, = sess.plans.values()
        return [n.weight for n in plan.nodes if n.kind == "xent"], [n.kind for n in plan.nodes]

    assert build(lambda xe: xe[0])[0] == [1.0]
    assert "xent_sum" not in build(lambda xe: xe[0])[1]                       # the bare form is the node it was
    assert build(lambda xe: xe[0] + (0.4 * xe[1] + 1.6 * xe[2]))[0] == [1.0, 0.4, 1.6]      # nested the other way
    assert build(lambda xe: 2 * (xe[0] + 0.5 * xe[1]))[0] == [2.0, 1.0]
    with pytest.raises(NotImplementedError, match="reduce_mean"):
        build(lambda xe: tf.nn.relu(xe[0]))
    with pytest.raises(NotImplementedError, match="reduce_mean"):
        build(lambda xe: xe[0] + 1)


def test_heads_of_a_weighted_loss_share_their_shape(dry):
    G.reset_default_graph()
    a = tf.placeholder(tf.float32, [None, 4, 6, 2])
    b = tf.placeholder(tf.float32, [None, 4, 6, 2])
    lab = tf.placeholder(tf.uint8, [None, 4, 6])
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=a, labels=lab, valid_hw=(3, 5))
                          + 0.4 * tf.nn.softmax_cross_entropy_with_logits(logits=b, labels=lab))
    feed = {a: np.zeros((1, 4, 6, 2), np.float32), b: np.zeros((1, 4, 6, 2), np.float32),
            lab: np.zeros((1, 4, 6), np.uint8)}
    with pytest.raises(ValueError, match="share"):
        _session().run([loss], feed_dict=feed)
