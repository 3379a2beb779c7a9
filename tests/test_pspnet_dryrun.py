"""PSPNet50 on the Session compiler, host logic only (no GPU): the C-ABI is
replaced by the recording stub of tests/test_lidcamnet_dryrun.py (with the
pooling descriptor's host-only init let through), so the stage shapes at
1 x 160 x 576 x 4, the launch census of one training step -- the pool and pad
launches, and no strided input gradient -- and the checkpoint variable names
can be checked on the CPU.  Numerics: tests/test_gpu_pspnet.py."""
import os

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import session as S
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.pspnet import PYRAMID_WINDOWS, PSPNet50, build_train_graph
from tests.test_lidcamnet_dryrun import _Rec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pspnet50_variables.txt")
N, H, W = 1, 160, 576


class _PoolRec(_Rec):
    """The LidCamNet dry run's recorder; seg_pool_desc_init is host-only
    arithmetic and runs for real, and the pool descriptors are recorded too."""

    def __init__(self, real):
        super().__init__(real)
        self.pools = []        # (symbol, copy of the seg_pool_desc) of every recorded pool launch

    def __getattr__(self, name):
        if name == "seg_pool_desc_init":
            return getattr(self.real, name)
        fn = super().__getattr__(name)
        if name not in ("seg_pool2d_fwd", "seg_pool2d_bwd"):
            return fn

        def pool(*a):
            self.pools.append((name, _lib.SegPoolDesc.from_buffer_copy(a[0]._obj)))
            return fn(*a)
        return pool


@pytest.fixture
def dry(monkeypatch):
    rec = _PoolRec(_lib.load())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return rec


def _model():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 4], name="input_image")
    labels = tf.placeholder(tf.uint8, [None, H, W], name="annotation")
    pred, logits = PSPNet50(image, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    feed = {image: np.zeros((N, H, W, 4), np.float32), labels: np.zeros((N, H, W), np.uint8)}
    return pred, logits, loss, feed


def test_default_windows_are_the_reference_constants():
    assert PYRAMID_WINDOWS == ((5, 18), (3, 9), (2, 6), (1, 3))


def test_stage_shapes_at_160x576(dry):
    pred, logits, loss, feed = _model()
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    sess.run([logits, pred], feed_dict=feed)
    plan, = sess.plans.values()
    convs = {n.w.var_name.split("/")[0]: n for n in plan.nodes if n.kind == "conv"}

    def out_hw(name):
        return tuple(plan.shapes[id(convs[name].output)][1:3])
    assert out_hw("conv1") == (80, 288)
    pool1 = next(n for n in plan.nodes if n.kind == "Pool2D" and n.ops[0].name == "pool1")
    assert plan.shapes[id(pool1.inputs[0])] == (N, 82, 290, 64) and plan.shapes[id(pool1.output)] == (N, 40, 144, 64)
    assert out_hw("conv2_3_3") == (40, 144) and out_hw("conv3_1") == (20, 72) and out_hw("shortcut2") == (20, 72)
    assert out_hw("conv3_4_3") == (20, 72) and out_hw("conv4_1_1") == (10, 36) and out_hw("conv4_6_3") == (10, 36)
    assert out_hw("conv5_1_1") == (5, 18) and out_hw("shortcut4") == (5, 18)
    assert plan.shapes[id(convs["encoder_output"].output)] == (N, 5, 18, 512)
    pools = [n for n in plan.nodes if n.kind == "Pool2D" and n is not pool1]
    assert [tuple(plan.shapes[id(n.output)][1:]) for n in pools] == [(1, 1, 512), (1, 2, 512), (2, 3, 512), (5, 6, 512)]
    assert [(n.desc.kh, n.desc.kw, n.desc.sh, n.desc.sw, n.desc.kind) for n in pools] == \
        [(kh, kw, kh, kw, ops.POOL_AVG) for kh, kw in PYRAMID_WINDOWS]
    cat, = [n for n in plan.nodes if n.kind == "ConcatV2"]
    assert plan.shapes[id(cat.output)] == (N, 160, 576, 1024)
    assert [plan.shapes[id(t)][3] for t in cat.inputs] == [512, 128, 128, 128, 128]
    assert plan.shapes[id(logits)] == (N, 160, 576, 2) and plan.shapes[id(pred)] == (N, 160, 576, 1)
    pads = [n for n in plan.nodes if n.kind == "Pad"]
    assert [tuple(plan.shapes[id(n.output)][1:3]) for n in pads] == [(166, 582), (82, 290)]
    # an inference plan records no switches
    assert not plan.pool_idx
    # the six strided 1x1 convs read three shared compact copies, at stride 1
    subs = [n for n in plan.nodes if n.kind == "Subsample"]
    assert [(n.stride, plan.shapes[id(n.inputs[0])][1:], plan.shapes[id(n.output)][1:]) for n in subs] == \
        [(2, (40, 144, 256), (20, 72, 256)), (2, (20, 72, 512), (10, 36, 512)), (2, (10, 36, 1024), (5, 18, 1024))]
    for a, b in (("conv3_1", "shortcut2"), ("conv4_1_1", "shortcut3"), ("conv5_1_1", "shortcut4")):
        assert convs[a].inputs[0] is convs[b].inputs[0] and convs[a].stride == convs[b].stride == 1
        assert (convs[a].desc.stride_h, convs[a].desc.H, convs[a].desc.OH) == (1, convs[a].desc.OH, convs[a].desc.OH)
    # under the misbinding: BN on the reducing and 3x3 convs only, ReLU only after each add and in the head
    bns = [n for n in plan.nodes if n.kind == "bn"]
    assert len(bns) == 38 and sum(n.relu for n in bns) == 5
    assert sum(1 for n in plan.nodes if n.kind == "Relu") == 16 and sum(1 for n in plan.nodes if n.kind == "Add") == 16
    assert not any(n.relu for n in plan.nodes if n.kind == "conv")


def _census(rec):
    c = rec.calls
    fwd = sum(c.count(s) for s in ("seg_conv2d_fwd", "seg_conv2d_fwd_bn2", "seg_conv2d_fwd_pro", "seg_conv2d_fwd_hwio"))
    assert fwd == 60
    # forward: pool1 + the four pyramid pools + the three shared subsamples; each has its gradient
    assert c.count("seg_pool2d_fwd") == 8 and c.count("seg_pool2d_bwd") == 8
    fw = [(d.kh, d.kw, d.sh, d.sw, d.kind, d.OH, d.OW) for s, d in rec.pools if s == "seg_pool2d_fwd"]
    assert fw == [(3, 3, 2, 2, ops.POOL_MAX, 40, 144),
                  (1, 1, 2, 2, ops.POOL_AVG, 20, 72), (1, 1, 2, 2, ops.POOL_AVG, 10, 36), (1, 1, 2, 2, ops.POOL_AVG, 5, 18),
                  (5, 18, 5, 18, ops.POOL_AVG, 1, 1), (3, 9, 3, 9, ops.POOL_AVG, 1, 2), (2, 6, 2, 6, ops.POOL_AVG, 2, 3),
                  (1, 3, 1, 3, ops.POOL_AVG, 5, 6)]
    bw = [(d.kh, d.kw, d.kind) for s, d in rec.pools if s == "seg_pool2d_bwd"]
    assert sorted(bw) == sorted((f[0], f[1], f[4]) for f in fw)
    # both paddings run forward; only the second has an input that needs a gradient
    assert c.count("seg_pad2d_fwd") == 2 and c.count("seg_pad2d_bwd") == 1
    assert not any(s.startswith("seg_maxpool2x2") or s.startswith("seg_avgpool2x2") for s in c)
    dgrads = [d for s, d in rec.descs if s in ("seg_conv2d_bwd_data", "seg_conv2d_bwd_data_bn",
                                                "seg_conv2d_bwd_data_bn_part", "seg_conv2d_bwd_data_bits")]
    assert len(dgrads) == 59                             # every conv but conv1 (its input is the padded image)
    assert all(d.stride_h == 1 and d.stride_w == 1 for d in dgrads)      # NO strided input gradient
    assert not any(d.R == 7 for d in dgrads)
    wgrads = sum(c.count(s) for s in ("seg_conv2d_bwd_filter", "seg_conv2d_bwd_filter_begin", "seg_conv2d_bwd_filter_pro",
                                      "seg_conv2d_bwd_filter_adam"))
    assert wgrads == 60
    bn_bwd = sum(c.count(s) for s in ("seg_bn_relu_bwd", "seg_bn_relu_dropout_bwd", "seg_conv2d_bwd_data_bn",
                                      "seg_conv2d_bwd_data_bn_part"))
    assert bn_bwd == 38
    assert c.count("seg_resize_bilinear_fwd") + c.count("seg_spatial_broadcast") == 5
    assert c.count("seg_resize_bilinear_bwd") + c.count("seg_spatial_reduce") == 5
    assert c.count("seg_concat_fwd") == 1 and c.count("seg_concat_bwd") == 1
    assert c.count("seg_softmax_xent_fwd_bwd") + c.count("seg_softmax_xent_soft_fwd_bwd") == 1


def test_minimize_step_census(dry):
    pred, logits, loss, feed = _model()
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    dry.calls.clear()
    dry.descs.clear()
    dry.pools.clear()
    sess.run([train, loss], feed_dict=feed)
    _census(dry)
    plan, = sess.plans.values()
    pool1 = next(n for n in plan.nodes if n.kind == "Pool2D" and n.ops[0].name == "pool1")
    assert list(plan.pool_idx) == [id(pool1)] and plan.pool_idx[id(pool1)].numel() == N * 40 * 144 * 64
    # the 7x7 stride-2 stem stays a strided conv (forward and filter gradient only)
    stem = next(n for n in plan.nodes if n.kind == "conv" and n.w.var_name == "conv1/weights")
    assert (stem.desc.R, stem.desc.S, stem.desc.stride_h, stem.desc.OH, stem.desc.OW, stem.desc.pad_top) == \
        (7, 7, 2, 80, 288, 0)


def test_accumulate_template_step_census(dry):
    """The reference driver's step (Network/model/PSPNet.py:617-636, :684-690)."""
    G.reset_default_graph()
    g = build_train_graph()
    feed = {g["image"]: np.zeros((N, H, W, 4), np.float32), g["prediction"]: np.zeros((N, H, W, 2), np.float32),
            g["keep_probability"]: 0.8}
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    sess.run(g["zero_ops"])
    dry.calls.clear()
    dry.descs.clear()
    dry.pools.clear()
    sess.run(g["accum_ops"], feed_dict=feed)
    _census(dry)
    assert "seg_adam_tf1_pack" not in dry.calls and "seg_adam_tf1_step" not in dry.calls
    dry.calls.clear()
    sess.run(g["train_step"], feed_dict=feed)
    assert sess.store.step == 1
    assert not any(s.startswith(("seg_conv2d", "seg_pool2d", "seg_pad2d")) for s in dry.calls)   # Adam only


def _golden():
    with open(GOLDEN) as f:
        rows = [line.split() for line in f.read().splitlines() if line]
    return [(name, tuple(int(v) for v in shape.split(","))) for name, shape in rows]


def test_variable_names_and_shapes_follow_tf():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 4])
    PSPNet50(image, 2)
    want = _golden()
    assert len(want) == 60 + 38 * 4
    assert [(v.var_name, tuple(v.shape)) for v in tf.global_variables()] == want
    assert [v.var_name for v in tf.trainable_variables()] == \
        [n for n, _ in want if not n.rsplit("/", 1)[1].startswith("moving_")]
    # which layers own a batch_normalization scope under the misbinding
    owners, last = [], None
    for name, _ in want:
        scope, leaf = name.rsplit("/", 1)
        if leaf == "weights":
            last = scope
        elif leaf == "gamma":
            owners.append(last)
    assert owners[0] == "conv1" and owners[1:3] == ["conv2_1_1", "conv2_1_2"]
    assert not any(o.endswith("_3") and o != "conv3_3_1" and o.count("_") == 2 for o in owners)   # no expanding conv
    assert not any(o.startswith("shortcut") or o in ("encoder_output", "conv6") for o in owners)
    assert owners[-5:] == ["conv5_3_pool1_conv", "conv5_3_pool2_conv", "conv5_3_pool3_conv", "conv5_3_pool6_conv",
                           "conv5_4"]


def test_saver_round_trip_keeps_the_names(dry, tmp_path):
    from semanticsegmentation_tensorflow_amd import tf_bundle
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, 64, 96, 4])
    PSPNet50(image, 2, pyramid_windows=((2, 3), (1, 3), (2, 1), (1, 1)))
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    saver = tf.train.Saver(tf.global_variables())
    path = saver.save(sess, str(tmp_path / "PSPNet.ckpt"))
    names = [n for n, _ in _golden()]
    index = tf_bundle.read_index(path)
    assert all(n in index for n in names)
    before = {n: sess.variable_value(n).copy() for n in names}
    for n in names[:3]:
        sess.assign(n, np.zeros_like(before[n]))
    saver.restore(sess, path)
    for n in names:
        assert np.array_equal(sess.variable_value(n), before[n]), n
