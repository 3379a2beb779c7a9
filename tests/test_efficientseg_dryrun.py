"""EfficientSeg on the Session compiler, host logic only (no GPU): the C-ABI is
replaced by the recording stub of tests/test_deeplab_sep_dryrun.py, so the
checkpoint variable names, the stage shapes at 1 x 160 x 576 x 3 and the launch
census of one training step -- depthwise, BatchNorm + activation, squeeze and
excite launches -- can be checked on the CPU.  Numerics:
tests/test_gpu_efficientseg.py, tests/test_gpu_mbconv.py."""
import os

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, layers, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import session as S
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.efficientnet import (DEFAULT_BLOCK_ARGS, BlockArgs, EfficientSeg,
                                                              round_filters, round_repeats)
from tests.test_deeplab_sep_dryrun import _DwRec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "efficientseg_b0_variables.txt")
N, H, W, CLASSES = 1, 160, 576, 2
HOST_ONLY = ("seg_bn_act_bwd_workspace", "seg_se_squeeze_workspace", "seg_se_excite_bwd_workspace")
# (kernel, stride) of the encoder's depthwise convs, block by block, then the decoder's five
B0_DW = ([(3, 1), (3, 2), (3, 1), (5, 2), (5, 1), (3, 2), (3, 1), (5, 1), (5, 1), (5, 1), (5, 2), (5, 1), (5, 1),
          (5, 1), (3, 1)] + [(3, 1)] * 5)


class _MbRec(_DwRec):
    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self.real, name)
        return super().__getattr__(name)


@pytest.fixture
def dry(monkeypatch):
    rec = _MbRec(_lib.load())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return rec


def _model(phi="b0", h=H, w=W):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, h, w, 3], name="input")
    labels = tf.placeholder(tf.uint8, [None, h, w], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    logits = EfficientSeg(image, keep, phi, CLASSES)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    feed = {image: np.zeros((N, h, w, 3), np.float32), labels: np.zeros((N, h, w), np.uint8), keep: 0.8}
    return logits, loss, feed


def _golden():
    with open(GOLDEN) as f:
        rows = [line.split() for line in f.read().splitlines() if line]
    return [(name, tuple(int(v) for v in shape.split(","))) for name, shape in rows]


def test_block_table_and_rounding_are_the_reference_constants():
    assert BlockArgs._fields == ("kernel_size", "num_repeat", "input_filters", "output_filters", "expand_ratio",
                                 "id_skip", "strides", "se_ratio")
    assert [(a.kernel_size, a.num_repeat, a.input_filters, a.output_filters, a.expand_ratio, tuple(a.strides))
            for a in DEFAULT_BLOCK_ARGS] == [(3, 1, 32, 16, 1, (1, 1)), (3, 2, 16, 24, 6, (2, 2)),
                                            (5, 2, 24, 40, 6, (2, 2)), (3, 2, 40, 80, 6, (2, 2)),
                                            (5, 3, 80, 112, 6, (1, 1)), (5, 4, 112, 192, 7, (2, 2)),
                                            (3, 1, 192, 320, 6, (1, 1))]
    assert all(a.id_skip is True and a.se_ratio == 0.25 for a in DEFAULT_BLOCK_ARGS)
    assert round_filters(32, 1.0, 8) == 32 and round_filters(32, 1.1, 8) == 32 and round_filters(40, 1.1, 8) == 48
    assert round_filters(16, 1.4, 8) == 24 and round_filters(1280, 2.0, 8) == 2560
    assert round_repeats(2, 1.1) == 3 and round_repeats(4, 1.0) == 4 and round_repeats(1, 3.1) == 4


def test_variable_names_and_shapes_follow_tf():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 3])
    EfficientSeg(image, 0.8, "b0", CLASSES)
    want = _golden()
    assert [(v.var_name, tuple(v.shape)) for v in tf.global_variables()] == want
    names = [n for n, _ in want]
    assert "bock1a__filter" in names and "bock2a_expand_bn/gamma" in names and "block6d_se_reduce/weights" in names
    assert "bock1a_expand_conv/weights" not in names                      # expand ratio 1: no expansion phase
    # the decoder's anonymous BatchNorms count from zero: the encoder's named ones took no index
    anon = [n for n in names if n.startswith("batch_normalization") and n.endswith("/gamma")]
    assert anon[0] == "batch_normalization/gamma" and anon[-1] == "batch_normalization_12/gamma" and len(anon) == 13
    filters = [v for v in tf.global_variables() if v.var_name.endswith("_filter")]
    assert len(filters) == 20 and all(isinstance(v.initializer, G.glorot_uniform_initializer) for v in filters)
    assert [v.var_name for v in tf.trainable_variables()] == \
        [n for n in names if not n.rsplit("/", 1)[-1].startswith("moving_")]


def test_a_named_batch_norm_does_not_shift_default_names():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 4, 4, 8])
    layers.Batch_Normalization(x)
    layers.Batch_Normalization(x, axis=3, name="stem_bn")
    layers.Batch_Normalization(x, name="other_bn")
    layers.Batch_Normalization(x)
    assert [v.var_name for v in tf.global_variables() if v.var_name.endswith("/gamma")] == \
        ["batch_normalization/gamma", "stem_bn/gamma", "other_bn/gamma", "batch_normalization_1/gamma"]
    with pytest.raises(NotImplementedError):
        layers.Batch_Normalization(x, axis=1)


def test_conv2d_block_without_activation_builds_the_same_ops():
    def types(**kw):
        G.reset_default_graph()
        x = tf.placeholder(tf.float32, [None, 4, 4, 8])
        layers.Conv2D_Block(x, 16, name="c", **kw)
        return [op.type for op in G.get_default_graph().ops]
    plain = ["Placeholder", "VariableV2", "Conv2D"]
    bn = ["VariableV2"] * 4 + ["FusedBatchNorm"]
    assert types() == plain and types(activation=None) == plain
    assert types(batch_normalization=True, relu=True) == plain + bn + ["Relu"]
    assert types(batch_normalization=True, activation="relu") == plain + bn + ["Relu"]
    assert types(activation="swish") == plain + ["Swish"] and types(activation="sigmoid") == plain + ["Sigmoid"]
    with pytest.raises(ValueError):
        types(activation="tanh")


def test_multiply_takes_only_a_channel_gate():
    G.reset_default_graph()
    x = tf.placeholder(tf.float32, [None, 4, 6, 8])
    s = tf.placeholder(tf.float32, [None, 1, 1, 8])
    a, b = tf.math.multiply(x, s), tf.multiply(s, x)
    assert a.op.type == b.op.type == "Mul" and a.op.inputs == b.op.inputs == [x, s] and a.shape == x.shape
    for bad in ((x, x), (x, tf.placeholder(tf.float32, [None, 1, 1, 16])), (x, tf.placeholder(tf.float32, [None, 8])),
                (x, tf.placeholder(tf.float32, [None, 4, 1, 8]))):
        with pytest.raises(NotImplementedError):
            tf.math.multiply(*bad)
    assert tf.math.add(x, x).op.type == "Add" and tf.nn.swish(x).op.type == "Swish"
    assert tf.nn.sigmoid(x).op.type == tf.sigmoid(x).op.type == "Sigmoid"


@pytest.mark.parametrize("phi, repeats", [("b0", (1, 2, 2, 2, 3, 4, 1)), ("b1", (2, 3, 3, 3, 4, 5, 2))])
def test_stage_shapes_at_160x576(dry, phi, repeats):
    logits, loss, feed = _model(phi)
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    sess.run([logits], feed_dict=feed)
    plan, = sess.plans.values()
    convs = {n.w.var_name.split("/")[0]: n for n in plan.nodes if n.kind == "conv"}
    out = lambda n: plan.shapes[id(n.output)]      # noqa: E731
    assert out(convs["stem_conv"]) == (N, 80, 288, 32)
    stages = ((80, 288, 16), (40, 144, 24), (20, 72, 40), (10, 36, 80), (10, 36, 112), (5, 18, 192), (5, 18, 320))
    for i, ((h, w, c), reps) in enumerate(zip(stages, repeats), 1):
        assert out(convs[f"bock{i}a_project_conv"]) == (N, h, w, c)
        last = "bock{}a_".format(i) if reps == 1 else "block{}{}_".format(i, "abcdefgh"[reps - 1])
        assert out(convs[last + "project_conv"]) == (N, h, w, c)
        assert f"block{i}{'abcdefgh'[reps]}_project_conv" not in convs
    assert out(convs["top_conv"]) == (N, 5, 18, 1280)                     # the feature map is 5 x 18
    assert out(convs["bock2a_expand_conv"]) == (N, 80, 288, 96)
    # the squeeze-excite convs are ordinary padded 1x1 convs on [N, 1, 1, C]
    for name, k in (("bock1a_se_reduce", 8), ("bock2a_se_reduce", 4), ("block2b_se_reduce", 6),
                    ("bock3a_se_reduce", 6), ("block3b_se_reduce", 10)):
        d = convs[name].desc
        assert out(convs[name]) == (N, 1, 1, k)
        assert (d.H, d.W, d.R, d.S, d.k_valid, d.K) == (1, 1, 1, 1, k, 8 * -(-k // 8))
    assert out(convs["image_pooling"]) == (N, 1, 1, 256) and out(convs["aspp0"]) == (N, 5, 18, 256)
    assert out(convs["concatenation_conv"]) == (N, 5, 18, 256) and out(convs["last_layer"]) == (N, 10, 36, CLASSES)
    assert plan.shapes[id(logits)] == (N, H, W, CLASSES)
    blocks = sum(repeats)
    kinds = [n.kind for n in plan.nodes]
    assert kinds.count("se_excite") == blocks and kinds.count("act") == 2 * blocks
    assert kinds.count("Add") == blocks - 7                 # the identity add: every repeat, no stage's first block
    swish_bn = [n for n in plan.nodes if n.kind == "bn" and n.act == "swish"]
    # two per block, less the expansion phase the first stage (expand ratio 1) does not have
    assert len(swish_bn) == 2 * blocks - repeats[0] and not any(n.relu for n in swish_bn)
    assert not any(n.kind in ("Swish", "Sigmoid", "Mul") for n in plan.nodes)
    # no ReLU-BatchNorm fusion took a swish BatchNorm
    assert not any(id(n) in plan.folded or id(n) in plan.bn_out2_done for n in swish_bn)
    assert not any(b.act is not None for b in plan.bn_before.values())


def _census(dry, dtype):
    logits, loss, feed = _model("b0")
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    sess = S.Session(device=torch.device("cpu"), compute_dtype=dtype)
    sess.run(tf.global_variables_initializer())
    dry.calls.clear()
    dry.descs.clear()
    dry.dws.clear()
    sess.run([train, loss], feed_dict=feed)
    return sess, dry.calls


def test_minimize_step_census(dry):
    sess, c = _census(dry, "bf16")
    assert [c.count(s) for s in ("seg_dwconv2d_fwd", "seg_dwconv2d_bwd_data", "seg_dwconv2d_bwd_filter")] == [20] * 3
    fwd = [(d.R, d.stride) for s, d in dry.dws if s == "seg_dwconv2d_fwd"]
    assert fwd == B0_DW and all(d.R == d.S for _, d in dry.dws)
    for sym in ("seg_dwconv2d_bwd_data", "seg_dwconv2d_bwd_filter"):
        assert [(d.R, d.stride) for s, d in dry.dws if s == sym] == B0_DW[::-1]
    # 15 blocks: 14 expand_bn + 15 bn with swish, 15 se_reduce swish + 15 se_expand sigmoid
    assert c.count("seg_bn_act_fwd") == 59 and c.count("seg_bn_act_bwd") == 59
    assert c.count("seg_se_excite_fwd") == 15 and c.count("seg_se_excite_bwd") == 15
    # bf16: every squeeze fits the present kernel (1344 channels = 168 chunks), with the decoder's pool and the
    # gradient of its 1x1 -> 5x18 broadcast
    assert c.count("seg_spatial_reduce") == 17 and c.count("seg_se_squeeze") == 0
    assert c.count("seg_spatial_broadcast") == 17
    assert c.count("seg_softmax_xent_fwd_bwd") + c.count("seg_softmax_xent_soft_fwd_bwd") == 1
    plan, = sess.plans.values()
    assert not plan.uncovered and len(plan.adam_names) == len([v for v in tf.trainable_variables()])
    need = max(ops.bn_act_bwd_workspace(N * 80 * 288, 96), ops.se_squeeze_workspace(N, 80, 288, 96))
    assert need > 0 and sess.ws.buf.numel() >= need


def test_wide_fp32_maps_take_the_squeeze_kernel(dry):
    """fp32: 1344 (block6b-d), 1152 (bock7a) and the decoder's 1280 channels are
    336, 288 and 320 sixteen-byte chunks, more than seg_spatial_reduce takes."""
    sess, c = _census(dry, "f32")
    assert c.count("seg_se_squeeze") == 5 and c.count("seg_spatial_reduce") == 12
    assert c.count("seg_se_excite_fwd") == 15 and c.count("seg_bn_act_fwd") == 59
