"""DeepLabSepASPP on the Session compiler, host logic only (no GPU): the C-ABI
is replaced by the recording stub of tests/test_lidcamnet_dryrun.py (with the
depthwise descriptor's host-only functions let through), so the stage shapes
at 1 x 160 x 576 x 3, the launch census of one training step -- five depthwise
forwards, input gradients and filter gradients, with their descriptors -- and
the checkpoint variable names can be checked on the CPU.  Numerics:
tests/test_gpu_deeplab_sep.py."""
import os

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import session as S
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.deeplab import ASPP_RATES, DeepLabSepASPP
from tests.test_lidcamnet_dryrun import _Rec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeplab_sep_variables.txt")
N, H, W, CLASSES = 1, 160, 576, 2
DW_LAUNCHES = ("seg_dwconv2d_fwd", "seg_dwconv2d_bwd_data", "seg_dwconv2d_bwd_filter")


class _DwRec(_Rec):
    """The LidCamNet dry run's recorder; seg_dwconv_desc_init and the workspace
    query are host-only arithmetic and run for real, and the depthwise
    descriptors are recorded too."""

    def __init__(self, real):
        super().__init__(real)
        self.dws = []          # (symbol, copy of the seg_dwconv_desc) of every recorded depthwise launch

    def __getattr__(self, name):
        if name in ("seg_dwconv_desc_init", "seg_dwconv_bwd_filter_workspace"):
            return getattr(self.real, name)
        fn = super().__getattr__(name)
        if name not in DW_LAUNCHES:
            return fn

        def dw(*a):
            self.dws.append((name, _lib.SegDwconvDesc.from_buffer_copy(a[0]._obj)))
            return fn(*a)
        return dw


@pytest.fixture
def dry(monkeypatch):
    rec = _DwRec(_lib.load())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return rec


def _model(h=H, w=W, **kw):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, h, w, 3], name="input_image")
    labels = tf.placeholder(tf.uint8, [None, h, w], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    pred, logits = DeepLabSepASPP(image, keep, CLASSES, **kw)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    feed = {image: np.zeros((N, h, w, 3), np.float32), labels: np.zeros((N, h, w), np.uint8), keep: 0.9}
    return pred, logits, loss, feed


def test_default_rates_are_the_reference_constants():
    assert ASPP_RATES == (6, 12, 18)


def test_stage_shapes_at_160x576(dry):
    pred, logits, loss, feed = _model()
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    sess.run([logits, pred], feed_dict=feed)
    plan, = sess.plans.values()
    convs = {n.w.var_name.split("/")[0]: n for n in plan.nodes if n.kind == "conv"}
    dws = {n.w.var_name: n for n in plan.nodes if n.kind == "dwconv"}

    def out(n):
        return plan.shapes[id(n.output)]
    assert out(convs["conv5_3"]) == (N, 20, 72, 512)                      # output stride 8
    assert out(convs["image_pooling"]) == (N, 1, 1, 256) and out(convs["aspp0"]) == (N, 20, 72, 256)
    assert list(dws) == ["aspp1_filter", "aspp2_filter", "aspp3_filter", "decoder_conv0_filter",
                         "decoder_conv1_filter"]
    for i, r in enumerate(ASPP_RATES):
        n = dws[f"aspp{i + 1}_filter"]
        assert n.inputs[0] is convs["conv5_3"].output and out(n) == (N, 20, 72, 512)
        d = n.desc
        assert (d.H, d.W, d.C, d.c_valid, d.R, d.S, d.stride, d.dil_h, d.dil_w, d.pad_top, d.pad_left) == \
            (20, 72, 512, 512, 3, 3, 1, r, r, r, r)
        assert out(convs[f"aspp{i + 1}_pointwise_BN"]) == (N, 20, 72, 256)
    cat, = [n for n in plan.nodes if n.kind == "ConcatV2"]
    assert out(cat) == (N, 20, 72, 1280) and [plan.shapes[id(t)][3] for t in cat.inputs] == [256] * 5
    assert out(convs["concatenation_conv"]) == (N, 20, 72, 256)
    up, final = [n for n in plan.nodes if n.kind == "ResizeBilinear"][1:]
    assert out(up) == (N, 40, 144, 256) and out(final) == (N, H, W, CLASSES)
    for name in ("decoder_conv0_filter", "decoder_conv1_filter"):
        d = dws[name].desc
        assert out(dws[name]) == (N, 40, 144, 256)
        assert (d.H, d.W, d.C, d.R, d.S, d.stride, d.dil_h, d.dil_w, d.pad_top, d.pad_left) == \
            (40, 144, 256, 3, 3, 1, 1, 1, 1, 1)
    assert out(convs["last_layer"]) == (N, 40, 144, CLASSES)
    assert plan.shapes[id(logits)] == (N, H, W, CLASSES) and plan.shapes[id(pred)] == (N, H, W, 1)
    # the depthwise conv is a node of its own: no conv fusion holds it, and
    # every BatchNorm around it is a bn node (13 of them: 3 + 2 per SepConv_BN)
    assert sum(1 for n in plan.nodes if n.kind == "bn") == 13
    assert not any(n.kind == "Relu" for n in plan.nodes)                  # every ReLU rides on its BN / conv node


def test_minimize_step_census(dry):
    pred, logits, loss, feed = _model()
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    dry.calls.clear()
    dry.descs.clear()
    dry.dws.clear()
    sess.run([train, loss], feed_dict=feed)
    c = dry.calls
    assert [c.count(s) for s in DW_LAUNCHES] == [5, 5, 5]
    geo = lambda d: (d.N, d.H, d.W, d.C, d.c_valid, d.OH, d.OW, d.R, d.S, d.stride, d.dil_h, d.dil_w,   # noqa: E731
                     d.pad_top, d.pad_left, d.ldx, d.ldy, d.dtype)
    aspp = [(N, 20, 72, 512, 512, 20, 72, 3, 3, 1, r, r, r, r, 512, 512, ops.BF16) for r in ASPP_RATES]
    dec = [(N, 40, 144, 256, 256, 40, 144, 3, 3, 1, 1, 1, 1, 1, 256, 256, ops.BF16)] * 2
    assert [geo(d) for s, d in dry.dws if s == "seg_dwconv2d_fwd"] == aspp + dec
    for sym in DW_LAUNCHES[1:]:                                           # backward: the reverse order
        assert [geo(d) for s, d in dry.dws if s == sym] == (aspp + dec)[::-1]
    # the dense convs around them: 13 backbone + image_pooling, aspp0, 5 pointwise, concatenation_conv, last_layer
    fwd = sum(c.count(s) for s in ("seg_conv2d_fwd", "seg_conv2d_fwd_bn2", "seg_conv2d_fwd_pro", "seg_conv2d_fwd_hwio",
                                   "seg_conv2d_fwd_pool", "seg_conv2d_fwd_relu_bits"))
    assert fwd == 22
    wgrads = sum(c.count(s) for s in ("seg_conv2d_bwd_filter", "seg_conv2d_bwd_filter_begin",
                                      "seg_conv2d_bwd_filter_pro", "seg_conv2d_bwd_filter_adam"))
    assert wgrads == 22
    assert not any(d.R == 3 and d.dil_h in ASPP_RATES for s, d in dry.descs)     # no dense atrous ASPP branch
    bn_bwd = sum(c.count(s) for s in ("seg_bn_relu_bwd", "seg_bn_relu_dropout_bwd", "seg_conv2d_bwd_data_bn",
                                      "seg_conv2d_bwd_data_bn_part"))
    assert bn_bwd == 13
    assert c.count("seg_softmax_xent_fwd_bwd") + c.count("seg_softmax_xent_soft_fwd_bwd") == 1
    # Adam sees the depthwise filters: they are in the plan's update list and nothing is left uncovered
    plan, = sess.plans.values()
    names = [f"aspp{i}_filter" for i in (1, 2, 3)] + ["decoder_conv0_filter", "decoder_conv1_filter"]
    assert all(nm in plan.adam_names for nm in names) and not plan.uncovered
    assert not any(nm in plan.never_ready for nm in names)
    # the filter-gradient workspaces are sized from the library's query
    for n in plan.nodes:
        if n.kind == "dwconv":
            assert plan.wg_ws[id(n)].numel() >= ops.dwconv_bwd_filter_workspace(n.desc) > 0
            assert sess.ws.buf.numel() >= ops.dwconv_bwd_filter_workspace(n.desc)


def _golden():
    with open(GOLDEN) as f:
        rows = [line.split() for line in f.read().splitlines() if line]
    return [(name, tuple(int(v) for v in shape.split(","))) for name, shape in rows]


def test_variable_names_and_shapes_follow_tf():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 3])
    DeepLabSepASPP(image, 0.9, CLASSES)
    want = _golden()
    assert len(want) == 13 * 2 + 9 + 5 + 13 * 4
    assert [(v.var_name, tuple(v.shape)) for v in tf.global_variables()] == want
    assert [v.var_name for v in tf.trainable_variables()] == \
        [n for n, _ in want if not n.rsplit("/", 1)[-1].startswith("moving_")]
    filters = [v for v in tf.global_variables() if v.var_name.endswith("_filter")]
    assert len(filters) == 5 and all(isinstance(v.initializer, G.glorot_uniform_initializer) for v in filters)


def test_saver_round_trip_keeps_the_names(dry, tmp_path):
    from semanticsegmentation_tensorflow_amd import tf_bundle
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, 32, 48, 3])
    DeepLabSepASPP(image, 0.9, CLASSES, aspp_rates=(1, 2, 3))
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    saver = tf.train.Saver(tf.global_variables())
    path = saver.save(sess, str(tmp_path / "DeepLabSep.ckpt"))
    names = [n for n, _ in _golden()]
    index = tf_bundle.read_index(path)
    assert all(n in index for n in names)
    before = {n: sess.variable_value(n).copy() for n in names}
    for n in ("aspp1_filter", "decoder_conv1_filter", "last_layer/weights"):
        sess.assign(n, np.zeros_like(before[n]))
    saver.restore(sess, path)
    for n in names:
        assert np.array_equal(sess.variable_value(n), before[n]), n
