"""LidCamNet on the Session compiler, host logic only (no GPU): the C-ABI is
replaced by a recording stub (the pattern of tests/test_session_dryrun.py),
so the launch census of one training step, the descriptors of the strided and
the per-axis dilated convs and the checkpoint variable names can be checked on
the CPU.  Numerics: tests/test_gpu_lidcamnet.py."""
import os

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from semanticsegmentation_tensorflow_amd import graph as G
from semanticsegmentation_tensorflow_amd import session as S
from semanticsegmentation_tensorflow_amd import tf
from semanticsegmentation_tensorflow_amd.lidcamnet import LidCamNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidcamnet_variables.txt")


class _Rec:
    def __init__(self, real):
        self.real = real
        self.calls = []
        self.descs = []        # (symbol, copy of the descriptor) of every recorded conv launch

    def __getattr__(self, name):
        real_fn = getattr(self.real, name)
        host_only = name in ("seg_conv_desc_init", "seg_conv_desc_init2", "seg_tconv_desc_init", "seg_conv_workspace",
                             "seg_bias_grad_workspace", "seg_xent_workspace", "seg_status_string",
                             "seg_adam_segments_plan", "seg_tconv_filter_apad",
                             "seg_conv_wgrad_adam_fusable", "seg_conv_bwd_data_bn_workspace",
                             "seg_conv2d_fwd_pool_ok", "seg_conv2d_fwd_bn2_ok", "seg_conv2d_fwd_hwio_ok",
                             "seg_conv2d_fwd_relu_bits_ok", "seg_conv2d_bwd_data_bits_ok",
                             "seg_conv2d_bwd_data_s2_ok")

        def fn(*a):
            if host_only:
                return real_fn(*a)
            self.calls.append(name)
            d = getattr(a[0], "_obj", None) if a else None
            if isinstance(d, _lib.SegConvDesc):
                self.descs.append((name, _lib.SegConvDesc.from_buffer_copy(d)))
            return 0
        return fn


@pytest.fixture
def dry(monkeypatch):
    rec = _Rec(_lib.load())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    return rec


N, H, W = 2, 32, 64


def _model():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 4], name="input_image")
    labels = tf.placeholder(tf.uint8, [None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    pred, logits = LidCamNet(image, keep, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    feed = {image: np.zeros((N, H, W, 4), np.float32), labels: np.zeros((N, H, W), np.uint8), keep: 0.8}
    return pred, logits, loss, feed


def _census(rec):
    c = rec.calls
    fwd = sum(c.count(s) for s in ("seg_conv2d_fwd", "seg_conv2d_fwd_bn2", "seg_conv2d_fwd_pro", "seg_conv2d_fwd_hwio"))
    assert fwd == 18                                     # conv1..14, 16, 18, 20, 21
    assert c.count("seg_tconv2d_fwd") == 3               # conv15, 17, 19
    dgrads = [d for s, d in rec.descs if s in ("seg_conv2d_bwd_data", "seg_conv2d_bwd_data_bn",
                                                "seg_conv2d_bwd_data_bn_part")]
    assert len(dgrads) == 17                             # every Conv2D but conv1 (x is a placeholder)
    strided = [(d.H, d.W, d.c_valid, d.k_valid, d.R, d.S) for d in dgrads if d.stride_h == 2]
    assert sorted(strided) == sorted([(H // 2, W // 2, 32, 64, 4, 4), (H // 4, W // 4, 64, 128, 4, 4)])   # conv3, conv5
    assert all(d.stride_w == d.stride_h for d in dgrads)
    assert not any(d.c_valid == 4 and d.R == 4 for d in dgrads)    # no input gradient for conv1 (4 -> 32, 4x4 / 2)
    assert c.count("seg_tconv2d_bwd_data") == 3
    wgrads = sum(c.count(s) for s in ("seg_conv2d_bwd_filter", "seg_conv2d_bwd_filter_begin", "seg_conv2d_bwd_filter_pro",
                                      "seg_conv2d_bwd_filter_adam")) + c.count("seg_tconv2d_bwd_filter")
    assert wgrads == 21
    bn_bwd = sum(c.count(s) for s in ("seg_bn_relu_bwd", "seg_bn_relu_dropout_bwd", "seg_conv2d_bwd_data_bn",
                                      "seg_conv2d_bwd_data_bn_part"))
    assert bn_bwd == 20                                  # every layer but conv21
    assert c.count("seg_softmax_xent_fwd_bwd") == 1


def test_minimize_step_census_and_descriptors(dry):
    pred, logits, loss, feed = _model()
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    dry.calls.clear()
    dry.descs.clear()
    sess.run([train, loss], feed_dict=feed)
    _census(dry)
    assert dry.calls.count("seg_adam_tf1_pack") == 1
    # the context module's five per-axis dilations reach the descriptors
    plan, = sess.plans.values()
    by_name = {n.w.var_name: n for n in plan.nodes if n.kind == "conv"}
    got = [(by_name[f"conv{i}/weights"].desc.dil_h, by_name[f"conv{i}/weights"].desc.dil_w) for i in range(8, 13)]
    assert got == [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32)]
    for i in (6, 7, 13, 14, 16, 21):
        d = by_name[f"conv{i}/weights"].desc
        assert (d.dil_h, d.dil_w, d.stride_h) == (1, 1, 1)
    for i, (c, k) in ((1, (4, 32)), (3, (32, 64)), (5, (64, 128))):
        d = by_name[f"conv{i}/weights"].desc
        assert (d.R, d.S, d.stride_h, d.stride_w, d.c_valid, d.k_valid) == (4, 4, 2, 2, c, k)
    # the halo kernel takes conv3's and conv5's input gradients (bf16)
    assert ops.conv2d_bwd_data_s2_ok(by_name["conv3/weights"].desc)
    assert ops.conv2d_bwd_data_s2_ok(by_name["conv5/weights"].desc)
    # the decoder's transposed convs take only shapes: conv19 has x's 4 channels
    t19 = next(n for n in plan.nodes if n.kind == "tconv" and n.w.var_name == "conv19/weights")
    assert (t19.desc.OH, t19.desc.OW, t19.desc.k_valid, t19.desc.c_valid) == (H, W, 4, 32)


def test_accumulate_template_step_census(dry):
    """The reference driver's step (Network/model/LidCamNet.py:106-125)."""
    pred, logits, loss, feed = _model()
    opt = tf.train.AdamOptimizer(1e-4)
    const = tf.constant(1 / 4 * 3)
    t_vars = tf.trainable_variables()
    accum = [tf.Variable(tf.zeros_like(t.initialized_value()), trainable=False) for t in t_vars]
    zero_ops = [a.assign(tf.zeros_like(a)) for a in accum]
    gvs = opt.compute_gradients(loss, t_vars)
    accum_ops = [accum[i].assign_add(tf.scalar_mul(const, gv[0])) for i, gv in enumerate(gvs)]
    train_step = opt.apply_gradients([(accum[i], gv[1]) for i, gv in enumerate(gvs)])
    sess = S.Session(device=torch.device("cpu"), compute_dtype="bf16")
    sess.run(tf.global_variables_initializer())
    sess.run(zero_ops)
    dry.calls.clear()
    dry.descs.clear()
    sess.run(accum_ops, feed_dict=feed)
    _census(dry)
    assert "seg_adam_tf1_pack" not in dry.calls and "seg_adam_tf1_step" not in dry.calls
    dry.calls.clear()
    sess.run(train_step, feed_dict=feed)
    assert sess.store.step == 1
    assert not any(s.startswith(("seg_conv2d", "seg_tconv2d")) for s in dry.calls)   # Adam only


def test_variable_names_follow_tf():
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, [None, H, W, 4])
    LidCamNet(image, 1.0, 2)
    names = [v.var_name for v in tf.global_variables()]
    with open(GOLDEN) as f:
        want = f.read().split()
    assert len(want) == 21 + 20 * 4
    assert names == want
    assert [v.var_name for v in tf.trainable_variables()] == [n for n in want if not n.rsplit("/", 1)[1].startswith("moving_")]
