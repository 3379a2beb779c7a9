"""Time LidCamNet training steps (Network/model/LidCamNet.py) at the shape
the reference runs, batch 4 at 160 x 576 x 4, keep_prob 0.8:

    python tools/lidcamnet_step.py [--form minimize|accumulate] [--dtype bf16] [--steps 50] [--warmup 10]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/lidcamnet_step.py --steps 5 --warmup 3

`minimize` is one forward + backward + Adam per step; `accumulate` is the
reference driver's step (LidCamNet.py:106-125): zero the accumulators, B
forward + backward passes adding const * g, then Adam on the accumulators.
Prints one JSON line with images/s over the timed steps (host clock around
work that ends in a device synchronise)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import graph as G  # noqa: E402
from semanticsegmentation_tensorflow_amd import ops, tf  # noqa: E402
from semanticsegmentation_tensorflow_amd.lidcamnet import BATCH_SIZE, IMAGE_SHAPE_KITTI, KEEP_PROB, LidCamNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["minimize", "accumulate"], default="minimize")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=BATCH_SIZE)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lidcamnet_step: no GPU (timings are taken on the device only)")
    H, W = IMAGE_SHAPE_KITTI
    B = a.batch
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 4], name="input_image")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    _, logits = LidCamNet(image, keep, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    opt = tf.train.AdamOptimizer(1e-4)
    rng = np.random.default_rng(0)
    feed = {image: rng.standard_normal((B, H, W, 4)).astype(np.float32),
            labels: (rng.random((B, H, W)) < 0.5).astype(np.uint8), keep: KEEP_PROB}
    if a.form == "minimize":
        train = opt.minimize(loss)

        def step():
            sess.run(train, feed_dict=feed)
    else:
        const = tf.constant(1 / B * 3)
        t_vars = tf.trainable_variables()
        accum = [tf.Variable(tf.zeros_like(t.initialized_value()), trainable=False) for t in t_vars]
        zero_ops = [v.assign(tf.zeros_like(v)) for v in accum]
        gvs = opt.compute_gradients(loss, t_vars)
        accum_ops = [accum[i].assign_add(tf.scalar_mul(const, gv[0])) for i, gv in enumerate(gvs)]
        train = opt.apply_gradients([(accum[i], gv[1]) for i, gv in enumerate(gvs)])

        def step():
            sess.run(zero_ops)
            for _ in range(B):
                sess.run(accum_ops, feed_dict=feed)
            sess.run(train, feed_dict=feed)
    sess = tf.Session(compute_dtype=a.dtype)
    sess.run(tf.global_variables_initializer())
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    passes = B if a.form == "accumulate" else 1
    print(json.dumps({"model": "LidCamNet", "form": a.form, "dtype": a.dtype, "batch": B, "hw": [H, W],
                      "keep_prob": KEEP_PROB, "steps": a.steps, "step_ms": round(dt / a.steps * 1e3, 3),
                      "images_per_s": round(B * passes * a.steps / dt, 1),
                      "dgrad_s2": ops.get_option("dgrad_s2")}))


if __name__ == "__main__":
    main()
