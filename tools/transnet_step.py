"""Time FC-DenseNet + TransNet training steps
(Network/model/FCDenseNet_TransNet.py) at batch 4, 160 x 576, image 3 channels
+ ADI 1 channel, keep_prob 0.2, under the weighted three-head loss -- the
method of tools/lidcamnet_step.py:

    python tools/transnet_step.py [--form minimize|accumulate] [--dtype bf16] [--steps 50] [--warmup 10]

`minimize` is one forward + backward + Adam per step; `accumulate` is the
reference driver's step (:279-297, :352-361): zero the accumulators, B forward
+ backward passes adding const * g, then Adam on the accumulators with the
main head's loss fetched beside it.  Prints one JSON line with the step time
and images/s over the timed steps (host clock around work that ends in a
device synchronise) and the launch count of one step's plan."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import graph as G  # noqa: E402
from semanticsegmentation_tensorflow_amd import tf  # noqa: E402
from semanticsegmentation_tensorflow_amd.fcdensenet_transnet import KEEP_PROB, FCDenseNet, training_loss  # noqa: E402

H, W = 160, 576


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["minimize", "accumulate"], default="minimize")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("transnet_step: no GPU (timings are taken on the device only)")
    B = a.batch
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 3], name="input_image")
    adi = tf.placeholder(tf.float32, shape=[None, H, W, 1], name="input_adi")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    _, logits, lid_logits, aux_logits = FCDenseNet(image, adi, keep, 2)
    loss, total = training_loss(logits, lid_logits, aux_logits, labels)
    opt = tf.train.AdamOptimizer(1e-4)
    rng = np.random.default_rng(0)
    feed = {image: rng.standard_normal((B, H, W, 3)).astype(np.float32),
            adi: rng.standard_normal((B, H, W, 1)).astype(np.float32),
            labels: (rng.random((B, H, W)) < 0.5).astype(np.uint8), keep: KEEP_PROB}
    if a.form == "minimize":
        train = opt.minimize(total)

        def step():
            sess.run(train, feed_dict=feed)
    else:
        const = tf.constant(1 / B * 3)
        t_vars = tf.trainable_variables()
        accum = [tf.Variable(tf.zeros_like(t.initialized_value()), trainable=False) for t in t_vars]
        zero_ops = [v.assign(tf.zeros_like(v)) for v in accum]
        gvs = opt.compute_gradients(total, t_vars)
        accum_ops = [accum[i].assign_add(tf.scalar_mul(const, gv[0])) for i, gv in enumerate(gvs)]
        train = opt.apply_gradients([(accum[i], gv[1]) for i, gv in enumerate(gvs)])

        def step():
            sess.run(zero_ops)
            for _ in range(B):
                sess.run(accum_ops, feed_dict=feed)
            sess.run([train, loss], feed_dict=feed)
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
    plan = max(sess.plans.values(), key=lambda p: len(p.nodes))
    kinds = [n.kind for n in plan.nodes]
    print(json.dumps({"model": "FCDenseNet_TransNet", "form": a.form, "dtype": a.dtype, "batch": B, "hw": [H, W],
                      "keep_prob": KEEP_PROB, "steps": a.steps, "warmup": a.warmup,
                      "step_ms": round(dt / a.steps * 1e3, 3),
                      "images_per_s": round(B * passes * a.steps / dt, 1), "plan_nodes": len(kinds),
                      "film": kinds.count("film"), "axpy": kinds.count("axpy"), "xent": kinds.count("xent"),
                      "copying_concats": sum(1 for n in plan.nodes if n.kind == "ConcatV2"
                                             and id(n) not in plan.alias_nodes)}))


if __name__ == "__main__":
    main()
