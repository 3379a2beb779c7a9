"""Time training steps of DeepLabSepASPP (separable ASPP + SepConv decoder)
and of DeepLabASPP (dense atrous ASPP) on the same VGG atrous backbone,
alternating in one process at one shape and dtype:

    python tools/deeplab_sep_step.py [--dtype bf16] [--batch 4] [--height 384] [--width 1248] [--steps 10] [--repeats 3]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/deeplab_sep_step.py --only sep --steps 5 --repeats 1

One step is forward + backward + Adam (minimize), keep_prob 0.9.  Prints one
JSON line per model and repeat with ms/step over the timed steps (host clock
around work that ends in a device synchronise), then a summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import graph as G  # noqa: E402
from semanticsegmentation_tensorflow_amd import tf  # noqa: E402
from semanticsegmentation_tensorflow_amd.deeplab import KEEP_PROB, DeepLabASPP, DeepLabSepASPP  # noqa: E402


def make(model, B, H, W, dtype):
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 3], name="input_image")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    _, logits = model(image, keep, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    rng = np.random.default_rng(0)
    feed = {image: rng.standard_normal((B, H, W, 3)).astype(np.float32),
            labels: (rng.random((B, H, W)) < 0.5).astype(np.uint8), keep: KEEP_PROB}
    sess = tf.Session(compute_dtype=dtype)
    sess.run(tf.global_variables_initializer())
    return lambda: sess.run(train, feed_dict=feed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1248)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["sep", "dense"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("deeplab_sep_step: no GPU (timings are taken on the device only)")
    models = {"sep": ("DeepLabSepASPP", DeepLabSepASPP), "dense": ("DeepLabASPP", DeepLabASPP)}
    if a.only:
        models = {a.only: models[a.only]}
    steps = {k: make(m, a.batch, a.height, a.width, a.dtype) for k, (_, m) in models.items()}
    for step in steps.values():
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for rep in range(a.repeats):
        for k, step in steps.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
            print(json.dumps({"model": models[k][0], "dtype": a.dtype, "batch": a.batch, "hw": [a.height, a.width],
                              "repeat": rep, "steps": a.steps, "step_ms": round(ms[k][-1], 3),
                              "images_per_s": round(a.batch * 1e3 / ms[k][-1], 1)}), flush=True)
    print(json.dumps({"summary": {models[k][0]: {"median_step_ms": round(statistics.median(v), 3),
                                                 "min_step_ms": round(min(v), 3)} for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
