"""Time training steps of EfficientSeg and split the step's kernel time by
kernel family, in one process at one shape and dtype:

    python tools/efficientseg_step.py [--phi b0] [--dtype bf16] [--batch 4] [--height 160] [--width 576]
                                      [--steps 10] [--repeats 3]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/efficientseg_step.py --steps 5 --repeats 1
    python tools/efficientseg_step.py --stats-csv prof_out/.../kernel_stats.csv --traced-steps 8

One step is forward + backward + Adam (minimize), keep_prob 0.8.  Prints one
JSON line per repeat with ms/step over the timed steps (host clock around work
that ends in a device synchronise) and a summary line.  With --stats-csv it
reads the kernel statistics of such a trace instead and prints the launch
count per step and the kernel-time share of each kernel family (depthwise,
BatchNorm + swish / sigmoid, squeeze, excite, dense convs, BatchNorm + ReLU,
the rest)."""
import argparse
import collections
import csv
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
from semanticsegmentation_tensorflow_amd.efficientnet import EfficientSeg  # noqa: E402

# kernel-name fragment -> family, first match wins
FAMILIES = [("dw_", "depthwise"), ("bn_act_", "bn + swish/sigmoid"), ("se_sum_k", "squeeze / excite grad"),
            ("se_finish", "squeeze / excite grad"), ("se_excite_fwd", "excite fwd"), ("spatial_", "global pool"),
            ("scale_cast", "global pool"), ("bn_relu", "bn (+relu)"), ("bn_finish", "bn (+relu)"),
            ("bn_fold", "bn (+relu)"), ("adam", "adam + pack"), ("pack", "adam + pack"), ("igemm", "dense conv"),
            ("conv", "dense conv"), ("halo", "dense conv"), ("wgrad", "dense conv"), ("dense1x1", "dense conv"),
            ("smallc", "dense conv"), ("bn1x1", "dense conv"), ("reduce", "dense conv")]


def family(name):
    for frag, fam in FAMILIES:
        if frag in name:
            return fam
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phi", default="b0")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--width", type=int, default=576)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stats-csv", default=None, help="a kernel_stats.csv to split by family (no GPU needed)")
    ap.add_argument("--traced-steps", type=int, default=8, help="steps the trace behind --stats-csv held")
    a = ap.parse_args()
    if a.stats_csv:
        shares(a.stats_csv, a.traced_steps)
        return
    if not torch.cuda.is_available():
        sys.exit("efficientseg_step: no GPU (timings are taken on the device only)")
    B, H, W = a.batch, a.height, a.width
    G.reset_default_graph()
    image = tf.placeholder(tf.float32, shape=[None, H, W, 3], name="input")
    labels = tf.placeholder(tf.uint8, shape=[None, H, W], name="annotation")
    keep = tf.placeholder(tf.float32, name="keep_probability")
    logits = EfficientSeg(image, keep, a.phi, 2)
    loss = tf.reduce_mean(tf.nn.softmax_cross_entropy_with_logits(logits=logits, labels=labels))
    train = tf.train.AdamOptimizer(1e-4).minimize(loss)
    rng = np.random.default_rng(0)
    feed = {image: rng.standard_normal((B, H, W, 3)).astype(np.float32),
            labels: (rng.random((B, H, W)) < 0.5).astype(np.uint8), keep: 0.8}
    sess = tf.Session(compute_dtype=a.dtype)
    sess.run(tf.global_variables_initializer())
    step = lambda: sess.run(train, feed_dict=feed)      # noqa: E731
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for rep in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
        print(json.dumps({"model": f"EfficientSeg({a.phi!r})", "dtype": a.dtype, "batch": B, "hw": [H, W],
                          "repeat": rep, "steps": a.steps, "step_ms": round(ms[-1], 3),
                          "images_per_s": round(B * 1e3 / ms[-1], 1)}), flush=True)

    print(json.dumps({"summary": {"median_step_ms": round(statistics.median(ms), 3), "min_step_ms": round(min(ms), 3),
                                  "traced_steps": a.warmup + a.steps * a.repeats}}))


def shares(path, steps):
    """Kernel-time share and launches per step by family from a kernel_stats.csv
    (Name, Calls, TotalDurationNs, ...) of a trace that held `steps` steps."""
    ns, calls = collections.Counter(), collections.Counter()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            fam = family(row["Name"])
            ns[fam] += int(row["TotalDurationNs"])
            calls[fam] += int(row["Calls"])
    total = sum(ns.values()) or 1
    print(f"{path}: {steps} steps, {sum(calls.values()) / steps:.0f} launches and {total / steps / 1e6:.3f} ms of "
          f"kernel time per step")
    for fam, t in ns.most_common():
        print(f"  {fam:24s} {calls[fam] / steps:7.1f} launches/step {t / steps / 1e6:8.3f} ms/step "
              f"{100 * t / total:5.1f} %")


if __name__ == "__main__":
    main()
