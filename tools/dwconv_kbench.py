"""Time the depthwise launches of DeepLabSepASPP with HIP events, interleaved
rounds in ONE process (the method of tools/kbench.py), at batch 4, bf16, on
the maps the KITTI-shaped step runs: 47 x 156 x 512 at rates 6 / 12 / 18 (the
separable ASPP branches) and 94 x 312 x 256 at rate 1 (decoder_conv0 / 1).

    python tools/dwconv_kbench.py [--reps 20] [--rounds 5] [--batch 4]

Per launch and pass (forward, input gradient dx, filter gradient dw): median
and min microseconds, the algorithmic bytes of the pass (x + y, dy + dx, x +
dy: each tensor once) and GB/s against the 6.3 TB/s achievable HBM rate; a
pass whose bytes would take under 5 us at that rate is marked launch-latency-
sized.

Then the yardstick: one ASPP branch both ways, per rate -- the dense atrous
3x3 512 -> 256 conv (forward, input gradient, filter gradient) against the
separable form (depthwise 3x3 + BatchNorm/ReLU on 512 channels + 1x1 512 ->
256, and their gradients); the branch's closing BatchNorm + ReLU on 256
channels is common to both and left out."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import ops  # noqa: E402

HBM_GBS = 6300.0
# (name, H, W, C, rate)
LAUNCHES = [("aspp1", 47, 156, 512, 6), ("aspp2", 47, 156, 512, 12), ("aspp3", 47, 156, 512, 18),
            ("decoder_conv0", 94, 312, 256, 1), ("decoder_conv1", 94, 312, 256, 1)]


def rand(shape, dev, g, dtype=torch.bfloat16, scale=0.5):
    return (torch.randn(shape, device=dev, generator=g) * scale).to(dtype)


def depthwise(N, H, W, C, rate, dev, g):
    d = ops.dwconv_desc(N, H, W, C, C, 3, 3, 1, rate, "SAME", ops.BF16)
    x, dy = rand((N, H, W, C), dev, g), rand((N, H, W, C), dev, g)
    w = torch.randn(3, 3, C, device=dev, generator=g) / 3.0
    y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w)
    ws = torch.empty(ops.dwconv_bwd_filter_workspace(d), dtype=torch.uint8, device=dev)
    return d, {"fwd": lambda: ops.dwconv2d_fwd(d, x, w, y), "dx": lambda: ops.dwconv2d_bwd_data(d, dy, w, dx),
               "dw": lambda: ops.dwconv2d_bwd_filter(d, x, dy, dw, ws)}


def dense(N, H, W, C, K, R, rate, dev, g, ws):
    d = ops.conv_desc(N, H, W, C, K, R, R, 1, rate, "SAME", ops.BF16)
    x, dy = rand((N, H, W, C), dev, g), rand((N, H, W, K), dev, g)
    w32 = torch.randn(R, R, C, K, device=dev, generator=g) / (R * R * C) ** 0.5
    wk = torch.zeros(ops.packed_shape(R, R, C, K, ops.PACK_KRSC, d.C), dtype=torch.bfloat16, device=dev)
    wh = torch.zeros(ops.packed_shape(R, R, C, K, ops.PACK_HWIO, d.C), dtype=torch.bfloat16, device=dev)
    ops.pack_filter(w32, wk, d.C, d.K, ops.PACK_KRSC)
    ops.pack_filter(w32, wh, d.C, d.K, ops.PACK_HWIO)
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w32)
    ws.get(max(ops.conv_workspace(d, o) for o in (ops.OP_FWD, ops.OP_BWD_DATA, ops.OP_BWD_FILTER)))
    return {"fwd": lambda: ops.conv2d_fwd(d, x, wk, y, None, ws), "dx": lambda: ops.conv2d_bwd_data(d, dy, wh, dx, ws),
            "dw": lambda: ops.conv2d_bwd_filter(d, x, dy, dw, ws)}


def bn(N, H, W, C, dev, g, ws):
    x, dy = rand((N, H, W, C), dev, g), rand((N, H, W, C), dev, g)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    return {"fwd": lambda: ops.bn_relu_fwd(x, y, gamma, beta, C, True),
            "bwd": lambda: ops.bn_relu_bwd(x, y, dy, dx, gamma, dg, db, C, True, ws=ws, beta=beta)}


def measure(fns, reps, rounds):
    """{key: [us per launch, one entry per round]}, the keys interleaved within each round."""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) * 1e3 / reps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwconv_kbench: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N = a.batch
    ws = ops.Workspace(dev)

    fns, nbytes = {}, {}
    for name, H, W, C, rate in LAUNCHES:
        _, f = depthwise(N, H, W, C, rate, dev, g)
        for p, fn in f.items():
            fns[(name, p)] = fn
            nbytes[(name, p)] = 2 * N * H * W * C * 2
    t = measure(fns, a.reps, a.rounds)
    print(f"depthwise launches, batch {N}, bf16 ({a.rounds} interleaved rounds x {a.reps} launches)")
    for (name, p), v in t.items():
        med, b = statistics.median(v), nbytes[(name, p)]
        H, W, C, rate = next(l[1:] for l in LAUNCHES if l[0] == name)
        small = "  launch-latency-sized" if b / (HBM_GBS * 1e3) < 5.0 else ""
        print(f"{name:14s} {H}x{W}x{C} rate {rate:<2d} {p:3s} med={med:8.1f}us min={min(v):8.1f}us "
              f"{b / 1e6:6.1f} MB  {b / med / 1e3:7.1f} GB/s = {100 * b / med / 1e3 / HBM_GBS:5.1f}% of {HBM_GBS:.0f}{small}",
              flush=True)

    print("\none ASPP branch 47x156, 512 -> 256: dense atrous 3x3 against depthwise 3x3 + BN/ReLU(512) + 1x1")
    H, W, C, K = 47, 156, 512, 256
    for rate in (6, 12, 18):
        fns = {}
        for p, fn in dense(N, H, W, C, K, 3, rate, dev, g, ws).items():
            fns[("dense", p)] = fn
        for p, fn in depthwise(N, H, W, C, rate, dev, g)[1].items():
            fns[("dw", p)] = fn
        for p, fn in bn(N, H, W, C, dev, g, ws).items():
            fns[("bn", p)] = fn
        for p, fn in dense(N, H, W, C, K, 1, 1, dev, g, ws).items():
            fns[("pw", p)] = fn
        med = {k: statistics.median(v) for k, v in measure(fns, a.reps, a.rounds).items()}
        d_f, d_b = med[("dense", "fwd")], med[("dense", "dx")] + med[("dense", "dw")]
        s_f = med[("dw", "fwd")] + med[("bn", "fwd")] + med[("pw", "fwd")]
        s_b = med[("dw", "dx")] + med[("dw", "dw")] + med[("bn", "bwd")] + med[("pw", "dx")] + med[("pw", "dw")]
        print(f"rate {rate:2d}: dense fwd {d_f:7.1f} dgrad {med[('dense', 'dx')]:7.1f} wgrad {med[('dense', 'dw')]:7.1f} us | "
              f"separable fwd {s_f:7.1f} (dw {med[('dw', 'fwd')]:.1f} + bn {med[('bn', 'fwd')]:.1f} + 1x1 "
              f"{med[('pw', 'fwd')]:.1f}) bwd {s_b:7.1f} (dw dx {med[('dw', 'dx')]:.1f} + dw dw {med[('dw', 'dw')]:.1f} + bn "
              f"{med[('bn', 'bwd')]:.1f} + 1x1 dgrad {med[('pw', 'dx')]:.1f} + wgrad {med[('pw', 'dw')]:.1f}) us | "
              f"dense / separable: fwd {d_f / s_f:.2f}x bwd {d_b / s_b:.2f}x step {(d_f + d_b) / (s_f + s_b):.2f}x",
              flush=True)


if __name__ == "__main__":
    main()
