"""Time the MBConvBlock launches of EfficientSeg('b0') with HIP events,
interleaved rounds in ONE process (the method of tools/kbench.py), at batch 4,
bf16, on the maps of a 160 x 576 step: BatchNorm + swish forward / backward
(seg_bn_act_*), the squeeze (seg_se_squeeze and, where it accepts the width,
seg_spatial_reduce), the excite forward / backward (seg_se_excite_*), and the
5 x 5 depthwise convs at stride 1 and 2 (dw_gather_k<T,0,0>).

    python tools/mbconv_kbench.py [--reps 20] [--rounds 5] [--batch 4] [--dtype bf16]

Per launch: median and min microseconds, the algorithmic bytes of the pass
(each tensor once: x + y, x + dy + dx, x, ...) and TB/s.  The yardstick on the
same bytes is the frozen BatchNorm + ReLU pass (seg_bn_relu_fwd / _bwd); the
last column is the launch's time over the yardstick's (forward passes and the
squeeze against bn_relu fwd, backward passes against bn_relu bwd)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import ops  # noqa: E402

# the depthwise outputs of B0's blocks at 160 x 576: (block, H, W, expanded channels)
MAPS = [("1a", 80, 288, 32), ("2a", 40, 144, 96), ("2b", 40, 144, 144), ("3a", 20, 72, 144), ("3b", 20, 72, 240),
        ("4a", 10, 36, 240), ("4b", 10, 36, 480), ("5a", 10, 36, 480), ("5b", 10, 36, 672), ("6a", 5, 18, 672),
        ("6b", 5, 18, 1344), ("7a", 5, 18, 1152), ("2a expand_bn", 80, 288, 96)]
# the 5 x 5 depthwise convs: (block, input H, W, channels, stride)
DW5 = [("3a", 40, 144, 144, 2), ("3b", 20, 72, 240, 1), ("5a", 10, 36, 480, 1), ("5b", 10, 36, 672, 1),
       ("6a", 10, 36, 672, 2), ("6b", 5, 18, 1344, 1)]


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
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mbconv_kbench: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    sdt = {"bf16": ops.BF16, "f16": ops.F16, "f32": ops.F32}[a.dtype]
    tdt = ops.torch_dtype(sdt)
    esz = 4 if sdt == ops.F32 else 2
    N = a.batch
    ws = ops.Workspace(dev)

    def rand(shape, scale=0.5):
        return (torch.randn(shape, device=dev, generator=g) * scale).to(tdt)

    print(f"MBConv launches of EfficientSeg('b0'), batch {N}, {a.dtype} ({a.rounds} interleaved rounds x {a.reps} "
          f"launches); yardstick: seg_bn_relu_fwd / _bwd on the same map")
    for name, H, W, C in MAPS:
        x, dy = rand((N, H, W, C)), rand((N, H, W, C))
        y, dx = torch.empty_like(x), torch.empty_like(x)
        s = torch.rand((N, 1, 1, C), device=dev, generator=g).to(tdt)
        sq, ds = torch.empty_like(s), torch.empty_like(s)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        n = N * H * W * C * esz
        fns = {
            ("bn_relu fwd", 2 * n): lambda: ops.bn_relu_fwd(x, y, gamma, beta, C, True),
            ("bn_relu bwd", 3 * n): lambda: ops.bn_relu_bwd(x, y, dy, dx, gamma, dg, db, C, True, ws=ws, beta=beta),
            ("bn_swish fwd", 2 * n): lambda: ops.bn_act_fwd(x, y, gamma, beta, C, "swish"),
            ("bn_swish bwd", 3 * n): lambda: ops.bn_act_bwd(x, dy, dx, gamma, beta, dg, db, C, "swish", ws=ws),
            ("se_squeeze", n): lambda: ops.se_squeeze(x, sq, C, 1.0 / (H * W), ws),
            ("excite fwd", 2 * n): lambda: ops.se_excite_fwd(x, s, y, C),
            ("excite bwd", 3 * n): lambda: ops.se_excite_bwd(x, s, dy, dx, ds, C, ws),
        }
        if ops.spatial_reduce_fits(C, sdt):
            fns[("spatial_reduce", n)] = lambda: ops.spatial_reduce(x, sq, 1.0 / (H * W), ws)
        tt = measure(fns, a.reps, a.rounds)
        t = {k: statistics.median(v) for k, v in tt.items()}
        ref = {k[0]: v for k, v in t.items()}
        for (what, b), med in t.items():
            yard = ref["bn_relu bwd"] if what.endswith("bwd") else ref["bn_relu fwd"]
            print(f"{name:14s} {H:3d}x{W:3d}x{C:<4d} {what:14s} med={med:7.1f}us min={min(tt[(what, b)]):7.1f}us "
                  f"{b / 1e6:7.2f} MB {b / med / 1e6:6.3f} TB/s  x{med / yard:5.2f} of the yardstick", flush=True)

    print(f"\n5 x 5 depthwise convs (dw_gather_k<T,0,0>), batch {N}, {a.dtype}: bytes = input + output of the pass")
    for name, H, W, C, stride in DW5:
        d = ops.dwconv_desc(N, H, W, C, C, 5, 5, stride, 1, "SAME", sdt)
        x, dy = rand((N, H, W, C)), rand((N, d.OH, d.OW, C))
        w = torch.randn(5, 5, C, device=dev, generator=g) / 5.0
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        wsb = torch.empty(max(256, ops.dwconv_bwd_filter_workspace(d)), dtype=torch.uint8, device=dev)
        b = (x.numel() + dy.numel()) * esz
        fns = {"fwd": lambda: ops.dwconv2d_fwd(d, x, w, y), "dx": lambda: ops.dwconv2d_bwd_data(d, dy, w, dx),
               "dw": lambda: ops.dwconv2d_bwd_filter(d, x, dy, dw, wsb)}
        for p, v in measure(fns, a.reps, a.rounds).items():
            med = statistics.median(v)
            print(f"{name:3s} {H:3d}x{W:3d}x{C:<4d} 5x5 stride {stride} {p:3s} med={med:7.1f}us min={min(v):7.1f}us "
                  f"{b / 1e6:7.2f} MB {b / med / 1e6:6.3f} TB/s", flush=True)


if __name__ == "__main__":
    main()
