"""Time the strided Conv2DBackpropInput of LidCamNet's conv3 / conv5 (4x4
stride 2, batch 4 at 160 x 576) on its two routes -- dgrad_s2 (one dy halo
per tile) and the phase GEMMs of seg_tconv2d_fwd -- alone, with HIP events,
alternating the routes round by round in ONE process.

    python tools/dgrad_s2_bench.py [--reps 200] [--rounds 9] [--batch 4]

Per shape, dtype and route: the median, min and max over rounds of the mean
launch time (us), i.e. the route's own run-to-run spread, TF/s at the median,
and the largest difference between the two routes' outputs (same inputs)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import ops  # noqa: E402

# name: (H, W, C, K) of the conv whose input gradient is timed (dx is [N, H, W, C])
SHAPES = {"conv3": (80, 288, 32, 64), "conv5": (40, 144, 64, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dgrad_s2_bench: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    ws = ops.Workspace(dev)
    for tdt, sdt, tag in ((torch.bfloat16, ops.BF16, "bf16"), (torch.float16, ops.F16, "f16")):
        for name, (H, W, C, K) in SHAPES.items():
            N = a.batch
            d = ops.conv_desc(N, H, W, C, K, 4, 4, 2, 1, "SAME", sdt)
            assert ops.conv2d_bwd_data_s2_ok(d), name
            g = torch.Generator(device=dev).manual_seed(1)
            dy = (torch.randn(N, d.OH, d.OW, d.K, device=dev, generator=g) * 0.5).to(tdt)
            w32 = torch.randn(4, 4, C, K, device=dev, generator=g) / (16 * C) ** 0.5
            wh = torch.zeros(ops.packed_shape(4, 4, C, K, ops.PACK_HWIO), dtype=tdt, device=dev)
            ops.pack_filter(w32, wh, d.C, d.K, ops.PACK_HWIO)
            out = {1: torch.empty(N, H, W, d.C, dtype=tdt, device=dev), 0: torch.empty(N, H, W, d.C, dtype=tdt, device=dev)}
            names, times = {}, {1: [], 0: []}
            for on in (1, 0):                      # warm both routes
                ops.set_option("dgrad_s2", on)
                names[on] = ops.conv_kernel_info(d, ops.OP_BWD_DATA)[0]
                for _ in range(20):
                    ops.conv2d_bwd_data(d, dy, wh, out[on], ws)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for on in (1, 0):
                    ops.set_option("dgrad_s2", on)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        ops.conv2d_bwd_data(d, dy, wh, out[on], ws)
                    e1.record()
                    torch.cuda.synchronize()
                    times[on].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            ops.set_option("dgrad_s2", 1)
            diff = (out[1].float() - out[0].float()).abs().max().item() / out[0].float().abs().max().item()
            flops = ops.conv_kernel_info(d, ops.OP_BWD_DATA)[2]
            for on in (1, 0):
                t = times[on]
                med = statistics.median(t)
                print(f"{name} N={N} {tag} {names[on]:28s} median {med:8.2f} us  min {min(t):8.2f}  max {max(t):8.2f}  "
                      f"spread {(max(t) - min(t)) / med * 100:5.1f} %  {flops / med * 1e-6:7.2f} TF/s")
            r = statistics.median(times[1]) / statistics.median(times[0])
            print(f"{name} N={N} {tag} dgrad_s2 / fallback = {r:.3f}   max |difference| / max |dx| = {diff:.2e}")


if __name__ == "__main__":
    main()
