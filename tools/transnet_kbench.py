"""Time the four TransNet launches (csrc/transnet.hip) with HIP events,
interleaved rounds in ONE process (the method of tools/mbconv_kbench.py), at
batch 4, bf16, on the four maps they run on in a 160 x 576 step of FC-DenseNet
+ TransNet: 40x144x56, 20x72x76, 10x36x110, 5x18x143 (padded to 56 / 80 / 112 /
144 channels).

    python tools/transnet_kbench.py [--reps 20] [--rounds 5] [--batch 4] [--dtype bf16]

Per launch: median, min and max microseconds over the rounds, the algorithmic
bytes of the pass (each tensor once: the modulation forward moves 4 tensors,
its gradient 7, the fusion 3 and 4) and TB/s at the median.  The yardstick on
the same maps, in the same process, is the frozen BatchNorm + ReLU pass
(seg_bn_relu_fwd: 2 tensors, seg_bn_relu_bwd: 3); its own round-to-round spread
(max - min over the rounds, as TB/s) is printed beside it."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticsegmentation_tensorflow_amd import ops  # noqa: E402

MAPS = [("trans1", 40, 144, 56), ("trans2", 20, 72, 76), ("trans3", 10, 36, 110), ("trans4", 5, 18, 143)]


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
        sys.exit("transnet_kbench: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    sdt = {"bf16": ops.BF16, "f16": ops.F16, "f32": ops.F32}[a.dtype]
    tdt = ops.torch_dtype(sdt)
    esz = 4 if sdt == ops.F32 else 2
    N = a.batch
    ws = ops.Workspace(dev)

    def rand(shape):
        return (torch.randn(shape, device=dev, generator=g) * 0.5).to(tdt)

    print(f"TransNet launches of FC-DenseNet + TransNet, batch {N}, {a.dtype} ({a.rounds} interleaved rounds x "
          f"{a.reps} launches); yardstick: seg_bn_relu_fwd / _bwd on the same map")
    for name, H, W, cv in MAPS:
        C = ops.round8(cv)
        alpha, f, beta, dy = (rand((N, H, W, C)) for _ in range(4))
        y, d0, d1, d2 = (torch.empty_like(alpha) for _ in range(4))
        gamma, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        n = N * H * W * C * esz
        fns = {
            ("bn_relu fwd", 2 * n): lambda: ops.bn_relu_fwd(alpha, y, gamma, bt, cv, True),
            ("bn_relu bwd", 3 * n): lambda: ops.bn_relu_bwd(alpha, y, dy, d0, gamma, dg, db, cv, True, ws=ws, beta=bt),
            ("film fwd", 4 * n): lambda: ops.film_fwd(alpha, f, beta, y, cv, 1.0, True),
            ("film bwd", 7 * n): lambda: ops.film_bwd(dy, y, alpha, f, d0, d1, d2, cv, 1.0, True),
            ("axpy fwd", 3 * n): lambda: ops.axpy_relu_fwd(alpha, f, y, cv, 0.1, True),
            ("axpy bwd", 4 * n): lambda: ops.axpy_relu_bwd(dy, y, d0, d1, cv, 0.1, True),
        }
        tt = measure(fns, a.reps, a.rounds)
        med = {k: statistics.median(v) for k, v in tt.items()}
        tbs = {k[0]: k[1] / m / 1e6 for k, m in med.items()}
        spread = {k[0]: k[1] / min(v) / 1e6 - k[1] / max(v) / 1e6 for k, v in tt.items()}
        for (what, b), m in med.items():
            yard = "bn_relu bwd" if what.endswith("bwd") else "bn_relu fwd"
            v = tt[(what, b)]
            tail = (f"spread {spread[what]:5.3f} TB/s" if what.startswith("bn_relu") else
                    f"{tbs[what] - tbs[yard]:+6.3f} TB/s against the yardstick (its spread {spread[yard]:5.3f})")
            print(f"{name} {H:3d}x{W:3d}x{C:<4d} {what:12s} med={m:7.1f}us min={min(v):7.1f}us max={max(v):7.1f}us "
                  f"{b / 1e6:7.2f} MB {tbs[what]:6.3f} TB/s  {tail}", flush=True)


if __name__ == "__main__":
    main()
