#!/usr/bin/env python3
"""Bilinear upsampling microbenchmark: the in-tree kernels
(csrc/upsample_bilinear.hip) against the library calls BilinearUpsample
replaces.

    python tools/upsample_bench.py [--iters 20] [--rounds 7] [--json out.json]

Shapes: the two DeepLabV3 calls at the benchmark batch, channels_last bf16,
align_corners=False: the head's 32 x 21 x 32^2 -> 512^2 and the ASPP pool
branch's 32 x 256 x 1^2 -> 32^2. Forward and backward are timed separately:

    in-tree   ext.upsample_bilinear_fwd / _bwd
    library   F.interpolate(mode="bilinear") / aten.upsample_bilinear2d_backward

in the same process, alternating the two round by round, with device events
after a warm-up; the figure is the median of the rounds and the spread is
max - min over them. GB/s is the traffic a direction needs (the small and the
large tensor once each) over the measured time; "floor" is that traffic at
COPY_TBS. The last column is what TFOS_UPSAMPLE=auto must say: in-tree only
if its median is lower than the library's by more than either side's spread.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DIRECTIONS = ("fwd", "bwd")
COPY_TBS = 4.8
# (N, C, Hin, Win, Hout, Wout)
SHAPES = ((32, 21, 32, 32, 512, 512), (32, 256, 1, 1, 32, 32))


def op_bytes(N, C, Hin, Win, Hout, Wout, itemsize=2):
    return N * C * (Hin * Win + Hout * Wout) * itemsize


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def make_calls(ext, N, C, Hin, Win, Hout, Wout, align=False):
    """{direction: (in_tree_fn, library_fn)} on seeded inputs."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    bf, cl = torch.bfloat16, torch.channels_last
    x = torch.randn(N, C, Hin, Win, device="cuda", generator=g).to(bf) \
        .contiguous(memory_format=cl)
    dy = torch.randn(N, C, Hout, Wout, device="cuda", generator=g).to(bf) \
        .contiguous(memory_format=cl)
    return {
        "fwd": (lambda: ext.upsample_bilinear_fwd(x, Hout, Wout, align),
                lambda: F.interpolate(x, size=(Hout, Wout), mode="bilinear",
                                      align_corners=align)),
        "bwd": (lambda: ext.upsample_bilinear_bwd(dy, Hin, Win, align),
                lambda: torch.ops.aten.upsample_bilinear2d_backward(
                    dy, [Hout, Wout], [N, C, Hin, Win], align, None, None)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None,
                    help="also write every round to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upsample_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)

    rows = []
    print("bilinear, channels_last bf16, align_corners=False; ms are medians "
          "of {} rounds of {} calls, +- is max - min".format(
              args.rounds, args.iters))
    print("{:<24s} {:<4s} {:>10s} {:>7s} {:>7s} {:>11s} {:>7s} {:>7s} {:>9s} "
          "{:>8s} {:<8s}".format("shape", "dir", "in-tree ms", "+-", "GB/s",
                                 "library ms", "+-", "GB/s", "floor ms",
                                 "speedup", "auto"))
    for shape in SHAPES:
        calls = make_calls(ext, *shape)
        nbytes = op_bytes(*shape)
        floor = nbytes / (COPY_TBS * 1e9)
        name = "{}x{}x{}x{}->{}x{}".format(*shape)
        for d in DIRECTIONS:
            new, lib = calls[d]
            for _ in range(args.warmup):
                new()
                lib()
            torch.cuda.synchronize()
            t_new, t_lib = [], []
            for _ in range(args.rounds):
                t_new.append(time_ms(new, args.iters))
                t_lib.append(time_ms(lib, args.iters))
            a, b = statistics.median(t_new), statistics.median(t_lib)
            sa, sb = max(t_new) - min(t_new), max(t_lib) - min(t_lib)
            if a > b:
                auto = "library"
            elif b - a <= max(sa, sb):
                auto = "library (inside the spread)"
            else:
                auto = "in-tree"
            rows.append({"shape": list(shape), "dir": d, "in_tree_ms": a,
                         "in_tree_spread_ms": sa, "library_ms": b,
                         "library_spread_ms": sb, "bytes": nbytes,
                         "floor_ms": floor, "in_tree_gbs": nbytes / a / 1e6,
                         "library_gbs": nbytes / b / 1e6, "auto": auto,
                         "in_tree_rounds_ms": t_new,
                         "library_rounds_ms": t_lib})
            print("{:<24s} {:<4s} {:>10.4f} {:>7.4f} {:>7.0f} {:>11.4f} "
                  "{:>7.4f} {:>7.0f} {:>9.4f} {:>7.2f}x {:<8s}".format(
                      name, d, a, sa, nbytes / a / 1e6, b, sb,
                      nbytes / b / 1e6, floor, b / a, auto), flush=True)
        del calls
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
