#!/usr/bin/env python3
"""Transposed-conv weight-gradient microbenchmark: csrc/convt_wrw.hip against
the library call it replaces, on the four U-Net up-stack layers.

    python tools/convt_wrw_bench.py [--batches 64,1024] [--iters 20]
                                    [--rounds 7] [--json out.json]

Shapes: UpBlock.up of UNetMobileNet at a 128 x 128 image, ConvTranspose2d(cin,
cout, 4, stride=2, padding=1) without bias, channels_last bf16:

    in-tree   ext.convt_wrw(dy, x), fp32 dW
    library   aten.convolution_backward on the bf16 weight, weight mask only

in the same process, alternating the two round by round, with device events
after a warm-up; the figure is the median of the rounds and the spread is
max - min over them. "floor" is the bytes of x, dy and dW at COPY_TBS, the
middle of the device-copy rates in docs/performance.md. The last column is
what a row of TFOS_CONVT_WRW=auto's table may say: in-tree only if its median
was no higher than the library's, and the library where the difference is
inside the library's own spread.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

COPY_TBS = 4.8
#: (layer, Cin, Cout, side of the input map)
LAYERS = (("up1", 320, 512, 4), ("up2", 608, 256, 8), ("up3", 288, 128, 16),
          ("up4", 152, 64, 32))


def op_bytes(N, cin, cout, H, W):
    return (N * cin * H * W + N * cout * 4 * H * W) * 2 + cin * cout * 16 * 4


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def make_calls(ext, N, cin, cout, H, W):
    """(in_tree_fn, library_fn) on seeded inputs."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    bf, cl = torch.bfloat16, torch.channels_last
    x = torch.randn(N, cin, H, W, device="cuda", generator=g).to(bf) \
        .contiguous(memory_format=cl)
    dy = torch.randn(N, cout, 2 * H, 2 * W, device="cuda", generator=g) \
        .to(bf).contiguous(memory_format=cl)
    w = (torch.randn(cin, cout, 4, 4, device="cuda", generator=g) / 4).to(bf) \
        .contiguous(memory_format=cl)
    return (lambda: ext.convt_wrw(dy, x),
            lambda: torch.ops.aten.convolution_backward(
                dy, x, w, None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1,
                [False, True, False]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None,
                    help="also write every round to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("convt_wrw_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)

    rows = []
    print("ConvTranspose2d(cin, cout, 4, 2, 1) weight gradient; ms are medians "
          "of {} rounds of {} calls, +- is max - min".format(
              args.rounds, args.iters))
    print("{:>5s} {:<5s} {:>9s} {:>5s} {:>6s} {:>10s} {:>7s} {:>11s} {:>7s} "
          "{:>9s} {:>8s} {:<8s}".format(
              "N", "layer", "cin>cout", "side", "slabs", "in-tree ms", "+-",
              "library ms", "+-", "floor ms", "speedup", "auto"))
    for N in [int(v) for v in args.batches.split(",")]:
        for layer, cin, cout, side in LAYERS:
            new, lib = make_calls(ext, N, cin, cout, side, side)
            plan = ext.convt_wrw_plan(N, side, side, cin, cout)
            nbytes = op_bytes(N, cin, cout, side, side)
            floor = nbytes / (COPY_TBS * 1e9)
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
            elif b - a <= sb:
                auto = "library (inside its spread)"
            else:
                auto = "in-tree"
            rows.append({"N": N, "layer": layer, "Cin": cin, "Cout": cout,
                         "H": side, "W": side, "plan": dict(plan),
                         "in_tree_ms": a, "in_tree_spread_ms": sa,
                         "library_ms": b, "library_spread_ms": sb,
                         "bytes": nbytes, "floor_ms": floor, "auto": auto,
                         "in_tree_rounds_ms": t_new,
                         "library_rounds_ms": t_lib})
            print("{:>5d} {:<5s} {:>9s} {:>5d} {:>6d} {:>10.4f} {:>7.4f} "
                  "{:>11.4f} {:>7.4f} {:>9.4f} {:>7.2f}x {:<8s}".format(
                      N, layer, "{}>{}".format(cin, cout), side,
                      plan["slabs"], a, sa, b, sb, floor, b / a, auto),
                  flush=True)
            del new, lib
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
