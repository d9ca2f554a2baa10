#!/usr/bin/env python3
"""Transposed-conv head microbenchmark: the in-tree kernels
(csrc/convt_head.hip) against the library calls ConvTranspose2dHead replaces.

    python tools/convt_head_bench.py [--batches 64,1024] [--iters 20]
                                     [--rounds 7] [--json out.json]

Shape: the U-Net head, ConvTranspose2d(80, 3, 4, stride=2, padding=1) with a
bias on the 64 x 64 map a 128 x 128 input leaves, at each batch size.
Forward, dgrad and wrw (weight and bias gradient together) are timed
separately on channels_last bf16:

    in-tree   ext.convt_head_fwd / _dgrad / _wrw on the fp32 weight and bias
    library   F.conv_transpose2d with the bf16 casts of weight and bias
              included; aten.convolution_backward with an output mask of one
              (wrw: weight and bias together)

in the same process, alternating the two round by round, with device events
after a warm-up; the figure is the median of the rounds and the spread is
max - min over them. GB/s is the traffic the direction needs (fwd: x + y,
dgrad: dy + dx, wrw: dy + x) over the measured time; "floor" is that traffic
at COPY_TBS, the middle of the device-copy rates in docs/performance.md. The
last column is what TFOS_CONVT_HEAD=auto must say: in-tree only if its median
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
import torch.nn.functional as F  # noqa: E402

DIRECTIONS = ("fwd", "dgrad", "wrw")
COPY_TBS = 4.8
CIN, COUT, SIDE = 80, 3, 64


def op_bytes(N, cin, cout, H, W, itemsize=2):
    """Bytes one direction has to move: the N x cin x H x W tensor and the
    N x cout x 2H x 2W one (the weight is noise next to them)."""
    return (N * cin * H * W + N * cout * 4 * H * W) * itemsize


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def make_calls(ext, N, cin=CIN, cout=COUT, H=SIDE, W=SIDE):
    """{direction: (in_tree_fn, library_fn)} on seeded inputs."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    bf, cl = torch.bfloat16, torch.channels_last
    x = torch.randn(N, cin, H, W, device="cuda", generator=g).to(bf) \
        .contiguous(memory_format=cl)
    dy = torch.randn(N, cout, 2 * H, 2 * W, device="cuda", generator=g) \
        .to(bf).contiguous(memory_format=cl)
    w = torch.randn(cin, cout, 4, 4, device="cuda", generator=g) / 4
    b = torch.randn(cout, device="cuda", generator=g)

    def lib_bwd(mask):
        return torch.ops.aten.convolution_backward(
            dy, x, w.to(bf), [cout], [2, 2], [1, 1], [1, 1], True, [0, 0], 1,
            mask)

    return {
        "fwd": (lambda: ext.convt_head_fwd(x, w, b),
                lambda: F.conv_transpose2d(x, w.to(bf), b.to(bf), 2, 1)),
        "dgrad": (lambda: ext.convt_head_dgrad(dy, w, H, W),
                  lambda: lib_bwd([True, False, False])),
        "wrw": (lambda: ext.convt_head_wrw(dy, x),
                lambda: lib_bwd([False, True, True])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--library-only", action="store_true",
                    help="time the library side alone (what the head costs "
                    "before any kernel exists)")
    ap.add_argument("--json", default=None,
                    help="also write every round to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("convt_head_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)

    rows = []
    print("ConvTranspose2d({}, {}, 4, 2, 1) on {} x {}; ms are medians of {} "
          "rounds of {} calls, +- is max - min".format(
              CIN, COUT, SIDE, SIDE, args.rounds, args.iters))
    print("{:>5s} {:<6s} {:>10s} {:>7s} {:>7s} {:>11s} {:>7s} {:>7s} {:>9s} "
          "{:>8s} {:<8s}".format("N", "dir", "in-tree ms", "+-", "GB/s",
                                 "library ms", "+-", "GB/s", "floor ms",
                                 "speedup", "auto"))
    for N in [int(v) for v in args.batches.split(",")]:
        calls = make_calls(ext, N)
        nbytes = op_bytes(N, CIN, COUT, SIDE, SIDE)
        floor = nbytes / (COPY_TBS * 1e9)
        for d in DIRECTIONS:
            new, lib = calls[d]
            if args.library_only:
                new = lib
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
            rows.append({"N": N, "Cin": CIN, "Cout": COUT, "H": SIDE,
                         "W": SIDE, "dir": d, "in_tree_ms": a,
                         "in_tree_spread_ms": sa, "library_ms": b,
                         "library_spread_ms": sb, "bytes": nbytes,
                         "floor_ms": floor, "in_tree_gbs": nbytes / a / 1e6,
                         "library_gbs": nbytes / b / 1e6, "auto": auto,
                         "in_tree_rounds_ms": t_new,
                         "library_rounds_ms": t_lib,
                         "library_only": args.library_only})
            print("{:>5d} {:<6s} {:>10.4f} {:>7.4f} {:>7.0f} {:>11.4f} "
                  "{:>7.4f} {:>7.0f} {:>9.4f} {:>7.2f}x {:<8s}".format(
                      N, d, a, sa, nbytes / a / 1e6, b, sb, nbytes / b / 1e6,
                      floor, b / a, auto), flush=True)
        del calls
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
