#!/usr/bin/env python3
"""Pointwise 1x1 conv microbenchmark: the in-tree kernels (csrc/pwconv.hip,
and conv_wrw2 for the weight gradient) against the library calls
PointwiseConv replaces, per layer and direction.

    python tools/pw_bench.py [--batches 64,1024] [--iters 20] [--rounds 7]
                             [--json out.json]

Shapes: every distinct pointwise layer (Cin, Cout, H) of unet_mobilenet on a
128 x 128 input, read off the model with forward hooks, at each batch size.
For each, forward, dgrad and wrw are timed separately on channels_last bf16:

    in-tree   ext.pwconv_fwd / pwconv_dgrad on the fp32 weight; for wrw
              ext.conv_wrw2(dy, x, 1, 1, 1, 0) ('wrw2')
    library   F.conv2d(x, w.to(bf16)), weight cast included, and
              aten.convolution_backward with an output mask of one

in the same process, alternating the candidates round by round, with device
events after a warm-up per shape; the figures are the median of the rounds
and their spread (max - min). GB/s is the traffic the op needs, computed from
the shapes (fwd: x + y, dgrad: dy + dx, wrw: dy + x, each plus the weight),
over the measured time; "floor" is those bytes at 4.8 TB/s. The last column is
what TFOS_PW=auto must say for the pair: an in-tree candidate only if its
median was no slower than the library's in this run, and of two the faster.
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
HBM_BYTES_PER_S = 4.8e12


def unet_pointwise_layers(size=128):
    """[(cin, cout, H, W, count)] of the pointwise convs of unet_mobilenet on
    a size x size input, in model order, duplicates merged."""
    from tensorflowonspark_amd.models import unet_mobilenet
    from tensorflowonspark_amd.ops.modules import PointwiseConv
    model = unet_mobilenet().eval()
    seen = []

    def hook(mod, args):
        x = args[0]
        seen.append((mod.in_channels, mod.out_channels, x.shape[2], x.shape[3]))

    handles = [m.register_forward_pre_hook(hook) for m in model.modules()
               if isinstance(m, PointwiseConv)]
    with torch.no_grad():
        model(torch.zeros(1, 3, size, size))
    for h in handles:
        h.remove()
    out = []
    for s in seen:
        if s not in [o[:4] for o in out]:
            out.append(s + (seen.count(s),))
    return out


def op_bytes(N, cin, cout, H, W, direction):
    """Bytes one direction has to move: the two bf16 activations it touches
    and the weight (read as fp32 by forward and dgrad, written as fp32 by
    wrw)."""
    M = N * H * W
    return 2 * M * (cin + cout) + 4 * cin * cout


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
    """{direction: {candidate: fn}} on seeded inputs; 'lib' is the library."""
    bf16, cl = torch.bfloat16, torch.channels_last
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(N, cin, H, W, device="cuda", generator=g).to(bf16) \
        .contiguous(memory_format=cl)
    dy = torch.randn(N, cout, H, W, device="cuda", generator=g).to(bf16) \
        .contiguous(memory_format=cl)
    w = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) / 4

    def lib_bwd(mask):
        return torch.ops.aten.convolution_backward(
            dy, x, w.to(bf16), None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            mask)

    wrw = {"wrw2": lambda: ext.conv_wrw2(dy, x, 1, 1, 1, 0),
           "lib": lambda: lib_bwd([False, True, False])}
    return {
        "fwd": {"hip": lambda: ext.pwconv_fwd(x, w),
                "lib": lambda: F.conv2d(x, w.to(bf16))},
        "dgrad": {"hip": lambda: ext.pwconv_dgrad(dy, w),
                  "lib": lambda: lib_bwd([True, False, False])},
        "wrw": wrw,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None,
                    help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pw_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)

    layers = unet_pointwise_layers()
    rows = []
    print("x = how many of the {} layers have this shape; ms are medians of "
          "{} rounds of {} calls, +- is max - min".format(
              sum(l[4] for l in layers), args.rounds, args.iters))
    print("{:>5s} {:>4s} {:>4s} {:>3s} {:>2s} {:<6s} {:<5s} {:>9s} {:>8s} "
          "{:>7s} {:>9s} {:>8s} {:>9s} {:<5s}".format(
              "N", "cin", "cout", "H", "x", "dir", "cand", "ms", "+-", "GB/s",
              "lib ms", "+-", "floor ms", "auto"))
    for N in [int(b) for b in args.batches.split(",")]:
        for cin, cout, H, W, count in layers:
            calls = make_calls(ext, N, cin, cout, H, W)
            for d in DIRECTIONS:
                cands = calls[d]
                for _ in range(args.warmup):
                    for fn in cands.values():
                        fn()
                torch.cuda.synchronize()
                times = {c: [] for c in cands}
                for _ in range(args.rounds):
                    for c, fn in cands.items():
                        times[c].append(time_ms(fn, args.iters))
                med = {c: statistics.median(t) for c, t in times.items()}
                spread = {c: max(t) - min(t) for c, t in times.items()}
                nbytes = op_bytes(N, cin, cout, H, W, d)
                best = min((c for c in cands if c != "lib"), key=med.get)
                auto = best if med[best] <= med["lib"] else "lib"
                for c in cands:
                    if c == "lib":
                        continue
                    rows.append({
                        "N": N, "cin": cin, "cout": cout, "H": H, "W": W,
                        "count": count, "dir": d, "cand": c, "ms": med[c],
                        "spread_ms": spread[c], "library_ms": med["lib"],
                        "library_spread_ms": spread["lib"], "bytes": nbytes,
                        "gbs": nbytes / med[c] / 1e6,
                        "floor_ms": nbytes / HBM_BYTES_PER_S * 1e3,
                        "auto": auto})
                    print("{:>5d} {:>4d} {:>4d} {:>3d} {:>2d} {:<6s} {:<5s} "
                          "{:>9.4f} {:>8.4f} {:>7.0f} {:>9.4f} {:>8.4f} "
                          "{:>9.4f} {:<5s}".format(
                              N, cin, cout, H, count, d, c, med[c], spread[c],
                              nbytes / med[c] / 1e6, med["lib"],
                              spread["lib"], nbytes / HBM_BYTES_PER_S * 1e3,
                              auto), flush=True)
            del calls
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
