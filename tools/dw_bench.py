#!/usr/bin/env python3
"""Depthwise 3x3 microbenchmark: the in-tree kernels (csrc/dwconv3x3.hip)
against the library calls DepthwiseConv3x3 replaces, per layer and direction.

    python tools/dw_bench.py [--batches 64,1024] [--iters 20] [--rounds 5]
                             [--json out.json]

Shapes: every distinct depthwise layer (C, H, stride) of unet_mobilenet on a
128 x 128 input, read off the model with forward hooks, at each batch size.
For each, forward, dgrad and wrw are timed separately on channels_last bf16:

    in-tree   ext.dwconv3x3_fwd / _dgrad / _wrw on the fp32 weight
    library   F.conv2d(x, w.to(bf16), groups=C), weight cast included, and
              aten.convolution_backward with an output mask of one

in the same process, alternating the two round by round, with device events
after a warm-up per shape; the figure is the median of the rounds. GB/s is the
traffic the op needs, computed from the shapes (fwd: x + y, dgrad: dy + dx,
wrw: dy + x), over the measured time. The last column is what TFOS_DW=auto
must say for the pair: in-tree only if it was no slower than the library in
this run.
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


def unet_depthwise_layers(size=128):
    """[(C, H, W, stride, count)] of the depthwise convs of unet_mobilenet
    on a size x size input, in model order, duplicates merged."""
    from tensorflowonspark_amd.models import unet_mobilenet
    from tensorflowonspark_amd.ops.modules import DepthwiseConv3x3
    model = unet_mobilenet().eval()
    seen = []

    def hook(mod, args):
        x = args[0]
        seen.append((mod.in_channels, x.shape[2], x.shape[3], mod.stride[0]))

    handles = [m.register_forward_pre_hook(hook) for m in model.modules()
               if isinstance(m, DepthwiseConv3x3)]
    with torch.no_grad():
        model(torch.zeros(1, 3, size, size))
    for h in handles:
        h.remove()
    out = []
    for s in seen:
        if s not in [o[:4] for o in out]:
            out.append(s + (seen.count(s),))
    return out


def op_bytes(N, C, H, W, stride, itemsize):
    """Bytes one direction has to move. All three move the same two
    tensors, the H x W one and the Ho x Wo one: forward x + y, dgrad
    dy + dx, wrw dy + x (the 9*C weights are noise next to them)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    big, small = N * C * H * W * itemsize, N * C * Ho * Wo * itemsize
    return big + small


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def make_calls(ext, N, C, H, W, stride, dtype=torch.bfloat16):
    """{direction: (in_tree_fn, library_fn)} on seeded inputs."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(N, C, H, W, device="cuda", generator=g).to(dtype) \
        .contiguous(memory_format=torch.channels_last)
    w = torch.randn(C, 1, 3, 3, device="cuda", generator=g) / 3
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, C, Ho, Wo, device="cuda", generator=g).to(dtype) \
        .contiguous(memory_format=torch.channels_last)
    s2, p2, d2, z2 = [stride, stride], [1, 1], [1, 1], [0, 0]

    def lib_bwd(mask):
        return torch.ops.aten.convolution_backward(
            dy, x, w.to(dtype), None, s2, p2, d2, False, z2, C, mask)

    return {
        "fwd": (lambda: ext.dwconv3x3_fwd(x, w, stride),
                lambda: F.conv2d(x, w.to(dtype), None, stride, 1, 1, C)),
        "dgrad": (lambda: ext.dwconv3x3_dgrad(dy, w, stride, H, W),
                  lambda: lib_bwd([True, False, False])),
        "wrw": (lambda: ext.dwconv3x3_wrw(dy, x, stride),
                lambda: lib_bwd([False, True, False])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None,
                    help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dw_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)

    layers = unet_depthwise_layers()
    rows = []
    print("s = stride, x = how many of the 17 layers have this shape")
    print("{:>5s} {:>4s} {:>4s} {:>2s} {:>2s} {:<6s} {:>10s} {:>8s} "
          "{:>11s} {:>8s} {:>8s} {:<8s}".format(
              "N", "C", "H", "s", "x", "dir", "in-tree ms", "GB/s",
              "library ms", "GB/s", "speedup", "auto"))
    for N in [int(b) for b in args.batches.split(",")]:
        for C, H, W, stride, count in layers:
            calls = make_calls(ext, N, C, H, W, stride)
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
                nbytes = op_bytes(N, C, H, W, stride, 2)
                auto = "in-tree" if a <= b else "library"
                rows.append({"N": N, "C": C, "H": H, "W": W, "stride": stride,
                             "count": count, "dir": d, "in_tree_ms": a,
                             "library_ms": b, "bytes": nbytes,
                             "in_tree_gbs": nbytes / a / 1e6,
                             "library_gbs": nbytes / b / 1e6, "auto": auto})
                print("{:>5d} {:>4d} {:>4d} {:>2d} {:>2d} {:<6s} {:>10.4f} "
                      "{:>8.0f} {:>11.4f} {:>8.0f} {:>7.2f}x {:<8s}".format(
                          N, C, H, stride, count, d, a, nbytes / a / 1e6, b,
                          nbytes / b / 1e6, b / a, auto), flush=True)
            del calls
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
