#!/usr/bin/env python3
"""Softmax cross-entropy microbenchmark: the in-tree dense kernels against the
library composition they replace, forward + backward, per workload shape.

    python tools/xent_bench.py [--iters 20] [--rounds 5]

Shapes: the U-Net (b64 x 3 x 128^2) and DeepLabV3 (b32 x 21 x 512^2) logits in
bf16, in both memory layouts, and a (1024, 1000) classifier head. For each,
``softmax_cross_entropy(logits, y)`` is timed against

    flat = logits.permute(0, 2, 3, 1).reshape(-1, C)
    F.cross_entropy(flat.float(), y.reshape(-1))

in the same process, alternating between the two round by round, with device
events after a warm-up. GB/s is the minimal traffic of the op (logits read in
forward and backward, dlogits written, targets and lse) over the measured
time, so the composition's figure is what it achieves on the same useful
bytes, not on the bytes it actually moves.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("xent_bench needs a GPU")
    from tensorflowonspark_amd.ops import get_ext
    from tensorflowonspark_amd.ops.modules import softmax_cross_entropy
    get_ext(required=True)

    cases = [
        ("unet b64x3x128^2", (64, 3, 128, 128), "nchw"),
        ("unet b64x3x128^2", (64, 3, 128, 128), "nhwc"),
        ("deeplab b32x21x512^2", (32, 21, 512, 512), "nchw"),
        ("deeplab b32x21x512^2", (32, 21, 512, 512), "nhwc"),
        ("head 1024x1000", (1024, 1000), "2d"),
    ]
    print("{:<22s} {:<5s} {:>10s} {:>9s} {:>12s} {:>9s} {:>8s}".format(
        "shape", "lay", "new ms", "GB/s", "library ms", "GB/s", "speedup"))
    for name, shape, layout in cases:
        c = shape[1]
        x = torch.randn(*shape, device="cuda").mul_(3).to(torch.bfloat16)
        if layout == "nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, c, shape[:1] + shape[2:], device="cuda")
        leaf = x.requires_grad_()
        p = y.numel()
        nbytes = 3 * p * c * x.element_size() + 2 * p * 8 + 2 * p * 4

        def new():
            leaf.grad = None
            softmax_cross_entropy(leaf, y).backward()

        def library():
            leaf.grad = None
            flat = leaf.permute(0, 2, 3, 1).reshape(-1, c) \
                if leaf.dim() == 4 else leaf
            F.cross_entropy(flat.float(), y.reshape(-1)).backward()

        for _ in range(args.warmup):
            new()
            library()
        torch.cuda.synchronize()
        t_new, t_lib = [], []
        for _ in range(args.rounds):
            t_new.append(time_ms(new, args.iters))
            t_lib.append(time_ms(library, args.iters))
        a, b = statistics.median(t_new), statistics.median(t_lib)
        print("{:<22s} {:<5s} {:>10.3f} {:>9.0f} {:>12.3f} {:>9.0f} {:>7.2f}x"
              .format(name, layout, a, nbytes / a / 1e6, b, nbytes / b / 1e6,
                      b / a), flush=True)
        del leaf, x, y


if __name__ == "__main__":
    main()
