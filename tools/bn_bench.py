#!/usr/bin/env python3
"""Per-shape, per-kernel bandwidth of the NHWC fast-path BatchNorm kernels.

The four kernel families of csrc/bn_relu.hip (stats, apply, bwd stats, bwd dx)
are launched one at a time through ``bn_stage`` on preallocated tensors and
timed with device events: per round, ``--iters`` back-to-back launches between
two events; the figure reported is the median over ``--rounds`` rounds. The
numerator of TB/s is the bytes the launch really moves: every activation
stream it reads or writes, the mask bytes and the fp32 partials. Each shape
starts with a ``(copy)`` row, a plain device copy of the same tensor (1 read +
1 write), as the yardstick of what a streaming kernel reaches on the machine
at hand.

    python tools/bn_bench.py --batch 1024
    python tools/bn_bench.py --batch 1024 --ext parent=/path/to/tfosr_hip_ops_parent.so

``--ext NAME=PATH`` (repeatable) loads further builds of the extension next to
the in-tree one and alternates all of them inside every round, shape by shape,
so that drift hits each build alike. Such a build needs a module name of its
own, equal to its file name (compile bindings.cpp with
``-DTORCH_EXTENSION_NAME=tfosr_hip_ops_parent`` for the example above), and
``bn_stage``: for an older commit, compile its csrc/bn_relu.hip with this
commit's csrc/bindings.cpp.

``--epilogue`` is a different table: per forward (conv, BN) pair of ResNet-50,
the conv kernel followed by the statistics pass against the conv kernel with
the statistics epilogue followed by the tile merge (see ``epilogue_main``); it
is what the ``TFOS_BN_EPI=auto`` rule in ops/modules.py was read off.

The variants timed are the ones the ResNet-50 step runs most: stats; apply
with ReLU (and with ReLU + residual, ``apply+res``); bwd stats with the mask
(and writing the gated gradient, ``bwd stats+g``); bwd dx with the mask.
"""

import argparse
import importlib.util
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

# ResNet-50 BN shapes (C, H=W)
RESNET50 = [(64, 112), (64, 56), (256, 56), (128, 56), (128, 28),
            (512, 28), (256, 28), (256, 14), (1024, 14), (512, 14),
            (512, 7), (2048, 7)]

KERNELS = ["stats", "apply", "apply+res", "bwd stats", "bwd stats+g", "bwd dx"]

COPY_TBS = 6.3   # streaming-copy bandwidth of the part, TB/s


def load_ext(path):
    name = os.path.basename(path).split(".")[0]
    if name == "tfosr_hip_ops":
        raise SystemExit("{}: pybind11 hands back the module already loaded "
                         "under a name; build the other extension as, say, "
                         "tfosr_hip_ops_parent.so".format(path))
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not hasattr(mod, "bn_stage"):
        raise SystemExit("{}: no bn_stage; build it with this commit's "
                         "csrc/bindings.cpp".format(path))
    return mod


def bytes_moved(kernel, numel, esize, nvec, nb, C):
    """Bytes one launch reads plus writes."""
    t = numel * esize
    part = nb * 2 * C * 4
    return {
        "stats": t + part,
        "apply": 2 * t + nvec,
        "apply+res": 3 * t + nvec,
        "bwd stats": 2 * t + nvec + part,
        "bwd stats+g": 3 * t + nvec + part,
        "bwd dx": 3 * t + nvec,
    }[kernel]


def make_calls(ext, t):
    """kernel name -> zero-argument launch, for one extension build."""
    x, res, dy, out, mask, ws = (t["x"], t["res"], t["dy"], t["out"],
                                 t["mask"], t["ws"])
    mean, rstd, w, b, dg, db = (t["mean"], t["rstd"], t["w"], t["b"],
                                t["dg"], t["db"])
    st = ext.bn_stage
    return {
        "stats": lambda: st(0, x, None, None, None, ws, [], False),
        "apply": lambda: st(1, x, None, out, mask, ws, [mean, rstd, w, b],
                            True),
        "apply+res": lambda: st(1, x, res, out, mask, ws, [mean, rstd, w, b],
                                True),
        "bwd stats": lambda: st(2, x, dy, None, mask, ws, [mean, rstd], True),
        "bwd stats+g": lambda: st(2, x, dy, out, mask, ws, [mean, rstd],
                                  True),
        "bwd dx": lambda: st(3, x, dy, out, mask, ws, [mean, rstd, w, dg, db],
                             True),
    }


def time_round(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms


# Forward (conv, BN) pairs of the ResNet-50 bottlenecks (the stem is a module
# of its own): (kind, Cin, Cout, input H=W, kernel, stride, pairs per step).
# 'gemm' is a 1x1 stride-1 conv through gemm_bt, 'conv' goes through conv_mfma.
RESNET50_CONV_BN = [
    ("gemm", 64, 64, 56, 1, 1, 1), ("gemm", 256, 64, 56, 1, 1, 2),
    ("conv", 64, 64, 56, 3, 1, 3), ("gemm", 64, 256, 56, 1, 1, 4),
    ("gemm", 256, 128, 56, 1, 1, 1), ("conv", 128, 128, 56, 3, 2, 1),
    ("gemm", 128, 512, 28, 1, 1, 4), ("conv", 256, 512, 56, 1, 2, 1),
    ("gemm", 512, 128, 28, 1, 1, 3), ("conv", 128, 128, 28, 3, 1, 3),
    ("gemm", 512, 256, 28, 1, 1, 1), ("conv", 256, 256, 28, 3, 2, 1),
    ("gemm", 256, 1024, 14, 1, 1, 6), ("conv", 512, 1024, 28, 1, 2, 1),
    ("gemm", 1024, 256, 14, 1, 1, 5), ("conv", 256, 256, 14, 3, 1, 5),
    ("gemm", 1024, 512, 14, 1, 1, 1), ("conv", 512, 512, 14, 3, 2, 1),
    ("gemm", 512, 2048, 7, 1, 1, 3), ("conv", 1024, 2048, 14, 1, 2, 1),
    ("gemm", 2048, 512, 7, 1, 1, 2), ("conv", 512, 512, 7, 3, 1, 2),
]


def epilogue_main(args):
    """--epilogue: per (conv, BN) pair, the plain conv kernel followed by the
    statistics pass over its output and that pass's merge (``old``) against
    the conv kernel with the statistics epilogue followed by the tile merge
    (``new``); neither side runs the BN apply. Both alternate inside every
    round; the columns are the medians over the rounds, each side's spread
    (max - min over the rounds) and the conv kernels alone, which shows what
    the epilogue itself costs. A pair counts as ahead when old - new exceeds
    the larger of the two spreads."""
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    N, dev = args.batch, "cuda"
    print("batch {}: ms per (conv + statistics), median of {} rounds x {} "
          "launches".format(N, args.rounds, args.iters))
    print("{:<5s}{:>5s}{:>5s}{:>4s} k s  n {:>7s} | {:>8s} {:>8s} {:>7s} "
          "{:>7s} | {:>8s} {:>8s} | {:>8s} {}".format(
              "kind", "Cin", "Cout", "H", "MB", "old", "new", "sprd o",
              "sprd n", "conv", "conv+epi", "old-new", "verdict"))
    step_old = step_new = step_auto = 0.0
    for kind, cin, cout, H, k, stride, count in RESNET50_CONV_BN:
        OH = (H - 1) // stride + 1
        x = torch.randn(N, cin, H, H, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, k * k * cin, device=dev)
             / (k * k * cin) ** 0.5).to(torch.bfloat16)
        rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        x2d = x.permute(0, 2, 3, 1).reshape(-1, cin)

        def as4d(t):
            return t.view(N, OH, OH, cout).permute(0, 3, 1, 2)

        if kind == "gemm":
            def plain():
                return as4d(ext.gemm_bt(x2d, w, True))

            def fused():
                t, part, rows = ext.gemm_bt_stats(x2d, w)
                return as4d(t), part, rows
        else:
            def plain():
                return ext.conv_mfma(x, w, cout, k, k, stride, k // 2, 1, -1,
                                     -1)

            def fused():
                return ext.conv_mfma_stats(x, w, cout, k, k, stride, k // 2,
                                           1, -1, -1)

        def old():
            ext.bn_batch_stats(plain(), None, 0, rm, rv, 0.1, 1e-5)

        def new():
            t, part, rows = fused()
            ext.bn_batch_stats(t, part, rows, rm, rv, 0.1, 1e-5)

        has_epi = fused()[1] is not None
        calls = [("old", old), ("new", new), ("conv", plain),
                 ("conv+epi", fused)]
        for _, fn in calls:
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n, _ in calls}
        for _ in range(args.rounds):
            for n, fn in calls:
                ms[n].append(time_round(fn, args.iters))
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = {n: max(v) - min(v) for n, v in ms.items()}
        gain = med["old"] - med["new"]
        if not has_epi:
            verdict = "no epilogue (256^2 GEMM route)"
        elif gain > max(spread["old"], spread["new"]):
            verdict = "ahead"
        else:
            verdict = "not ahead"
        step_old += count * med["old"]
        step_new += count * med["new"]
        step_auto += count * (med["new"] if verdict == "ahead" else med["old"])
        print("{:<5s}{:5d}{:5d}{:4d} {} {} {:2d} {:7.0f} | {:8.4f} {:8.4f} "
              "{:7.4f} {:7.4f} | {:8.4f} {:8.4f} | {:8.4f} {}".format(
                  kind, cin, cout, H, k, stride, count,
                  N * OH * OH * cout * 2 / 1e6, med["old"], med["new"],
                  spread["old"], spread["new"], med["conv"], med["conv+epi"],
                  gain, verdict), flush=True)
        del x, w, x2d
    print("per step (pairs x medians), ms: old {:.3f}  new everywhere {:.3f}  "
          "new where ahead {:.3f}".format(step_old, step_new, step_auto))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ext", action="append", default=[], metavar="NAME=PATH",
                    help="another build of the extension to alternate with")
    ap.add_argument("--epilogue", action="store_true",
                    help="per ResNet-50 (conv, BN) pair: statistics from the "
                         "conv epilogue vs the separate pass")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_bench needs a GPU")
    if args.epilogue:
        return epilogue_main(args)
    from tensorflowonspark_amd.ops import get_ext
    exts = [("tree", get_ext(required=True))]
    for spec in args.ext:
        name, path = spec.split("=", 1)
        exts.append((name, load_ext(path)))
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    esize, vec = (2, 8) if args.dtype == "bf16" else (4, 4)
    N = args.batch
    dev = "cuda"

    print("batch {} {}: ms and TB/s per launch, median of {} rounds x {} "
          "launches".format(N, args.dtype, args.rounds, args.iters))
    print("{:>5s} {:>4s} {:>7s} {:<12s}".format("C", "HW", "MB", "kernel")
          + "".join(" {:>9s} ms {:>5s}TB/s {:>5s}".format(n[:9], "", "nb")
                    for n, _ in exts))
    total_ms = {n: 0.0 for n, _ in exts}
    slow = []
    for C, HW in RESNET50:
        shape = (N, C, HW, HW)

        def act():
            return torch.randn(shape, device=dev).to(dtype).contiguous(
                memory_format=torch.channels_last)

        numel = N * C * HW * HW
        nvec = numel // vec
        t = {"x": act(), "res": act(), "dy": act(),
             "out": torch.empty(shape, device=dev, dtype=dtype).contiguous(
                 memory_format=torch.channels_last),
             "mask": torch.randint(0, 256, (nvec,), device=dev,
                                   dtype=torch.uint8),
             "mean": torch.randn(C, device=dev),
             "rstd": torch.rand(C, device=dev) + 0.5,
             "w": torch.rand(C, device=dev) + 0.5,
             "b": torch.randn(C, device=dev),
             "dg": torch.randn(C, device=dev),
             "db": torch.randn(C, device=dev)}
        nbs = {n: e.bn_fast_blocks(numel, C, args.dtype == "bf16", True)
               for n, e in exts}
        t["ws"] = torch.empty(max(nbs.values()) * 2 * C, device=dev)
        calls = {n: make_calls(e, t) for n, e in exts}
        # yardstick on the same tensors: a plain device copy, 1 read + 1 write
        copy = [time_round(lambda: t["out"].copy_(t["x"]), args.iters)
                for _ in range(args.rounds + 1)][1:]
        med = statistics.median(copy)
        print("{:5d} {:4d} {:7.0f} {:<12s} {:12.4f} {:9.2f}".format(
            C, HW, numel * esize / 1e6, "(copy)", med,
            2 * numel * esize / med / 1e9), flush=True)
        for k in KERNELS:
            for n, _ in exts:          # warm up: code objects, caches
                calls[n][k]()
            torch.cuda.synchronize()
            ms = {n: [] for n, _ in exts}
            for _ in range(args.rounds):
                for n, _ in exts:      # alternate the builds inside a round
                    ms[n].append(time_round(calls[n][k], args.iters))
            line = "{:5d} {:4d} {:7.0f} {:<12s}".format(
                C, HW, numel * esize / 1e6, k)
            for n, _ in exts:
                med = statistics.median(ms[n])
                tbs = bytes_moved(k, numel, esize, nvec, nbs[n], C) / med / 1e9
                total_ms[n] += med
                line += " {:12.4f} {:9.2f} {:5d}".format(med, tbs, nbs[n])
                if n == "tree" and tbs < COPY_TBS * 2 / 3:
                    slow.append((C, HW, k, tbs))
            print(line, flush=True)
        del t, calls
    print("sum of medians, ms: " + ", ".join(
        "{} {:.3f}".format(n, v) for n, v in total_ms.items()))
    print("in-tree (shape, kernel) pairs under 2/3 of {} TB/s:".format(COPY_TBS))
    for C, HW, k, tbs in slow:
        print("  C={} HW={} {}: {:.2f} TB/s".format(C, HW, k, tbs))


if __name__ == "__main__":
    main()
