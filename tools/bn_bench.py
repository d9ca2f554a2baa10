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

``--rows`` is a third table: per BatchNorm of the U-Net (MobileNetV2 encoder)
whose width takes the NHWC row tier, each kernel family with ``TFOS_BN_ROWS``
on against off (the generic kernels), see ``rows_main``.

``--stempool`` is a fourth: the stem's BatchNorm + ReLU + max-pool as three ops
against the fused kernels of csrc/bn_pool.hip, see ``stempool_main``.

``--gate`` is a fifth: the backward tail of an identity bottleneck, ``bn_bwd``
writing the gated gradient + ``gemm_bt_acc`` against ``bn_bwd`` without it +
``gemm_bt_gate``, see ``gate_main``; it is what the ``TFOS_BN_GATE=auto`` rule
was read off.

The variants timed are the ones the ResNet-50 step runs most: stats; apply
with ReLU (and with ReLU + residual, ``apply+res``); bwd stats with the mask
(and writing the gated gradient, ``bwd stats+g``); bwd dx with the mask.
"""

import argparse
import collections
import importlib.util
import json
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


def unet_bn_shapes(ext, batch, bf16):
    """(C, H, W, relu, add) -> count over the U-Net's fused BatchNorms that
    take the row tier at this batch, from a CPU forward of the model."""
    from tensorflowonspark_amd.models import unet_mobilenet
    from tensorflowonspark_amd.ops.modules import FusedBNReLU
    model = unet_mobilenet().eval()
    seen = collections.Counter()

    def hook(m, args, out):
        _, C, H, W = out.shape
        if ext.bn_rows_plan(batch * C * H * W, C, bf16, True)[0] > 0:
            seen[(C, H, W, m.RELU, m.ADD)] += 1

    for m in model.modules():
        if isinstance(m, FusedBNReLU):
            m.register_forward_hook(hook)
    with torch.no_grad():
        model(torch.zeros(1, 3, 128, 128))
    return sorted(seen.items())


def rows_main(args):
    """--rows: per row-tier BatchNorm of the U-Net at 128x128, the four kernel
    families as that layer runs them (ReLU gated on y; the project BN of a
    skip block adds the residual and writes the gated gradient), with
    TFOS_BN_ROWS=on and =off alternating inside every round on the same
    tensors. Columns: medians over the rounds in ms and GB/s of the bytes the
    launch must move, the spread (max - min) of off, off/on, and the plain
    device copy of the same tensor as the yardstick. ``on`` counts as slower
    only where on - off exceeds off's own spread."""
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    bf16 = args.dtype == "bf16"
    dtype = torch.bfloat16 if bf16 else torch.float32
    esize = 2 if bf16 else 4
    N, dev = args.batch, "cuda"
    os.environ["TFOS_BN_ROWS"] = "on"
    shapes = unet_bn_shapes(ext, N, bf16)
    for key, n in shapes:
        print("# C={} H={} W={} relu={} add={} x{}".format(*key, n))
    print("batch {} {}: U-Net row-tier BatchNorms, median of {} rounds x {} "
          "launches".format(N, args.dtype, args.rounds, args.iters))
    print("{:>4s} {:>3s} {:>2s} {:<8s} {:<10s} {:>6s} {:>9s} | {:>8s} {:>7s} "
          "{:>7s} | {:>8s} {:>7s} | {:>6s}".format(
              "C", "H", "n", "layer", "kernel", "MB", "copy GB/s", "off ms",
              "GB/s", "spread", "on ms", "GB/s", "off/on"))
    records, slower = [], []
    step = {"on": 0.0, "off": 0.0}
    for (C, H, W, relu, add), count in shapes:
        shape = (N, C, H, W)

        def act():
            return torch.randn(shape, device=dev).to(dtype).contiguous(
                memory_format=torch.channels_last)

        x, other, y, out = act(), act(), act(), act()
        vecs = [torch.rand(C, device=dev) + 0.5 for _ in range(5)]
        nb = ext.bn_rows_plan(x.numel(), C, bf16, True)[0]
        ws = torch.zeros(nb * 2 * C, device=dev)
        t = x.numel() * esize
        st = ext.bn_stage
        g = out if add else None
        calls = [
            ("stats", t, lambda: st(0, x, None, None, None, ws, [], False)),
            ("apply", (3 if add else 2) * t,
             lambda: st(1, x, other if add else None, out, None, ws, vecs[:4],
                        relu)),
            ("bwd stats", (2 + relu + add) * t,
             lambda: st(2, x, other, g, None, ws, vecs[:2], relu, y)),
            ("bwd dx", (3 + relu) * t,
             lambda: st(3, x, other, out, None, ws, vecs, relu, y)),
        ]
        copy = statistics.median(
            [time_round(lambda: out.copy_(x), args.iters)
             for _ in range(args.rounds + 1)][1:])
        layer = ("relu" if relu else "lin") + ("+res" if add else "")
        for kernel, nbytes, fn in calls:
            ms = {"off": [], "on": []}
            for mode in ms:                      # warm up both tiers
                os.environ["TFOS_BN_ROWS"] = mode
                fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for mode in ms:                  # alternate inside a round
                    os.environ["TFOS_BN_ROWS"] = mode
                    ms[mode].append(time_round(fn, args.iters))
            med = {m: statistics.median(v) for m, v in ms.items()}
            spread = max(ms["off"]) - min(ms["off"])
            for m in med:
                step[m] += count * med[m]
            if med["on"] - med["off"] > spread:
                slower.append((C, H, layer, kernel))
            records.append({"batch": N, "C": C, "H": H, "W": W,
                            "layer": layer, "count": count, "kernel": kernel,
                            "bytes": nbytes, "copy_ms": copy,
                            "off_ms": ms["off"], "on_ms": ms["on"]})
            print("{:4d} {:3d} {:2d} {:<8s} {:<10s} {:6.0f} {:9.0f} | {:8.4f} "
                  "{:7.0f} {:7.4f} | {:8.4f} {:7.0f} | {:6.2f}".format(
                      C, H, count, layer, kernel, t / 1e6, 2 * t / copy / 1e6,
                      med["off"], nbytes / med["off"] / 1e6, spread,
                      med["on"], nbytes / med["on"] / 1e6,
                      med["off"] / med["on"]), flush=True)
        del x, other, y, out, calls
    os.environ["TFOS_BN_ROWS"] = "on"
    print("per step (count x medians), ms: off {:.3f}  on {:.3f}".format(
        step["off"], step["on"]))
    print("on slower than off beyond off's spread: {}".format(slower or "none"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


# --stempool shapes: the ResNet-50 stem at b1024 and DeepLabV3's at b32
STEM_SHAPES = [(1024, 64, 112, 112), (32, 64, 256, 256)]


def stempool_main(args):
    """--stempool: the stem tail BatchNorm + ReLU + max-pool (3/2/1) as three
    ops against the fused entries of csrc/bn_pool.hip, on the two stem shapes,
    alternating in one process: every row of a shape is timed once per round,
    one after the other. Rows: a plain device copy of the conv output (the
    yardstick), each kernel alone (old: apply, maxpool fwd, maxpool bwd, bwd
    stats, bwd dx; new: fwd, bwd stats, bwd dx) with the bytes it must move
    over its time, and the chains as the autograd functions run them (fwd and
    fwd + bwd). Then the two acceptance comparisons, each with its margin
    against the larger of the two spreads (max - min over the rounds)."""
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    dev, bf = "cuda", torch.bfloat16
    K, S, P = 3, 2, 1
    records = []
    print("stem tail, bf16: ms per launch, median / spread of {} rounds x {} "
          "launches".format(args.rounds, args.iters))
    for N, C, H, W in STEM_SHAPES:
        OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
        shape = (N, C, H, W)

        def act(s):
            return torch.randn(s, device=dev).to(bf).contiguous(
                memory_format=torch.channels_last)

        x, out = act(shape), act(shape)
        dp = act((N, C, OH, OW))
        w = torch.rand(C, device=dev) + 0.5
        b = torch.randn(C, device=dev) * 0.1
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        # one real forward of each path: y, mask, idx as training has them
        y, mean, rstd, mask = ext.bn_fwd_train(x, None, w, b, rm, rv, 0.1,
                                               1e-5, True)
        p_old, idx_old = ext.maxpool_fwd(y, K, S, P)
        p_new, idx_new, _, _ = ext.bn_relu_pool_fwd(x, w, b, rm, rv, 0.1,
                                                    1e-5, K, S, P)
        dy = ext.maxpool_bwd(dp, idx_old, H, W, K, S, P)
        _, dg, db = ext.bn_bwd(x, dy, y, mask, w, mean, rstd, True, False)
        nb_old = ext.bn_fast_blocks(x.numel(), C, True, True)
        nb_new = ext.bn_relu_pool_blocks(dp.numel())
        ws = torch.empty(max(nb_old, nb_new) * 2 * C, device=dev)
        t, tp = x.numel() * 2, dp.numel() * 2       # bytes: x-sized, pooled
        ti, tm = dp.numel(), x.numel() // 8          # index bytes, mask bytes
        st, ps = ext.bn_stage, ext.bn_relu_pool_stage
        v4, v2 = [mean, rstd, w, b], [mean, rstd]
        v5 = [mean, rstd, w, dg, db]

        def old_fwd():
            yy = ext.bn_fwd_train(x, None, w, b, rm, rv, 0.1, 1e-5, True)
            return yy, ext.maxpool_fwd(yy[0], K, S, P)

        def new_fwd():
            return ext.bn_relu_pool_fwd(x, w, b, rm, rv, 0.1, 1e-5, K, S, P)

        def old_both():
            yy, (_, ii) = old_fwd()
            d = ext.maxpool_bwd(dp, ii, H, W, K, S, P)
            ext.bn_bwd(x, d, yy[0], yy[3], w, yy[1], yy[2], True, False)

        def new_both():
            _, ii, m, r = new_fwd()
            ext.bn_relu_pool_bwd(x, dp, ii, w, m, r, K, S, P)

        rows = [
            ("(copy)", 2 * t, lambda: out.copy_(x)),
            ("stats (both)", t, lambda: st(0, x, None, None, None, ws, [],
                                           False, None)),
            ("old apply", 2 * t + tm,
             lambda: st(1, x, None, out, mask, ws, v4, True, None)),
            ("old maxpool fwd", t + tp + ti,
             lambda: ext.maxpool_fwd(y, K, S, P)),
            ("new fwd", t + tp + ti,
             lambda: ps(0, x, p_new, idx_new, None, None, v4, K, S, P)),
            ("old maxpool bwd", tp + ti + t,
             lambda: ext.maxpool_bwd(dp, idx_old, H, W, K, S, P)),
            ("old bwd stats", 2 * t + tm,
             lambda: st(2, x, dy, None, mask, ws, v2, True, None)),
            ("old bwd dx", 3 * t + tm,
             lambda: st(3, x, dy, out, mask, ws, v5, True, None)),
            ("new bwd stats", t + tp + ti,
             lambda: ps(1, x, dp, idx_new, None, ws, v2, K, S, P)),
            ("new bwd dx", 2 * t + tp + ti,
             lambda: ps(2, x, dp, idx_new, out, None, v5, K, S, P)),
            ("old chain fwd", None, old_fwd),
            ("new chain fwd", None, new_fwd),
            ("old chain fwd+bwd", None, old_both),
            ("new chain fwd+bwd", None, new_both),
        ]
        for _, _, fn in rows:
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n, _, _ in rows}
        for _ in range(args.rounds):
            for n, _, fn in rows:
                ms[n].append(time_round(fn, args.iters))
        med = {n: statistics.median(v) for n, v in ms.items()}
        spr = {n: max(v) - min(v) for n, v in ms.items()}
        print("{}x{}x{}x{} ({:.0f} MB)".format(N, C, H, W, t / 1e6))
        print("  {:<18s} {:>8s} {:>8s} {:>8s} {:>7s}".format(
            "row", "ms", "spread", "GB", "TB/s"))
        for n, nbytes, _ in rows:
            if nbytes is None:
                print("  {:<18s} {:8.4f} {:8.4f}".format(n, med[n], spr[n]))
            else:
                print("  {:<18s} {:8.4f} {:8.4f} {:8.3f} {:7.2f}".format(
                    n, med[n], spr[n], nbytes / 1e9, nbytes / med[n] / 1e9))
            records.append({"shape": shape, "row": n, "bytes": nbytes,
                            "ms": ms[n]})

        def verdict(what, old_names, new_names):
            o = sum(med[n] for n in old_names)
            nw = sum(med[n] for n in new_names)
            sp = max(sum(spr[n] for n in old_names),
                     sum(spr[n] for n in new_names))
            ok = o - nw > sp
            print("  {}: old {:.4f} new {:.4f} margin {:+.4f} spread {:.4f} "
                  "-> {}".format(what, o, nw, o - nw, sp,
                                 "ahead" if ok else "NOT ahead"), flush=True)

        verdict("fwd kernel vs maxpool fwd alone", ["old maxpool fwd"],
                ["new fwd"])
        verdict("bwd pair vs maxpool bwd + bwd dx",
                ["old maxpool bwd", "old bwd dx"],
                ["new bwd stats", "new bwd dx"])
        verdict("chain fwd", ["old chain fwd"], ["new chain fwd"])
        verdict("chain fwd+bwd", ["old chain fwd+bwd"], ["new chain fwd+bwd"])
        del x, out, dp, y, dy, mask, p_old, p_new, idx_old, idx_new, rows
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


# --gate shapes: the join (batch, C3, H=W, C1, identity blocks per step) of
# the ResNet-50 identity bottlenecks at b1024 and one size below them
GATE_SHAPES = [(32, 256, 56, 64, 0), (1024, 256, 56, 64, 2),
               (1024, 512, 28, 128, 3), (1024, 1024, 14, 256, 5),
               (1024, 2048, 7, 512, 2)]


def gate_main(args):
    """--gate: the tail of an identity bottleneck's backward as two chains on
    the same tensors, alternating inside every round: ``old`` is bn_bwd
    writing the gated gradient out (relu, grad_res) + gemm_bt_acc into it,
    ``new`` is bn_bwd without that write + gemm_bt_gate, which gates dy by
    the mask in its own epilogue. Columns: medians over the rounds, each
    side's spread (max - min over the rounds), old - new; a size is ahead
    when old - new exceeds the larger spread. The ``TFOS_BN_GATE=auto`` rule
    in ops/modules.py routes from the smallest size that is ahead."""
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    dev, bf = "cuda", torch.bfloat16
    print("identity-block join, bf16: ms per chain, median of {} rounds x {} "
          "launches".format(args.rounds, args.iters))
    print("{:>5s} {:>5s} {:>3s} {:>4s} {:>2s} {:>6s} | {:>8s} {:>8s} {:>7s} "
          "{:>7s} | {:>8s} {}".format("batch", "C3", "H", "C1", "n", "MB",
                                      "old", "new", "sprd o", "sprd n",
                                      "old-new", "verdict"))
    records = []
    step_old = step_new = 0.0
    for N, C3, H, C1, count in GATE_SHAPES:
        shape = (N, C3, H, H)

        def act(s=shape):
            return torch.randn(s, device=dev).to(bf).contiguous(
                memory_format=torch.channels_last)

        t3, res, dy = act(), act(), act()
        dt1 = act((N, C1, H, H)).permute(0, 2, 3, 1).reshape(-1, C1)
        w1bT = (torch.randn(C3, C1, device=dev) / C1 ** 0.5).to(bf)
        w, b = torch.rand(C3, device=dev) + 0.5, torch.randn(C3, device=dev)
        rm, rv = torch.zeros(C3, device=dev), torch.ones(C3, device=dev)
        # one real forward: y, the mask and the statistics as training has them
        y, mean, rstd, mask = ext.bn_fwd_train(t3, res, w, b, rm, rv, 0.1,
                                               1e-5, True)
        del res
        dy2d = dy.permute(0, 2, 3, 1).reshape(-1, C3)
        assert ext.gemm_bt_gate_eligible(dt1.shape[0], C3, C1)

        def old():
            _, _, _, dres = ext.bn_bwd(t3, dy, y, mask, w, mean, rstd, True,
                                       True)
            return ext.gemm_bt_acc(dt1, w1bT,
                                   dres.permute(0, 2, 3, 1).reshape(-1, C3))

        def new():
            ext.bn_bwd(t3, dy, y, mask, w, mean, rstd, True, False)
            return ext.gemm_bt_gate(dt1, w1bT, dy2d, mask)

        assert torch.equal(old(), new()), "the two chains differ"
        torch.cuda.synchronize()
        ms = {"old": [], "new": []}
        for _ in range(args.rounds):
            for n, fn in (("old", old), ("new", new)):
                ms[n].append(time_round(fn, args.iters))
        med = {n: statistics.median(v) for n, v in ms.items()}
        spr = {n: max(v) - min(v) for n, v in ms.items()}
        gain = med["old"] - med["new"]
        ahead = gain > max(spr.values())
        step_old += count * med["old"]
        step_new += count * med["new"]
        records.append({"shape": shape, "C1": C1, "count": count,
                        "old_ms": ms["old"], "new_ms": ms["new"]})
        print("{:5d} {:5d} {:3d} {:4d} {:2d} {:6.0f} | {:8.4f} {:8.4f} {:7.4f} "
              "{:7.4f} | {:8.4f} {}".format(
                  N, C3, H, C1, count, t3.numel() * 2 / 1e6, med["old"],
                  med["new"], spr["old"], spr["new"], gain,
                  "ahead" if ahead else "NOT ahead"), flush=True)
        del t3, dy, dy2d, y, mask, dt1
        torch.cuda.empty_cache()
    print("per step (blocks x medians), ms: old {:.3f}  new {:.3f}".format(
        step_old, step_new))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


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
    ap.add_argument("--rows", action="store_true",
                    help="per U-Net row-tier BatchNorm: TFOS_BN_ROWS on vs off")
    ap.add_argument("--stempool", action="store_true",
                    help="the stem's BatchNorm + ReLU + max-pool: three ops vs "
                         "the fused entries")
    ap.add_argument("--gate", action="store_true",
                    help="identity-block join: bn_bwd + gemm_bt_acc vs the "
                         "mask-gating dgrad epilogue (gemm_bt_gate)")
    ap.add_argument("--json", metavar="PATH",
                    help="with --rows, --stempool or --gate: also write every "
                         "round's times here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_bench needs a GPU")
    if args.gate:
        return gate_main(args)
    if args.stempool:
        return stempool_main(args)
    if args.rows:
        return rows_main(args)
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
