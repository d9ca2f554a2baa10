#!/usr/bin/env python3
"""Per-shape conv microbenchmark: in-tree MFMA kernels vs library (MIOpen).

Covers the ResNet-50 stride-2 shapes and the U-Net decoder transposed convs
(VERDICT r01 item 1/7). Run on a GPU box:
    python tools/conv_bench.py [--batch 1024]
    python tools/conv_bench.py --atrous [--batch 32] [--rounds 9]
    python tools/conv_bench.py --wrwtail --parent-ext OLD/tfosr_hip_ops_parent.so
    python tools/conv_bench.py --halo [--parent-ext OLD/tfosr_hip_ops_parent.so]
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1000


def bench_module(mod_fwd, mod_lib, x, tag):
    """Compare fwd and fwd+bwd times of the MFMA module vs library module."""
    xg = x.requires_grad_(True)

    def fwd(m):
        return lambda: m(xg)

    def fwdbwd(m):
        def run():
            if xg.grad is not None:
                xg.grad = None
            y = m(xg)
            y.backward(torch.ones_like(y))
        return run

    f_m = timeit(fwd(mod_fwd))
    f_l = timeit(fwd(mod_lib))
    b_m = timeit(fwdbwd(mod_fwd))
    b_l = timeit(fwdbwd(mod_lib))
    print(f"{tag:45s} fwd {f_m:7.3f} vs lib {f_l:7.3f} ms | "
          f"fwd+bwd {b_m:7.3f} vs lib {b_l:7.3f} ms")
    return f_m, f_l, b_m, b_l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--wrw", action="store_true")
    ap.add_argument("--atrous", action="store_true",
                    help="DeepLabV3 dilated 3x3 shapes, in-tree vs library")
    ap.add_argument("--wrwtail", action="store_true",
                    help="split-M reduce and stem wrw: this tree's extension "
                         "against another build of it (--parent-ext)")
    ap.add_argument("--halo", action="store_true",
                    help="3x3 stride-1 shapes: TFOS_CONV3X3_TILE=im2col "
                         "against halo (both tile heights), alternating")
    ap.add_argument("--halo-shapes", default=None,
                    help="comma-separated tags to restrict --halo to")
    ap.add_argument("--parent-ext", default=None,
                    help="extension of the commit to compare against, built under "
                         "a module name of its own (see load_ext_from)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None,
                    help="also write the --atrous rows to this file")
    args = ap.parse_args()
    if args.wrw:
        bench_wrw(args.batch)
        return
    if args.wrwtail:
        bench_wrwtail(args.batch, args.parent_ext, max(args.rounds, 7),
                      args.iters, args.json)
        return
    if args.halo:
        bench_halo(args.batch, args.parent_ext, args.rounds, args.iters,
                   args.json, args.halo_shapes)
        return
    if args.atrous:
        bench_atrous(32 if args.batch == 1024 else args.batch, args.rounds,
                     args.iters, args.json)
        return
    from tensorflowonspark_amd.ops.modules import (Conv1x1, Conv3x3,
                                                   ConvTranspose2dMFMA)
    N = args.batch
    dev = "cuda"
    torch.manual_seed(0)

    # ResNet-50 stride-2 3x3 convs (v1.5: stride on the middle 3x3)
    shapes_3x3s2 = [(128, 56, 128), (256, 28, 256), (512, 14, 512)]
    for cin, hw, cout in shapes_3x3s2:
        x = torch.randn(N, cin, hw, hw, device=dev, dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        m = Conv3x3(cin, cout, stride=2).to(dev)
        lib = torch.nn.Conv2d(cin, cout, 3, 2, 1, bias=False) \
            .to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last)
        bench_module(m, lib, x, f"conv3x3 s2 {cin}->{cout} @{hw}")

    # ResNet-50 downsample 1x1 s2 convs
    shapes_1x1s2 = [(256, 56, 512), (512, 28, 1024), (1024, 14, 2048)]
    for cin, hw, cout in shapes_1x1s2:
        x = torch.randn(N, cin, hw, hw, device=dev, dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        m = Conv1x1(cin, cout, stride=2).to(dev)
        lib = torch.nn.Conv2d(cin, cout, 1, 2, bias=False) \
            .to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last)
        bench_module(m, lib, x, f"conv1x1 s2 {cin}->{cout} @{hw}")

    # U-Net decoder transposed convs (batch scaled down: seg batch is 64)
    Ns = max(1, N // 16)
    for cin, hw, cout in [(320, 4, 512), (608, 8, 256), (288, 16, 128)]:
        x = torch.randn(Ns, cin, hw, hw, device=dev, dtype=torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        m = ConvTranspose2dMFMA(cin, cout, 4, 2, 1).to(dev)
        lib = torch.nn.ConvTranspose2d(cin, cout, 4, 2, 1, bias=False) \
            .to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last)
        bench_module(m, lib, x, f"convT k4s2 {cin}->{cout} @{hw} (b{Ns})")


def bench_wrw(batch=1024):
    """wrw per ResNet-50 shape: wrw2 kernel vs MIOpen igemm."""
    import torch
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    N = batch
    shapes = [
        # (Cin, HW_in, Cout, k, stride, pad) — ResNet-50 conv zoo
        (64, 56, 64, 3, 1, 1), (128, 28, 128, 3, 1, 1),
        (256, 14, 256, 3, 1, 1), (512, 7, 512, 3, 1, 1),
        (128, 56, 128, 3, 2, 1), (256, 28, 256, 3, 2, 1),
        (512, 14, 512, 3, 2, 1),
        (64, 56, 256, 1, 1, 0), (256, 56, 64, 1, 1, 0),
        (512, 28, 128, 1, 1, 0), (1024, 14, 256, 1, 1, 0),
        (2048, 7, 512, 1, 1, 0), (256, 56, 512, 1, 2, 0),
        (1024, 14, 2048, 1, 2, 0),
    ]
    for cin, hw, cout, k, s, p in shapes:
        oh = (hw + 2 * p - k) // s + 1
        x = torch.randn(N, cin, hw, hw, device="cuda").to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        dy = torch.randn(N, cout, oh, oh, device="cuda").to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w4 = torch.randn(cout, cin, k, k, device="cuda").to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        t2 = timeit(lambda: ext.conv_wrw2(dy, x, k, k, s, p))
        tm = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w4, None, [s, s], [p, p], [1, 1], False, [0, 0], 1,
            [False, True, False]))
        flops = 2.0 * N * oh * oh * cout * k * k * cin
        print(f"wrw {k}x{k} s{s} {cin:5d}->{cout:5d} @{hw:3d}: "
              f"wrw2 {t2:7.3f} ms ({flops/t2/1e9:6.1f} TF) vs "
              f"MIOpen {tm:7.3f} ms ({flops/tm/1e9:6.1f} TF)")


# DeepLabV3 @512^2 (output stride 16 -> 32x32 feature map):
# (Cin, Cout, HW, dilation): stage-4 conv2, then the three ASPP branches
ATROUS_SHAPES = [(512, 512, 32, 2), (2048, 256, 32, 12), (2048, 256, 32, 24),
                 (2048, 256, 32, 36)]


def ab_median(sides, rounds, iters, spread=None):
    """Median ms per call of each side. The sides alternate inside every
    round (one process, one device), each timed with device events around
    ``iters`` back-to-back calls, after a warm-up of every side. ``spread``
    (a dict) receives max - min over the rounds of each side."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    if spread is not None:
        spread.update({k: max(v) - min(v) for k, v in times.items()})
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def bench_atrous(batch=32, rounds=9, iters=5, json_path=None):
    """Forward, dgrad and wrw of the DeepLabV3 atrous 3x3 convs, each timed
    separately: the in-tree MFMA kernels (with and without the per-step
    weight re-layout the module does from its fp32 parameter) against the
    library conv. The rate-36 shape also times the dead-tap collapse (a 1x1
    GEMM on the centre tap) against the library's 9-tap run."""
    import json
    import torch.nn.functional as F
    from tensorflowonspark_amd.ops import get_ext
    from tensorflowonspark_amd.ops.modules import live_taps
    ext = get_ext(required=True)
    conv_bwd = torch.ops.aten.convolution_backward
    bf16 = torch.bfloat16
    rows = []
    torch.manual_seed(0)
    for cin, cout, hw, fd in ATROUS_SHAPES:
        N = batch
        x = (torch.randn(N, cin, hw, hw, device="cuda") / 4).to(bf16) \
            .contiguous(memory_format=torch.channels_last)
        dy = (torch.randn(N, cout, hw, hw, device="cuda") / 4).to(bf16) \
            .contiguous(memory_format=torch.channels_last)
        w32 = torch.randn(cout, cin, 3, 3, device="cuda") / 16   # fp32 master
        w4 = w32.to(bf16).contiguous(memory_format=torch.channels_last)

        def w9_of():
            return w32.permute(0, 2, 3, 1).reshape(cout, 9 * cin).to(bf16) \
                .contiguous()

        def wperm_of():
            return w32.flip(2, 3).permute(1, 2, 3, 0).to(bf16).contiguous() \
                .reshape(cin, 9 * cout)
        w9, wperm = w9_of(), wperm_of()
        flops = 2.0 * N * hw * hw * cout * 9 * cin

        def lib_bwd(mask):
            return lambda: conv_bwd(dy, x, w4, None, [1, 1], [fd, fd],
                                    [fd, fd], False, [0, 0], 1, mask)
        plan = {
            "fwd": {
                "mfma": lambda: ext.conv_mfma(x, w9, cout, 3, 3, 1, fd, 1,
                                              -1, -1, fd=fd),
                "mfma+prep": lambda: ext.conv_mfma(x, w9_of(), cout, 3, 3, 1,
                                                   fd, 1, -1, -1, fd=fd),
                "lib": lambda: F.conv2d(x, w4, None, 1, fd, fd),
                "lib+cast": lambda: F.conv2d(x, w32.to(bf16), None, 1, fd,
                                             fd),
            },
            "dgrad": {
                "mfma": lambda: ext.conv_mfma(dy, wperm, cin, 3, 3, 1, fd, 1,
                                              hw, hw, fd=fd),
                "mfma+prep": lambda: ext.conv_mfma(dy, wperm_of(), cin, 3, 3,
                                                   1, fd, 1, hw, hw, fd=fd),
                "lib": lib_bwd([True, False, False]),
            },
            "wrw": {
                "mfma": lambda: ext.conv_wrw2(dy, x, 3, 3, 1, fd, fd=fd),
                "lib": lib_bwd([False, True, False]),
            },
        }
        if live_taps(hw, hw, 3, 1, fd, fd) == ((1,), (1,)):
            x2d = x.permute(0, 2, 3, 1).reshape(-1, cin)
            dy2d = dy.permute(0, 2, 3, 1).reshape(-1, cout)
            wc = w4[:, :, 1, 1].contiguous()
            wct = wc.t().contiguous()
            wc4 = wc.view(cout, cin, 1, 1)
            plan["fwd"]["collapse"] = lambda: ext.gemm_bt(x2d, wc, True)
            plan["fwd"]["collapse+prep"] = lambda: ext.gemm_bt(
                x2d, w32[:, :, 1, 1].to(bf16).contiguous(), True)
            plan["dgrad"]["collapse"] = lambda: ext.gemm_bt(dy2d, wct, True)
            plan["dgrad"]["collapse+prep"] = lambda: ext.gemm_bt(
                dy2d, w32[:, :, 1, 1].to(bf16).t().contiguous(), True)
            plan["wrw"]["collapse-wrw2"] = lambda: ext.conv_wrw2(
                dy, x, 1, 1, 1, 0)
            plan["wrw"]["collapse-lib1x1"] = lambda: conv_bwd(
                dy, x, wc4, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                [False, True, False])
        for direction, sides in plan.items():
            med = ab_median(sides, rounds, iters)
            tag = "{:5s} {}->{} @{} d{} b{}".format(direction, cin, cout, hw,
                                                     fd, N)
            cells = "  ".join("{} {:.3f} ms ({:.0f} TF/s)".format(
                k, v, flops / v / 1e9) for k, v in med.items())
            print(tag + ": " + cells, flush=True)
            rows.append(dict(direction=direction, cin=cin, cout=cout, hw=hw,
                             fd=fd, batch=N, flops=flops, ms=med))
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)),
                    exist_ok=True)
        with open(json_path, "w") as f:
            json.dump(rows, f, indent=1)


def load_ext_from(path):
    """Another build of the extension, next to the tree's own, in this
    process. pybind11 hands out one module per module NAME, so the other
    build's bindings.cpp is compiled with -DTORCH_EXTENSION_NAME=<stem of its
    file name> (say tfosr_hip_ops_parent.so); its extern "C" launchers stay
    its own, extension modules being loaded RTLD_LOCAL."""
    import importlib.util
    from tensorflowonspark_amd.ops import get_ext
    name = os.path.basename(path).split(".")[0]
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod is get_ext(required=True):
        raise RuntimeError(
            "{} loaded as the tree's own extension: build it under another "
            "module name (-DTORCH_EXTENSION_NAME)".format(path))
    return mod


def bench_wrwtail(batch=1024, parent_ext=None, rounds=7, iters=5,
                  json_path=None):
    """The two in-tree weight gradients of the ResNet-50 step end to end
    (kernel + split-M reduce): conv_wrw2 64->64 3x3 @56 and conv_stem_wrw,
    this tree's extension against --parent-ext, alternating. Next to them a
    plain device copy of each split workspace's bytes (split x n fp32): what
    a reduce at copy bandwidth would cost. The reduce kernels on their own
    are read from a kernel trace of this same run."""
    import json
    from tensorflowonspark_amd.ops import get_ext
    new = get_ext(required=True)
    exts = {"new": new}
    if parent_ext:
        exts = {"parent": load_ext_from(parent_ext), "new": new}
    bf16 = torch.bfloat16
    torch.manual_seed(0)
    N = batch

    def cl(t):
        return t.contiguous(memory_format=torch.channels_last)
    x = cl((torch.randn(N, 64, 56, 56, device="cuda") / 4).to(bf16))
    dy = cl((torch.randn(N, 64, 56, 56, device="cuda") / 4).to(bf16))
    x4 = cl((torch.randn(N, 4, 230, 230, device="cuda") / 4).to(bf16))
    dys = cl((torch.randn(N, 64, 112, 112, device="cuda") / 4).to(bf16))
    rows = []
    plan = [
        ("conv_wrw2 64->64 3x3 @56", 64 * 9 * 64, N * 56 * 56,
         lambda e: (lambda: e.conv_wrw2(dy, x, 3, 3, 1, 1))),
        ("conv_stem_wrw @224", 64 * 224, N * 112 * 112,
         lambda e: (lambda: e.conv_stem_wrw(dys, x4))),
    ]
    for tag, n, M, call in plan:
        split = 1024                      # tfosr_wrw2_split of one 64x64 tile
        while split * 8 > (M + 31) // 32 and split > 1:
            split //= 2
        src = torch.empty(split * n, device="cuda")
        dst = torch.empty_like(src)
        sides = {k: call(e) for k, e in exts.items()}
        sides["copy"] = lambda: dst.copy_(src)
        same = {k: fn().clone() for k, fn in sides.items() if k != "copy"}
        if "parent" in same:
            d = (same["new"].double() - same["parent"].double()).abs()
            print("{}: new vs parent max |d| {:.3e} on max |dW| {:.3e}".format(
                tag, d.max().item(), same["parent"].abs().max().item()))
        spread = {}
        med = ab_median(sides, rounds, iters, spread)
        mb = split * n * 4 / 1e6
        cells = "  ".join("{} {:.4f} ms (spread {:.4f})".format(
            k, v, spread[k]) for k, v in med.items())
        print("{} b{}: split {} x n {} = {:.0f} MB fp32 | {} | copy moves "
              "{:.0f} GB/s read+write".format(
                  tag, N, split, n, mb, cells, 2 * mb / med["copy"]),
              flush=True)
        rows.append(dict(tag=tag, batch=N, split=split, n=n, ws_mb=mb,
                         ms=med, spread=spread))
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)),
                    exist_ok=True)
        with open(json_path, "w") as f:
            json.dump(rows, f, indent=1)


def bench_halo(batch=1024, parent_ext=None, rounds=9, iters=5,
               json_path=None, only=None):
    """conv_mfma on the plain 3x3 stride-1 launch, forward (w9 pack) and
    dgrad (flipped pack; the same launch on dy): the im2col kernel against
    the halo kernel at both tile heights, switched per call through
    TFOS_CONV3X3_TILE / TFOS_CONV3X3_HALO_BM (read at call time), alternating
    in one process; --parent-ext adds the parent's build. `auto` is timed as
    well, so the table shows what the default routing launches."""
    import json
    from tensorflowonspark_amd.ops import get_ext
    ext = get_ext(required=True)
    parent = load_ext_from(parent_ext) if parent_ext else None
    bf16 = torch.bfloat16
    torch.manual_seed(0)
    # tag, N, C, H=W
    shapes = [
        ("64@56", batch, 64, 56), ("128@28", batch, 128, 28),
        ("256@14", batch, 256, 14), ("512@7", batch, 512, 7),
        # segmentation-sized launches (no model in the tree routes them here
        # yet): a U-Net decoder level and a DeepLab head, at their batches
        ("unet 64@128 b64", max(1, batch // 16), 64, 128),
        ("deeplab 256@33 b32", max(1, batch // 32), 256, 33),
        # small M, to place the `auto` threshold
        ("64@56 b64", max(1, batch // 16), 64, 56),
        ("64@56 b8", max(1, batch // 128), 64, 56),
        ("128@28 b32", max(1, batch // 32), 128, 28),
    ]
    if only:
        keep = set(only.split(","))
        shapes = [s for s in shapes if s[0] in keep]

    def side(e, mode, bm, x, w, C):
        def run():
            os.environ["TFOS_CONV3X3_TILE"] = mode
            if bm:
                os.environ["TFOS_CONV3X3_HALO_BM"] = str(bm)
            else:
                os.environ.pop("TFOS_CONV3X3_HALO_BM", None)
            return e.conv_mfma(x, w, C, 3, 3, 1, 1, 1, -1, -1)
        return run

    rows = []
    for tag, N, C, hw in shapes:
        x = (torch.randn(N, C, hw, hw, device="cuda") / 4).to(bf16) \
            .contiguous(memory_format=torch.channels_last)
        w4 = (torch.randn(C, C, 3, 3, device="cuda") / 16).to(bf16)
        packs = {"fwd": w4.permute(0, 2, 3, 1).reshape(C, -1).contiguous(),
                 "dgrad": w4.flip(2, 3).permute(1, 2, 3, 0).reshape(C, -1)
                 .contiguous()}
        for what, w in packs.items():
            sides = {"im2col": side(ext, "im2col", 0, x, w, C),
                     "halo512": side(ext, "halo", 512, x, w, C),
                     "halo256": side(ext, "halo", 256, x, w, C),
                     "auto": side(ext, "auto", 0, x, w, C)}
            if parent is not None:
                sides["parent"] = side(parent, "auto", 0, x, w, C)
            plans = {}
            for k, fn in sides.items():
                y = fn()
                if k != "parent":
                    pl = ext.conv3x3_halo_plan(N, hw, hw, C, C)
                    plans[k] = "{}{}".format(pl["kernel"], pl["BM"])
                if k == "im2col":
                    base = y.double()
                else:
                    d = (y.double() - base).abs().max().item()
                    assert d <= 2.0 ** -7 * base.abs().max().item(), (tag, k)
            spread = {}
            med = ab_median(sides, rounds, iters, spread)
            gflop = 2.0 * N * hw * hw * C * C * 9 / 1e9
            cells = "  ".join("{} {:.4f} ms ({:.0f} TF/s, spread {:.4f})"
                              .format(k, v, gflop / v, spread[k])
                              for k, v in med.items())
            print("{} {} N={}: {} | plans {}".format(tag, what, N, cells,
                                                    plans), flush=True)
            rows.append(dict(tag=tag, what=what, N=N, C=C, hw=hw, ms=med,
                             spread=spread, plans=plans, gflop=gflop))
    os.environ.pop("TFOS_CONV3X3_TILE", None)
    os.environ.pop("TFOS_CONV3X3_HALO_BM", None)
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)),
                    exist_ok=True)
        with open(json_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
