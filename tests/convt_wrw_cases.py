"""Shared by test_gpu_convt_wrw.py and test_convt_wrw_cpu.py: the probe
shapes of csrc/convt_wrw.hip, their inputs and the fp64 reference.

The reference is the fp64 autograd of ``F.conv_transpose2d(stride=2,
padding=1)`` on the CPU, on the bf16 values the kernel sees. Exact probes draw
x and dy as integers in [-3, 3], every channel its own random pattern, so
every (ci, co) pair has its own filter; a weight gradient sums at most
M = N*H*W products of magnitude <= 9, exact in fp32 in any order while
9*M < 2^24.
"""

import functools

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
CL = torch.channels_last

# id -> ((N, Cin, Cout, H, W), what the plan must say for the id to be true)
CASES = {
    "centre_taps_only": ((1, 8, 8, 1, 1), lambda p, G: p["grid"] == 4),
    "up4_widths_cin_tail_24_odd_w": ((1, 152, 64, 3, 5),
                                     lambda p, G: p["tiles"] == 3),
    "n3_cout_tail_24": ((3, 32, 24, 5, 3),
                        lambda p, G: p["block_rows"] == G),  # 3 images, 1 block
    "two_tiles_each_axis_both_ragged": ((2, 72, 72, 3, 4),
                                        lambda p, G: p["tiles"] == 4),
    "up1_class_less_than_a_k_step": ((1, 320, 512, 2, 2),
                                     lambda p, G: p["tiles"] == 40),
    "three_slabs_ragged_last": (
        (1, 8, 8, 23, 9),
        lambda p, G: p["slabs"] == 3 and G % p["slab_rows"]
        and p["ws_bytes"] == 3 * 64 * 8 * 8),
    "three_blocks_one_slab_ragged_last": (
        (2, 64, 64, 15, 17),
        lambda p, G: p["slabs"] == 1 and p["ws_bytes"] == 0
        and 2 * p["block_rows"] < G < 3 * p["block_rows"]),
    "lds_above_64k": ((1, 64, 64, 6, 100),
                      lambda p, G: 64 * 1024 < p["lds_bytes"] <= 160 * 1024),
}


def exact_premise(N, cin, cout, H, W):
    """sum |x||dy| per output: must stay below 2^24."""
    return 9 * N * H * W


def inputs(shape, exact, seed=0):
    N, cin, cout, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-3, 4, (N, cin, H, W), generator=g)
        dy = torch.randint(-3, 4, (N, cout, 2 * H, 2 * W), generator=g)
    else:
        x = torch.randn(N, cin, H, W, generator=g)
        dy = torch.randn(N, cout, 2 * H, 2 * W, generator=g)
    return (x.to(BF16).contiguous(memory_format=CL),
            dy.to(BF16).contiguous(memory_format=CL))


def wrw_ref(x, dy):
    """fp64 dW [Cin, Cout, 4, 4] on the CPU."""
    w = torch.zeros(x.shape[1], dy.shape[1], 4, 4, dtype=torch.float64,
                    requires_grad=True)
    y = F.conv_transpose2d(x.detach().cpu().double().contiguous(), w,
                           stride=2, padding=1)
    return torch.autograd.grad(y, w, dy.detach().cpu().double().contiguous())[0]


@functools.lru_cache(maxsize=None)
def case(shape, exact):
    """(x, dy, ref, sum |x||dy|) of a probe, computed once; do not modify."""
    x, dy = inputs(shape, exact)
    return x, dy, wrw_ref(x, dy), wrw_ref(x.abs(), dy.abs())
