"""Shared by test_gpu_pwconv.py and test_pwconv_cpu.py: the fp64 reference of
the pointwise-conv kernels (csrc/pwconv.hip) and their probe inputs.

The reference is an fp64 einsum on the CPU over the values the kernels see: x
and dy in bf16, the weight rounded to bf16.

Exact probes draw x and dy as integers in [-3, 3] and the weight as k / 8 with
integer |k| <= 63, a different k for neighbouring (co, ci). In units of 1/8 a
forward output sums Cin products of magnitude <= 189 and a dgrad output Cout
of them; a weight gradient sums M = N*H*W integer products of magnitude <= 9.
While those sums stay below 2^24 every fp32 partial sum is exact in any
order, so y and dx are the single bf16 rounding of the fp64 result and dw is
the fp64 result itself.
"""

import torch

BF16 = torch.bfloat16
FP32 = torch.float32
CL = torch.channels_last

# (N, Cin, Cout, H, W); "T" is pwconv_info()["tile_m"].
#   8x8 1x1        one row; one K step that is three quarters padding
#   16x96          K tail 16
#   96x24          Co = 24: one and a half 16-wide tiles; N = 3
#   24x144, 144x32 K tails 24 and 16 after full steps
#   32x16 T, T+1   one M tile exactly, and one row into the second
#   160x960, 960x320, 576x160   Co panels, widest K (the 32-row tile); dgrad
#                  swaps the roles
SHAPES = [
    (1, 8, 8, 1, 1), (1, 16, 96, 3, 5), (3, 96, 24, 5, 3), (3, 24, 144, 5, 3),
    (1, 144, 32, 3, 5), (1, 32, 16, 1, "T"), (1, 32, 16, 1, "T+1"),
    (1, 160, 960, 2, 2), (1, 960, 320, 2, 2), (1, 576, 160, 1, 3),
]


def exact_premise(N, cin, cout, H, W):
    """sum |a||b| per output in grid units, per direction: all < 2^24."""
    return {"fwd": 3 * 63 * cin, "dgrad": 3 * 63 * cout, "wrw": 9 * N * H * W}


def exact_inputs(N, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, cin, H, W), generator=g).to(BF16)
    dy = torch.randint(-3, 4, (N, cout, H, W), generator=g).to(BF16)
    code = (torch.arange(cin * cout, dtype=torch.int64) * 40503 + 12345) % 127
    w = ((code - 63).to(FP32) / 8).view(cout, cin, 1, 1)
    return x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL), w


def real_inputs(N, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=g).to(BF16)
    dy = torch.randn(N, cout, H, W, generator=g).to(BF16)
    w = torch.randn(cout, cin, 1, 1, generator=g) / 4
    return x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL), w


def pw_ref(x, w, dy):
    """fp64 (y, dx, dw) on the CPU; the weight as the kernels see it."""
    x64, dy64 = x.detach().cpu().double(), dy.detach().cpu().double()
    w64 = w.detach().cpu().to(BF16).double()[:, :, 0, 0]
    return (torch.einsum("nchw,oc->nohw", x64, w64),
            torch.einsum("nohw,oc->nchw", dy64, w64),
            torch.einsum("nohw,nchw->oc", dy64, x64))
