"""Shared by test_gpu_dwconv.py and test_dwconv_cpu.py: the fp64 reference of
the depthwise 3x3 kernels, the exact-probe inputs and the shape list.

The reference is fp64 ``F.conv2d(groups=C)`` and its autograd on the values
the kernel sees: activations rounded to the test dtype, and the weight
rounded to bf16 when the activations are bf16.

Exact probes draw x, dy and w as integers in [-3, 3]. A forward or dgrad
output is a sum of at most 9 products of magnitude at most 9, so every fp32
partial sum is an integer of magnitude <= 81: exact in fp32 and in bf16
(integers up to 256 are bf16 values). A weight gradient is a sum over
M = N*Ho*Wo pixels of such products, magnitude <= 9*M, exact in fp32 in any
summation order while 9*M < 2^24. So the kernels must match the reference
bit for bit. Every channel gets its own filter (the base-7 digits of a
per-channel number that a bijection keeps distinct), so a result landing in
a wrong channel slot cannot pass.
"""

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
FP32 = torch.float32

# (N, C/V, H, W): C is given in vectors of the dtype (8 bf16 / 4 fp32
# channels) unless the entry is in ABS_C below.
#   C = V           one vector, one lane per pixel
#   5x7             H != W, odd
#   7x5, 8x6        stride 2 on odd and even inputs (4x3 outputs; the even one
#                   has asymmetric right and bottom coverage)
#   1x1             only the centre tap is live
#   1x9, 2x2, 2x8   W on both sides of the 4-wide forward strip (outputs of
#                   9, 5 | 2, 1 | 8, 4) and of the stride-2 dgrad pair
#   N = 3           strips and wrw slabs must not run across an image
SMALL = [
    (1, "V", 5, 7),
    (3, "V", 7, 5),
    (2, "V", 8, 6),
    (3, "V", 1, 1),
    (1, "V", 1, 9),
    (1, "V", 2, 2),
    (2, "V", 2, 8),
    (3, 24, 5, 7),     # ragged against a 64-lane wave, bf16 and fp32
    (3, 144, 5, 7),    # a U-Net width, 18 bf16 vectors: wrw runs 2 slabs of
                       # 53 and 52 pixels, the boundary inside image 1
    (1, 960, 4, 4),    # the deepest U-Net layers: 2 channel chunks in wrw
    (2, 960, 9, 9),    # 11 wrw slabs: every finalize lane, ragged
]


def channels(c, dtype):
    return (8 if dtype == BF16 else 4) if c == "V" else c


def out_size(n, stride):
    return (n - 1) // stride + 1


def exact_inputs(N, C, H, W, stride, dtype, device, seed=0):
    """Integer-valued x, dy (in ``dtype``, channels_last) and fp32 w."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).to(dtype)
    dy = torch.randint(-3, 4, (N, C, Ho, Wo), generator=g).to(dtype)
    # c -> (c * 40503 + 12345) mod 7^9 is a bijection (40503 is coprime to
    # 7), so no two channels share a filter
    code = (torch.arange(C, dtype=torch.int64) * 40503 + 12345) % 7 ** 9
    digits = torch.stack([(code // 7 ** k) % 7 for k in range(9)], 1)
    w = (digits - 3).to(FP32).view(C, 1, 3, 3)
    cl = torch.channels_last
    return (x.to(device).contiguous(memory_format=cl),
            dy.to(device).contiguous(memory_format=cl), w.to(device))


def real_inputs(N, C, H, W, stride, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    dy = torch.randn(N, C, Ho, Wo, generator=g).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    cl = torch.channels_last
    return (x.to(device).contiguous(memory_format=cl),
            dy.to(device).contiguous(memory_format=cl), w.to(device))


def seen_weight(w, dtype):
    """The weight values the kernel multiplies by."""
    return w.to(BF16).to(FP32) if dtype == BF16 else w


def dw_ref(x, w, dy, stride):
    """fp64 (y, dx, dw) of the depthwise conv; ``w`` as the kernel sees it."""
    C = x.shape[1]
    x64 = x.double().contiguous().requires_grad_()
    w64 = w.double().contiguous().requires_grad_()
    y = F.conv2d(x64, w64, None, stride, 1, 1, C)
    dx, dw = torch.autograd.grad(y, (x64, w64), dy.double().contiguous())
    return y.detach(), dx, dw
