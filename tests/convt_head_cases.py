"""Shared by test_gpu_convt_head.py and test_convt_head_cpu.py: the fp64
reference of the transposed-conv head kernels and their probe inputs.

The reference is fp64 ``F.conv_transpose2d(stride=2, padding=1)`` and its
autograd on the CPU, on the values the kernel sees: x and dy in bf16, the
weight rounded to bf16, the bias in fp32.

Exact probes draw x, dy, w and the bias as integers in [-3, 3]. A forward
output sums at most 4*Cin products and a dgrad output at most 16*Cout, each of
magnitude <= 9, so every fp32 partial sum is an integer below 2^24 and the
single rounding to bf16 is the reference's. A weight gradient sums M = N*H*W
pixels of such products, exact in fp32 in any order while 9*M < 2^24; db sums
4*M values of magnitude <= 3. Every (ci, co) pair gets its own filter (the
base-7 digits of a number that a bijection keeps distinct), so a result
landing in a wrong slot cannot pass.
"""

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
FP32 = torch.float32
CL = torch.channels_last


def exact_premise(N, cin, cout, H, W):
    """sum |a||b| per output, per direction: all must stay below 2^24."""
    return {"fwd": 9 * 4 * cin + 3, "dgrad": 9 * 16 * cout,
            "wrw": 9 * N * H * W, "db": 3 * 4 * N * H * W}


def exact_inputs(N, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, cin, H, W), generator=g).to(BF16)
    dy = torch.randint(-3, 4, (N, cout, 2 * H, 2 * W), generator=g).to(BF16)
    # p -> (p * 40503 + 12345) mod 7^16 is a bijection (40503 is coprime to 7)
    code = (torch.arange(cin * cout, dtype=torch.int64) * 40503 + 12345) % 7 ** 16
    digits = torch.stack([(code // 7 ** k) % 7 for k in range(16)], 1)
    w = (digits - 3).to(FP32).view(cin, cout, 4, 4)
    b = torch.randint(-3, 4, (cout,), generator=g).to(FP32)
    return (x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL),
            w, b)


def real_inputs(N, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=g).to(BF16)
    dy = torch.randn(N, cout, 2 * H, 2 * W, generator=g).to(BF16)
    w = torch.randn(cin, cout, 4, 4, generator=g) / 4
    b = torch.randn(cout, generator=g)
    return (x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL),
            w, b)


def ct_ref(x, w, b, dy):
    """fp64 (y, dx, dw, db) on the CPU; the weight as the kernel sees it."""
    x64 = x.detach().cpu().double().contiguous().requires_grad_()
    w64 = w.detach().cpu().to(BF16).double().requires_grad_()
    b64 = b.detach().cpu().double().requires_grad_()
    y = F.conv_transpose2d(x64, w64, b64, 2, 1)
    dx, dw, db = torch.autograd.grad(y, (x64, w64, b64),
                                     dy.detach().cpu().double().contiguous())
    return y.detach(), dx, dw, db
