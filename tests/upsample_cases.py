"""Shared by test_gpu_upsample.py and test_upsample_cpu.py: the fp64 reference
of the bilinear upsampling kernels (csrc/upsample_bilinear.hip), probe inputs
and the bound of the real-valued probes.

Reference: Wy (Hout x Hin) and Wx (Wout x Win) from the index rule in fp64
(coinciding taps add into one column), y = Wy x Wx^T, dx = Wy^T dy Wx, on the
values the kernel sees.

Exact probes: integers in [-3, 3] at power-of-two scales s. src is a multiple
of 1/(2s), every weight product a multiple of 1/(4 sy sx) >= 1/1024; forward
terms are <= 3 and a backward sum <= 3 * 256 * 1024 < 2^24 such units, so any
fp32 summation order is exact and the one rounding is the reference's.

Real probes, |got - ref| <= tol, u = 2^-24, from the kernel's own count:
  fwd  per axis l0 = 1 - l1, a product and the add round: 6u on every term
  bwd  a lane adds m column taps and n row contributions, each with a weight
       rounding and a product: (m + n + 4) u, m and n the largest tap counts
  src  fp32 src is within d = 4u * max(1, src) of fp64's (scale, product,
       subtraction): l1 moves by d, and where floor lands on the other side
       of an integer the taps shift by one with weights still within d.
       Forward: d times the largest difference of neighbouring pixels around
       i0 on the other axis' exact interpolant. Backward: d on columns
       i0 - 1 .. i0 + 2 of the weight matrix, times |dy|.
  plus half an ulp of the output dtype; products of two errors are left out.
"""

import torch

from test_gpu_bn import _half_ulp as half_ulp

BF16 = torch.bfloat16
FP32 = torch.float32
F64 = torch.float64
CL = torch.channels_last

# (N, C, Hin, Win, Hout, Wout, align_corners values, exact too?)
CASES = [
    (1, 8, 5, 7, 10, 14, (False,), True),         # H != W, high-edge double tap
    (3, 21, 3, 2, 48, 32, (False,), True),        # 42-byte pixels at x16, N = 3
    (2, 1, 2, 3, 4, 6, (False,), True),           # C = 1
    (1, 3, 3, 5, 6, 10, (False,), True),          # C = 3, odd W
    (2, 256, 1, 1, 3, 5, (False, True), True),    # 1x1 input: broadcast / sum
    (1, 21, 1, 1, 32, 32, (False, True), True),
    (1, 24, 4, 5, 4, 5, (False, True), True),     # identity
    (1, 8, 4, 5, 4, 10, (False,), True),          # one axis only
    (2, 21, 5, 7, 13, 9, (False, True), False),   # non-dyadic
    (1, 8, 4, 4, 13, 13, (False, True), False),
    (1, 8, 3, 1, 7, 1, (True,), False),           # align_corners scale 0
    (1, 8, 8, 8, 16, 16, (False,), True),         # the backward tile exactly
    (1, 21, 9, 9, 18, 18, (False, True), True),   # ... and a ragged second
    (1, 8, 4, 16, 8, 32, (False,), True),         # the forward tile exactly
    (1, 3, 5, 17, 10, 34, (False,), True),        # ... and a ragged second
    (1, 33, 2, 2, 4, 4, (False,), True),          # past a backward chunk (32)
    (1, 513, 2, 2, 4, 4, (False,), True),         # past a forward chunk (512)
    (1, 32, 1, 5, 2, 80, (False,), True),         # fp32 bwd: dy in two pieces
]


def case_id(c):
    return "{}x{}x{}x{}-{}x{}".format(*c[:6]) if isinstance(c, tuple) else str(c)


def axis_taps(n_in, n_out, align):
    """(src, i0, i1, l1) of every output index, by the rule, in fp64."""
    dst = torch.arange(n_out, dtype=F64)
    if align:
        src = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * dst
    else:
        src = ((n_in / n_out) * (dst + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    return src, i0, i1, src - i0


def axis_matrix(n_in, n_out, align):
    _, i0, i1, l1 = axis_taps(n_in, n_out, align)
    W = torch.zeros(n_out, n_in, dtype=F64)
    r = torch.arange(n_out)
    W.index_put_((r, i0), 1 - l1, accumulate=True)
    W.index_put_((r, i1), l1, accumulate=True)
    return W


def _fwd(Wy, x, Wx):
    return torch.einsum("oh,nchw,pw->ncop", Wy, x, Wx)


def _bwd(Wy, dy, Wx):
    return torch.einsum("oh,ncop,pw->nchw", Wy, dy, Wx)


def ub_ref(x, dy, align):
    """fp64 (y, dx) for x (N, C, Hin, Win) and dy (N, C, Hout, Wout)."""
    Wy = axis_matrix(x.shape[2], dy.shape[2], align)
    Wx = axis_matrix(x.shape[3], dy.shape[3], align)
    return (_fwd(Wy, x.cpu().double(), Wx), _bwd(Wy, dy.cpu().double(), Wx))


def inputs(case, dtype, exact, seed=0):
    N, C, Hin, Win, Hout, Wout = case[:6]
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-3, 4, (N, C, Hin, Win), generator=g).to(dtype)
        dy = torch.randint(-3, 4, (N, C, Hout, Wout), generator=g).to(dtype)
    else:
        x = torch.randn(N, C, Hin, Win, generator=g).to(dtype)
        dy = torch.randn(N, C, Hout, Wout, generator=g).to(dtype)
    return x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL)


def _src_err(n_in, n_out, align):
    """Per output index: d, and the 0/1 matrix of the columns d may touch."""
    src, i0, _, _ = axis_taps(n_in, n_out, align)
    d = 4 * 2.0 ** -24 * src.clamp_min(1)
    cols = torch.arange(n_in)[None, :] - i0[:, None]
    return d, ((cols >= -1) & (cols <= 2)).double()


def _local_diff(a, i0, dim):
    """Largest |a[j] - a[j-1]| for j = i0 .. i0 + 2 along ``dim`` (0 outside
    the image): the pairs either side's taps can be."""
    a = a.movedim(dim, -1)
    pad = torch.zeros_like(a[..., :1])
    d = torch.cat([pad, (a[..., 1:] - a[..., :-1]).abs(), pad, pad], -1)
    return torch.stack([d[..., i0 + k] for k in range(3)]).amax(0).movedim(-1, dim)


def bounds(x, dy, align, dtype):
    """(tol_fwd, tol_bwd) as derived in the module docstring."""
    (Hin, Win), (Hout, Wout) = x.shape[2:], dy.shape[2:]
    x, dy = x.cpu().double(), dy.cpu().double()
    Wy, Wx = axis_matrix(Hin, Hout, align), axis_matrix(Win, Wout, align)
    ey, Ey = _src_err(Hin, Hout, align)
    ex, Ex = _src_err(Win, Wout, align)
    y, dx = _fwd(Wy, x, Wx), _bwd(Wy, dy, Wx)
    eye_h, eye_w = torch.eye(Hin, dtype=F64), torch.eye(Win, dtype=F64)
    tol_f = 3 * 2.0 ** -23 * _fwd(Wy, x.abs(), Wx) + half_ulp(y, dtype) \
        + ey[:, None] * _local_diff(_fwd(eye_h, x, Wx), axis_taps(Hin, Hout, align)[1], 2) \
        + ex * _local_diff(_fwd(Wy, x, eye_w), axis_taps(Win, Wout, align)[1], 3)
    m = int((Wx != 0).sum(0).max()) + int((Wy != 0).sum(0).max())
    tol_b = (m + 4) * 2.0 ** -24 * _bwd(Wy, dy.abs(), Wx) + half_ulp(dx, dtype) \
        + _bwd(Ey * ey[:, None], dy.abs(), Wx) + _bwd(Wy, dy.abs(), Ex * ex[:, None])
    return tol_f, tol_b
