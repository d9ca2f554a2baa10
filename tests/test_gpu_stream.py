"""Streaming kernels (csrc/maxpool.hip, csrc/elementwise.hip) vs plain fp64.

``maxpool_fwd`` / ``maxpool_bwd``, ``nhwc_pack``, ``sgd_step``, ``adam_step``
and ``pack_bf16`` are driven through the extension entry points (and once
each through their Python wrappers) and compared with fp64 tensor arithmetic
on exactly the values the kernel sees: inputs rounded to the test dtype,
hyperparameters rounded to fp32.  No reference is the code under test or a
library op; the one library call (``F.max_pool2d`` in fp64) cross-checks the
pool reference itself, on the CPU.

u = 2^-24 is the fp32 unit roundoff.  half_ulp(dtype) is half an ulp of the
output dtype at the fp64 reference (the BatchNorm suite's ``_half_ulp``).
The extension is built without fast-math, so +, -, *, / and sqrtf are
correctly rounded; a contracted multiply-add rounds once where the count below
assumes twice, which only lowers its error.  No bound below was fitted to
what a kernel produced.

Exact probes (compared bit for bit; fp32 with the fp64 result, bf16 with its
round-to-nearest-even):
  * pool forward: max and argmax involve no arithmetic at all: ``y`` and
    ``idx`` are exact on any input.  Integer inputs in [-3, 3] put ties in
    nearly every window (first tap in row-major order wins); real inputs give
    every channel its own offset and scale.
  * pool backward: integer ``dy`` in [-3, 3]; a pixel sums at most
    ceil(K/S)^2 <= 16 such values, exact in fp32 and in bf16.
  * nhwc_pack: scale = 1, integer mean, power-of-two std: v - mean is an
    integer below 2^9 and the quotient a short dyadic.
  * sgd_step: integer p, g, m in [-8, 8], lr = mu = 0.5, wd in {0, 0.25}:
    three steps stay short dyadics (premise test).
  * adam_step state: b1 = 0.5, b2 = 0.75, integer g: m and v stay short
    dyadics over three steps (premise test).
  * pack_bf16: a gather and one cast: equal to ``.to(bfloat16)`` bit for bit.

Derived bounds (running error: the same formula in fp64 with every input
replaced by its absolute value and every subtraction by an addition, times u,
times the number of fp32 roundings on the longest path to that output):
  * pool backward, real dy:
        (n_windows - 1) * u * sum|dy over the contributing windows|
        + half_ulp(dtype)
    the kernel adds the contributions one after another into an fp32 zero.
  * nhwc_pack, real: 3 * u * (|v*scale| + |mean_c|) / |std_c| + half_ulp(out)
    (product, difference, quotient).
  * sgd_step (kernel source, per element):
        grad = g + wd*p            2 roundings   G = |g| + wd|p|
        m'   = mu*m + grad         +2 = 4        M = mu|m| + G
        plain:    p' = p - lr*m'   +2 = 6        P = |p| + lr*M
        nesterov: upd = grad+mu*m' +2 = 6
                  p' = p - lr*upd  +2 = 8        P = |p| + lr*(G + mu*M)
    bound(m) = 4uM, bound(p) = 6uP or 8uP.
  * adam_step (kg = 2 with L2 weight decay, grad = g + wd*p; else 0):
        m'  = b1*m + (1.f-b1)*grad     kg + 3        M = b1|m| + (1-b1)G
        v'  = b2*v + (1.f-b2)*grad*grad  2kg + 4     V = b2|v| + (1-b2)G^2
        mhat = m'/bc1                  kg + 5 (bc1 is a rounded float)
        vhat = v'/bc2                  2kg + 6
        den = sqrtf(vhat) + eps        (2kg+6)/2 + 2 = kg + 5
        upd = mhat/den                 (kg+5) + (kg+5) + 1, + 1 spare = 2kg+12
        decoupled: upd += wd*p         + 1
        p'  = p - lr*upd               + 2
    A quotient's error is relative to its true divisor, so the absolute-value
    evaluation keeps the reference's own ``den``:
    A = (M/bc1)/den (+ wd|p|), P = |p| + lr*A.  The error of ``den`` counted
    above is relative to V, not to v'; the inputs keep |g| >= 0.5 so that
    V <= 1.1 v' (asserted), and the spare rounding covers the excess
    (kg+3)*(V/v' - 1) <= 0.5 and every second-order term.  bound(m) = (kg+3)uM, bound(v) = (2kg+4)uV,
    bound(p) = 14uP plain, 18uP with L2, 15uP decoupled.  Each step is
    compared from the kernel's own previous state (one-step error); the
    reference's bias corrections are 1 - b^step in fp64 from the fp32 betas.
    ``test_adam_premise_cpu`` shows an fp32 emulation of these formulas, with
    the corrections formed in double, stays inside the bounds.

Pinned pool semantics: ties go to the first tap in row-major order; a NaN in
a window is its output, and its gradient lands on a NaN tap of that window;
a window whose in-bounds taps are all -inf outputs -inf and gives its
gradient to the first in-bounds tap.
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

BF16 = torch.bfloat16
FP32 = torch.float32
F64 = torch.float64
U = 2.0 ** -24
_DEV = "cuda"
GRID_CAP_THREADS = 2048 * 256        # TFOSR_MAX_GRID blocks of 256 threads
PACK_CAP_THREADS = 16384 * 256       # block cap of tfosr_pack_bf16


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _vec(dtype):
    return 8 if dtype == BF16 else 4


def _dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _half_ulp(ref64, dtype):
    """Half an ulp of ``dtype`` at |ref64|."""
    if dtype == BF16:
        _, e = torch.frexp(ref64)
        half = torch.ldexp(torch.ones_like(ref64), e - 9)
        return torch.where(ref64 == 0, torch.zeros_like(ref64), half)
    return 2.0 ** -24 * ref64.abs()


def _f32(v):
    """A Python float rounded to fp32 (what the binding passes down)."""
    return float(np.float32(v))


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _assert_bits(what, got, ref64):
    """got (fp32 or bf16) is bit-identical to the exactly representable
    fp64 reference."""
    want = ref64.to(got.dtype)
    assert torch.equal(want.double(), ref64), \
        "{}: reference is not representable in {}".format(what, got.dtype)
    bad = got != want
    print("  {:<24s} exact: {} of {} differ".format(
        what, int(bad.sum()), got.numel()))
    assert not bool(bad.any()), "{}: {} of {} elements differ".format(
        what, int(bad.sum()), got.numel())


def _assert_within(what, got, ref64, bound):
    """|got - ref64| <= bound elementwise; prints the worst ratio first."""
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    if got.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "{}: non-finite".format(what)
    err = (got.double() - ref64).abs()
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err > 0, torch.full_like(err, math.inf),
                                    torch.zeros_like(err)))
    worst = float(ratio.max())
    print("  {:<24s} err max {:.3e}  worst err/bound {:.3f}".format(
        what, float(err.max()), worst))
    assert worst <= 1.0, "{}: err/bound {:.3f}".format(what, worst)
    return worst


# ===========================================================================
# 1. max-pool
# ===========================================================================

def _out_hw(H, W, K, S, P):
    return (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1


def _pool_ref(x, K, S, P):
    """Window maximum and its tap index (ky*K + kx), in fp64.

    Taps in row-major order; a tap is taken when it is in bounds and it is
    the first such tap of the window, or beats the best so far, or is NaN."""
    X = x.double()
    N, C, H, W = X.shape
    OH, OW = _out_hw(H, W, K, S, P)
    Xp = X.new_zeros(N, C, H + 2 * P, W + 2 * P)
    Xp[:, :, P:P + H, P:P + W] = X
    inb = torch.zeros(H + 2 * P, W + 2 * P, dtype=torch.bool, device=X.device)
    inb[P:P + H, P:P + W] = True
    best = X.new_full((N, C, OH, OW), -math.inf)
    bidx = torch.full((N, C, OH, OW), -1, dtype=torch.int64, device=X.device)
    for ky in range(K):
        ys = slice(ky, ky + (OH - 1) * S + 1, S)
        for kx in range(K):
            xs = slice(kx, kx + (OW - 1) * S + 1, S)
            v = Xp[:, :, ys, xs]
            take = inb[ys, xs] & ((bidx < 0) | (v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            bidx = torch.where(take, torch.full_like(bidx, ky * K + kx), bidx)
    return best, bidx


def _pool_scatter(vals, bidx, H, W, K, S, P):
    """Each window's value goes to its recorded tap (fp64)."""
    V = vals.double()
    N, C, OH, OW = V.shape
    out = V.new_zeros(N, C, H + 2 * P, W + 2 * P)
    for ky in range(K):
        ys = slice(ky, ky + (OH - 1) * S + 1, S)
        for kx in range(K):
            xs = slice(kx, kx + (OW - 1) * S + 1, S)
            out[:, :, ys, xs] += torch.where(bidx == ky * K + kx, V,
                                             torch.zeros_like(V))
    return out[:, :, P:P + H, P:P + W]


def _tap_to_flat(bidx, W, K, S, P):
    """Tap index -> flat input index ih*W + iw (the library's convention)."""
    OH, OW = bidx.shape[2], bidx.shape[3]
    oh = torch.arange(OH, device=bidx.device)[:, None]
    ow = torch.arange(OW, device=bidx.device)[None, :]
    ih = oh * S - P + bidx // K
    iw = ow * S - P + bidx % K
    return ih * W + iw


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _int_input(shape, dtype, seed, device=_DEV, lo=-3, hi=3):
    g = _gen(seed, device)
    return _cl(torch.randint(lo, hi + 1, shape, device=device, generator=g)
               .to(dtype))


def _real_input(shape, dtype, seed, device=_DEV):
    """Every channel has its own offset and scale."""
    g = _gen(seed, device)
    C = shape[1]
    c = torch.arange(C, device=device, dtype=torch.float32)
    off = (((c * 7) % C) - C / 2.0) * 0.75
    scale = 0.5 + ((c * 3) % C) / C
    x = torch.randn(shape, device=device, generator=g)
    return _cl((x * scale[None, :, None, None]
                + off[None, :, None, None]).to(dtype))


def _edge_planes(dtype, device):
    """2 x V x 9 x 10 for a 3/2/1 pool: -inf planes, NaN planes."""
    C = _vec(dtype)
    x = torch.randn(2, C, 9, 10, device=device, generator=_gen(77, device))
    x[0, 0] = -math.inf                     # every border window
    x[0, 1, 0::2, 0::2] = math.nan          # exactly one NaN per window
    x[0, 2, 1:4, 1:4] = math.nan            # window (1, 1) is all NaN
    x[0, 3, 4, 4] = math.nan                # NaN next to a larger finite
    x[0, 3, 4, 5] = 1e30
    x[1, 0, 0:3, :] = -math.inf             # -inf top rows only
    x[1, 1, :, 0:2] = -math.inf             # -inf left columns only
    x[1, 2, 0, 0] = math.nan                # NaN in a corner window
    x[1, 3] = -math.inf
    x[1, 3, 8, 9] = math.nan                # lone NaN in a -inf plane
    return _cl(x.to(dtype))


def _pool_fwd_check(what, ext, x, K, S, P):
    """Forward is exact: y bit-identical, idx == the reference's tap."""
    N, C, H, W = x.shape
    OH, OW = _out_hw(H, W, K, S, P)
    y, idx = ext.maxpool_fwd(x, K, S, P)
    yr, br = _pool_ref(x, K, S, P)
    assert y.shape == (N, C, OH, OW) and y.dtype == x.dtype
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert idx.shape == (N, OH, OW, C) and idx.dtype == torch.uint8
    _assert_bits(what + " y", y, yr)
    got = idx.permute(0, 3, 1, 2).long()
    bad = got != br
    print("  {:<24s} idx: {} of {} differ".format(what, int(bad.sum()),
                                                  bad.numel()))
    assert not bool(bad.any())
    return y, idx, br


# (K, S, P, H, W)
_POOL_GEOM = {
    "k3s2p1-9x14": (3, 2, 1, 9, 14),
    "k3s2p1-10x7": (3, 2, 1, 10, 7),
    "k3s2p0-8x11": (3, 2, 0, 8, 11),     # row 7 belongs to no window
    "k2s2p0-6x9": (2, 2, 0, 6, 9),
    "k3s1p1-5x7": (3, 1, 1, 5, 7),       # every pixel in 9 windows
    "k2s3p0-8x10": (2, 3, 0, 8, 10),     # K < S: gaps between windows
    "k5s2p2-9x12": (5, 2, 2, 9, 12),
    "k7s2p3-11x16": (7, 2, 3, 11, 16),
    "k3s2p1-1x1": (3, 2, 1, 1, 1),
}


def _pool_cases():
    out = []
    for i, (name, geom) in enumerate(_POOL_GEOM.items()):
        for dtype in (BF16, FP32):
            # alternate minimum C with C = 24, and N = 1 with N = 3, so that
            # every geometry sees both with one dtype or the other
            minc = (i + (dtype == FP32)) % 2 == 0
            C = _vec(dtype) if minc else 24
            N = 1 if minc else 3
            out.append(pytest.param(
                dtype, N, C, geom,
                id="{}-{}x{}-{}".format(_dname(dtype), N, C, name)))
    return out


def test_pool_reference_matches_library_cpu():
    """The fp64 helper against F.max_pool2d(return_indices=True) in fp64,
    -inf and NaN inputs included."""
    for name, (K, S, P, H, W) in _POOL_GEOM.items():
        for maker in (_int_input, _real_input):
            x = maker((2, 5, H, W), F64, 11, device="cpu").contiguous()
            yr, br = _pool_ref(x, K, S, P)
            yl, il = F.max_pool2d(x, K, S, P, return_indices=True)
            assert torch.equal(yr, yl), name
            assert torch.equal(_tap_to_flat(br, W, K, S, P), il), name
    x = _edge_planes(FP32, "cpu").double().contiguous()
    yr, br = _pool_ref(x, 3, 2, 1)
    yl, il = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert torch.equal(torch.isnan(yr), torch.isnan(yl))
    assert torch.equal(torch.nan_to_num(yr, nan=7.0),
                       torch.nan_to_num(yl, nan=7.0))
    assert torch.equal(_tap_to_flat(br, 10, 3, 2, 1), il)
    # backward helper: the library's gradient of sum(w * y)
    for K, S, P, H, W in (_POOL_GEOM["k3s2p1-9x14"], _POOL_GEOM["k3s1p1-5x7"],
                          _POOL_GEOM["k2s3p0-8x10"]):
        x = _real_input((2, 5, H, W), F64, 12, device="cpu").contiguous()
        x.requires_grad_(True)
        y = F.max_pool2d(x, K, S, P)
        dy = torch.randint(-3, 4, y.shape).double()
        (y * dy).sum().backward()
        _, br = _pool_ref(x.detach(), K, S, P)
        assert torch.equal(_pool_scatter(dy, br, H, W, K, S, P), x.grad)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,N,C,geom", _pool_cases())
def test_maxpool_forward_exact(dtype, N, C, geom):
    K, S, P, H, W = geom
    ext = _ext()
    _pool_fwd_check("ties", ext, _int_input((N, C, H, W), dtype, 21), K, S, P)
    _pool_fwd_check("real", ext, _real_input((N, C, H, W), dtype, 22), K, S, P)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,N,C,geom", _pool_cases())
def test_maxpool_backward_exact(dtype, N, C, geom):
    """Integer dy: dx bit for bit, and exactly 0 where no window reaches."""
    K, S, P, H, W = geom
    ext = _ext()
    for maker in (_int_input, _real_input):
        x = maker((N, C, H, W), dtype, 23)
        y, idx, br = _pool_fwd_check(maker.__name__, ext, x, K, S, P)
        dy = _int_input(tuple(y.shape), dtype, 24)
        dx = ext.maxpool_bwd(dy, idx, H, W, K, S, P)
        assert dx.shape == x.shape and dx.dtype == dtype
        assert dx.is_contiguous(memory_format=torch.channels_last)
        _assert_bits("dx", dx, _pool_scatter(dy, br, H, W, K, S, P))
    if (K, S, P, H) == (3, 2, 0, 8):
        assert float(dx[:, :, 7, :].abs().max()) == 0.0
    if (K, S, P) == (2, 3, 0):
        assert float(dx[:, :, 2::3, :].abs().max()) == 0.0
        assert float(dx[:, :, :, 2::3].abs().max()) == 0.0


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,N,C,geom", _pool_cases())
def test_maxpool_backward_real(dtype, N, C, geom):
    K, S, P, H, W = geom
    ext = _ext()
    x = _int_input((N, C, H, W), dtype, 25)      # ties: many shared pixels
    y, idx, br = _pool_fwd_check("fwd", ext, x, K, S, P)
    dy = _real_input(tuple(y.shape), dtype, 26)
    dx = ext.maxpool_bwd(dy, idx, H, W, K, S, P)
    ref = _pool_scatter(dy, br, H, W, K, S, P)
    sabs = _pool_scatter(dy.double().abs(), br, H, W, K, S, P)
    nwin = _pool_scatter(torch.ones_like(dy), br, H, W, K, S, P)
    assert float(nwin.max()) <= math.ceil(K / S) ** 2
    bound = (nwin - 1).clamp_min(0) * U * sabs + _half_ulp(ref, dtype)
    _assert_within("dx", dx, ref, bound)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_dname)
def test_maxpool_grid_stride(dtype):
    """2 x V x 1025 x 1025, 3/2/1: 526338 forward threads, 2818 past
    TFOSR_MAX_GRID x 256, so the last stride is ragged; the backward's
    2.1 M threads stride four times."""
    ext = _ext()
    N, C, H, W, K, S, P = 2, _vec(dtype), 1025, 1025, 3, 2, 1
    OH, OW = _out_hw(H, W, K, S, P)
    nthr = N * OH * OW * C // _vec(dtype)
    assert GRID_CAP_THREADS < nthr < 2 * GRID_CAP_THREADS
    assert nthr % GRID_CAP_THREADS != 0
    assert N * H * W > 4 * GRID_CAP_THREADS
    x = _real_input((N, C, H, W), dtype, 31)
    x[:, :, ::5, ::3] = 2.0                      # some ties as well
    y, idx, br = _pool_fwd_check("grid-stride", ext, x, K, S, P)
    dy = _int_input(tuple(y.shape), dtype, 32)
    dx = ext.maxpool_bwd(dy, idx, H, W, K, S, P)
    _assert_bits("dx", dx, _pool_scatter(dy, br, H, W, K, S, P))


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_dname)
def test_maxpool_edge_values(dtype):
    """-inf planes and NaN windows, forward and backward.

    Measured on the MI355X with the forward as it was (``bidx`` starting at
    tap 0, ``v > best`` alone), where this test failed for both dtypes: all
    37 NaN windows output a finite value or -inf, 28 of the 59 all -inf
    windows (the top and left border ones) recorded tap 0 in the padding,
    and 54 (bf16) / 55 (fp32) of sum(dy) never reached dx.  With the
    sentinel start index and ``v != v`` all three figures are 0."""
    ext = _ext()
    K, S, P = 3, 2, 1
    x = _edge_planes(dtype, _DEV)
    N, C, H, W = x.shape
    y, idx = ext.maxpool_fwd(x, K, S, P)
    yr, br = _pool_ref(x, K, S, P)
    nanw = torch.isnan(yr)
    infw = yr == -math.inf
    lost = int((torch.isnan(y) != nanw).sum())
    got = idx.permute(0, 3, 1, 2).long()
    bad = (got != br) & ~nanw
    dy = _int_input(tuple(y.shape), dtype, 41, lo=1, hi=3)
    dx = ext.maxpool_bwd(dy, idx, H, W, K, S, P)
    gone = float(dy.double().sum() - dx.double().sum())
    print("  NaN windows {}: laundered or invented {};  -inf windows {}: "
          "with another tap than the first in bounds {};  other windows "
          "with a wrong tap {};  sum(dy) - sum(dx) = {}".format(
              int(nanw.sum()), lost, int(infw.sum()), int((bad & infw).sum()),
              int((bad & ~infw).sum()), gone))
    assert lost == 0, "y is NaN in other places than the reference"
    assert torch.equal(torch.nan_to_num(y.double(), nan=7.0),
                       torch.nan_to_num(yr, nan=7.0))
    # finite and -inf windows: the tap is the reference's (first in bounds)
    assert not bool(bad.any())
    # NaN windows: some in-bounds NaN tap of that window
    OH, OW = yr.shape[2], yr.shape[3]
    oh = torch.arange(OH, device=_DEV)[:, None]
    ow = torch.arange(OW, device=_DEV)[None, :]
    ih = oh * S - P + got // K
    iw = ow * S - P + got % K
    inb = (got < K * K) & (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    assert bool(inb.all()), "a window recorded a tap in the padding"
    flat = (ih * W + iw).reshape(N, C, -1)
    tapv = x.double().reshape(N, C, -1).gather(2, flat).reshape(yr.shape)
    assert bool(torch.isnan(tapv)[nanw].all()), \
        "a NaN window's tap does not point at a NaN"
    # backward, integer dy: every window's dy arrives somewhere, exactly
    assert bool(torch.isfinite(dx).all())
    _assert_bits("dx", dx, _pool_scatter(dy, got, H, W, K, S, P))
    assert gone == 0.0
    # -inf planes: the first in-bounds tap of window (0, 0) is pixel (0, 0)
    assert float(dx[0, 0, 0, 0]) == float(dy[0, 0, 0, 0])
    # the NaN at (4, 4) beats the 1e30 next to it in window (2, 2)
    assert bool(torch.isnan(y[0, 3, 2, 2])) and float(y[0, 3, 2, 3]) > 1e29
    assert float(dx[0, 3, 4, 4]) == float(dy[0, 3, 2, 2])


@gpu
@requires_gpu
def test_maxpool_expanded_grad():
    """y.sum().backward(): the incoming gradient is a stride-0 expand; dx is
    the exact count of windows that selected each pixel."""
    from tensorflowonspark_amd.ops.modules import FusedMaxPool2d
    for dtype in (BF16, FP32):
        x = _int_input((2, 16, 9, 14), dtype, 51).requires_grad_(True)
        y = FusedMaxPool2d(3, 2, 1)(x)
        assert type(y.grad_fn).__name__ == "_MaxPoolFnBackward"
        y.sum().backward()
        _, br = _pool_ref(x.detach(), 3, 2, 1)
        cnt = _pool_scatter(torch.ones_like(y.detach()), br, 9, 14, 3, 2, 1)
        _assert_bits("dx count", x.grad, cnt)


@gpu
@requires_gpu
def test_fused_maxpool_module_wiring():
    """In-tree route exactly when eligible; library route otherwise; the
    same values give the same result on both."""
    from tensorflowonspark_amd.ops.modules import FusedMaxPool2d
    pool = FusedMaxPool2d(3, 2, 1)

    grad = _int_input((2, 16, 5, 7), FP32, 62)

    def run(x):
        x = x.detach().requires_grad_(True)
        y = pool(x)
        dy = grad[:, :x.shape[1]].to(device=x.device, dtype=x.dtype)
        y.backward(dy)
        return y, x.grad, type(y.grad_fn).__name__

    lib = "MaxPool2DWithIndicesBackward0"
    base = _int_input((2, 16, 9, 14), BF16, 61)
    y0, g0, name = run(base)
    assert name == "_MaxPoolFnBackward"
    y1, g1, name = run(base.contiguous())                 # NCHW-contiguous
    assert name == lib
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    y2, g2, name = run(base.float().cpu())                # CPU
    assert name == lib
    assert torch.equal(y0.float().cpu(), y2)
    assert torch.equal(g0.float().cpu(), g2)
    y3, g3, name = run(_cl(base.float()))                 # fp32, C % 4 == 0
    assert name == "_MaxPoolFnBackward"
    assert torch.equal(y0.float(), y3) and torch.equal(g0.float(), g3)
    odd = _int_input((2, 12, 9, 14), BF16, 63)            # bf16, C = 12
    y4, g4, name = run(odd)
    assert name == lib
    yr, br = _pool_ref(odd, 3, 2, 1)
    _assert_bits("fallback y", y4, yr)


# ===========================================================================
# 2. nhwc_pack
# ===========================================================================

def _pack_ref(x_u8, mean, std, scale):
    """(N, C, H, W) fp64 from the fp32 values the kernel reads."""
    v = x_u8.double() * _f32(scale)
    return ((v - mean.double()) / std.double()).permute(0, 3, 1, 2)


def _pack_bound(x_u8, mean, std, scale, ref, out_dtype):
    v = (x_u8.double() * _f32(scale)).abs()
    e = 3 * U * (v + mean.double().abs()) / std.double().abs()
    return e.permute(0, 3, 1, 2) + _half_ulp(ref, out_dtype)


def _pack_inputs(shape, seed, device=_DEV):
    C = shape[3]
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device=device,
                      generator=_gen(seed, device))
    c = torch.arange(C, device=device, dtype=torch.float32)
    return x, c


def _exact_stats(c):
    mean = ((c * 3) % 7) - 2.0                     # integers in [-2, 4]
    std = torch.ldexp(torch.ones_like(c), (((c * 5) % 6) - 2).int())
    return mean, std


def _real_stats(c):
    C = c.numel()
    mean = 0.35 + 0.3 * ((c * 2) % C) / C + 0.011 * c
    std = 0.2 + 0.15 * ((c * 3) % C) / C + 0.007 * c
    return mean.float(), std.float()


def _check_pack_layout(out, channels_last, out_dtype, shape):
    N, H, W, C = shape
    assert out.shape == (N, C, H, W) and out.dtype == out_dtype
    if channels_last:
        assert out.is_contiguous(memory_format=torch.channels_last)
    else:
        assert out.is_contiguous()


# (N, H, W, C): total and total % 16 in the comments
_PACK_SHAPES = [
    (1, 2, 3, 1),      # 6: tail only, one block
    (1, 1, 3, 3),      # 9: tail only
    (1, 4, 7, 1),      # 28: % 16 = 12
    (1, 4, 5, 3),      # 60: % 16 = 12
    (2, 5, 8, 3),      # 240: % 16 = 0
    (2, 23, 31, 3),    # 4278: two blocks of vectors, % 16 = 6
    (3, 7, 9, 4),      # 756
    (4, 4, 7, 5),      # 560: % 16 = 0
    (2, 6, 11, 5),     # 660
    (1, 3, 5, 16),     # 240: % 16 = 0
    (3, 5, 7, 16),     # 1680
]


def test_nhwc_pack_exact_premise_cpu():
    """With scale 1, integer mean and power-of-two std every intermediate is
    an fp32 number, so fp32 evaluation (contracted or not) equals fp64."""
    for shape in _PACK_SHAPES:
        x, c = _pack_inputs(shape, 5, device="cpu")
        mean, std = _exact_stats(c)
        assert torch.equal(mean, mean.round()) and mean.abs().max() <= 4
        m, e = torch.frexp(std)
        assert bool((m == 0.5).all())
        diff = x.double() - mean.double()
        assert torch.equal(diff.float().double(), diff)
        ref = _pack_ref(x, mean, std, 1.0)
        assert torch.equal(ref.float().double(), ref)
        f32 = ((x.float() * 1.0 - mean) / std).permute(0, 3, 1, 2)
        assert torch.equal(f32.double(), ref)


@gpu
@requires_gpu
@pytest.mark.parametrize("shape", _PACK_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("out_dtype", [BF16, FP32], ids=_dname)
@pytest.mark.parametrize("channels_last", [True, False], ids=["cl", "nchw"])
def test_nhwc_pack_matrix(channels_last, out_dtype, shape):
    ext = _ext()
    x, c = _pack_inputs(shape, 71)
    # exact probe
    mean, std = _exact_stats(c)
    out = ext.nhwc_pack(x, mean, std, 1.0, out_dtype == BF16, channels_last)
    _check_pack_layout(out, channels_last, out_dtype, shape)
    ref = _pack_ref(x, mean, std, 1.0)
    if out_dtype == FP32:
        _assert_bits("exact", out, ref)
    else:
        want = ref.float().to(BF16)
        assert torch.equal(out, want), "{} differ".format(
            int((out != want).sum()))
    # real probe
    mean, std = _real_stats(c)
    out = ext.nhwc_pack(x, mean, std, 1.0 / 255, out_dtype == BF16,
                        channels_last)
    _check_pack_layout(out, channels_last, out_dtype, shape)
    ref = _pack_ref(x, mean, std, 1.0 / 255)
    _assert_within("real", out, ref,
                   _pack_bound(x, mean, std, 1.0 / 255, ref, out_dtype))


@gpu
@requires_gpu
@pytest.mark.parametrize("out_dtype", [BF16, FP32], ids=_dname)
@pytest.mark.parametrize("channels_last,shape", [
    (True, (57, 224, 224, 3)),     # total/16 = 536256 > 2048*256 vectors
    (False, (4, 224, 224, 3)),     # total = 602112 > 2048*256 elements
], ids=["cl-57x224x224x3", "nchw-4x224x224x3"])
def test_nhwc_pack_grid_stride(channels_last, shape, out_dtype):
    ext = _ext()
    total = shape[0] * shape[1] * shape[2] * shape[3]
    nthr = total // 16 if channels_last else total
    assert GRID_CAP_THREADS < nthr < 2 * GRID_CAP_THREADS
    x, c = _pack_inputs(shape, 72)
    mean, std = _exact_stats(c)
    out = ext.nhwc_pack(x, mean, std, 1.0, out_dtype == BF16, channels_last)
    _check_pack_layout(out, channels_last, out_dtype, shape)
    ref = _pack_ref(x, mean, std, 1.0)
    assert torch.equal(out, ref.float().to(out_dtype))
    del out, ref
    mean, std = _real_stats(c)
    out = ext.nhwc_pack(x, mean, std, 1.0 / 255, out_dtype == BF16,
                        channels_last)
    ref = _pack_ref(x, mean, std, 1.0 / 255)
    _assert_within("real", out, ref,
                   _pack_bound(x, mean, std, 1.0 / 255, ref, out_dtype))


@gpu
@requires_gpu
def test_nhwc_pack_wrapper_defaults():
    """Python wrapper: None defaults, a strided mean view, an fp64 mean and
    a CPU mean all reach the kernel as fp32 contiguous device vectors."""
    from tensorflowonspark_amd.ops.modules import nhwc_pack
    shape = (2, 5, 7, 3)
    x, c = _pack_inputs(shape, 73)
    zeros, ones = torch.zeros_like(c), torch.ones_like(c)
    mean, std = _real_stats(c)

    def check(what, out, m, s, dt, cl):
        _check_pack_layout(out, cl, dt, shape)
        ref = _pack_ref(x, m, s, 1.0 / 255)
        _assert_within(what, out, ref,
                       _pack_bound(x, m, s, 1.0 / 255, ref, dt))

    check("defaults", nhwc_pack(x, out_dtype=FP32), zeros, ones, FP32, False)
    check("mean only", nhwc_pack(x, mean=mean, channels_last=True),
          mean, ones, BF16, True)
    check("std only", nhwc_pack(x, std=std, out_dtype=FP32),
          zeros, std, FP32, False)
    wide = torch.stack([mean, mean + 100.0], dim=1).reshape(-1)  # m0 j m1 j..
    assert not wide[::2].is_contiguous()
    check("strided mean", nhwc_pack(x, wide[::2], std, out_dtype=FP32),
          mean, std, FP32, False)
    check("fp64 stats", nhwc_pack(x, mean.double(), std.double(),
                                  out_dtype=FP32, channels_last=True),
          mean, std, FP32, True)
    check("cpu stats", nhwc_pack(x, mean.cpu(), std.cpu(), out_dtype=FP32),
          mean, std, FP32, False)


# ===========================================================================
# 3. sgd_step
# ===========================================================================

_OPT_SIZES = [0, 1, 3, 4, 5, 10007, 4 * GRID_CAP_THREADS + 3]


def _sgd_formula(p, g, m, lr, mu, wd, nesterov):
    """The update in the dtype of its arguments; returns (p', m')."""
    grad = g + wd * p
    m2 = mu * m + grad
    upd = grad + mu * m2 if nesterov else m2
    return p - lr * upd, m2


def _sgd_check(what, got_p, got_m, p0, g, m0, lr, mu, wd, nesterov):
    lr, mu, wd = _f32(lr), _f32(mu), _f32(wd)
    P, G, M = p0.double(), g.double(), m0.double()
    rp, rm = _sgd_formula(P, G, M, lr, mu, wd, nesterov)
    aG = G.abs() + wd * P.abs()
    aM = mu * M.abs() + aG
    if nesterov:
        bp = 8 * U * (P.abs() + lr * (aG + mu * aM))
    else:
        bp = 6 * U * (P.abs() + lr * aM)
    _assert_within(what + " m", got_m, rm, 4 * U * aM)
    _assert_within(what + " p", got_p, rp, bp)


def _int_vec(n, seed, device=_DEV, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, (n,), device=device,
                         generator=_gen(seed, device)).float()


def test_sgd_exact_premise_cpu():
    """Integer p, g, m in [-8, 8] with lr = mu = 0.5 and wd in {0, 0.25}:
    three steps evaluated in fp32, one rounding per operation, equal fp64."""
    for nesterov in (False, True):
        for wd in (0.0, 0.25):
            p, m = _int_vec(4096, 1, "cpu"), _int_vec(4096, 2, "cpu")
            P, M = p.double(), m.double()
            for step in range(3):
                g = _int_vec(4096, 3 + step, "cpu")
                p, m = _sgd_formula(p, g, m, 0.5, 0.5, wd, nesterov)
                P, M = _sgd_formula(P, g.double(), M, 0.5, 0.5, wd, nesterov)
                assert p.dtype == FP32
                assert torch.equal(p.double(), P)
                assert torch.equal(m.double(), M)


@gpu
@requires_gpu
@pytest.mark.parametrize("wd", [0.0, 0.25], ids=["wd0", "wd.25"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("n", _OPT_SIZES)
def test_sgd_exact(n, nesterov, wd):
    ext = _ext()
    p, m = _int_vec(n, 81), _int_vec(n, 82)
    P, M = p.double(), m.double()
    for step in range(3):
        g = _int_vec(n, 83 + step)
        ext.sgd_step(p, g, m, 0.5, 0.5, wd, nesterov)
        P, M = _sgd_formula(P, g.double(), M, 0.5, 0.5, wd, nesterov)
        _assert_bits("p step {}".format(step + 1), p, P)
        _assert_bits("m step {}".format(step + 1), m, M)


@gpu
@requires_gpu
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("n", _OPT_SIZES)
def test_sgd_real(n, nesterov):
    ext = _ext()
    gen = _gen(84, _DEV)
    p = torch.randn(n, device=_DEV, generator=gen)
    m = torch.randn(n, device=_DEV, generator=gen)        # nonzero momentum
    for step in range(3):
        g = torch.randn(n, device=_DEV, generator=gen)
        p0, m0 = p.clone(), m.clone()
        ext.sgd_step(p, g, m, 0.1, 0.9, 1e-4, nesterov)
        _sgd_check("step {}".format(step + 1), p, m, p0, g, m0,
                   0.1, 0.9, 1e-4, nesterov)


def _tiny_engine():
    from tensorflowonspark_amd.parallel import DDPEngine
    torch.manual_seed(9)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(),
                                torch.nn.Linear(7, 3)).to(_DEV)
    engine = DDPEngine(model, flatten_params=True)
    assert len(engine._buckets) == 1
    b = engine._buckets[0]
    assert b.param_flat is not None and b.param_flat.is_cuda
    assert b.param_flat.numel() == 5 * 7 + 7 + 7 * 3 + 3
    return model, engine, b


def _params_are_views(bucket):
    flat = torch.cat([p.data.reshape(-1) for p in bucket.params])
    return torch.equal(flat, bucket.param_flat)


@gpu
@requires_gpu
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_bucket_sgd_wiring(nesterov):
    from tensorflowonspark_amd.ops.modules import BucketSGD
    model, engine, b = _tiny_engine()
    opt = BucketSGD(engine, lr=0.1, momentum=0.9, weight_decay=1e-4,
                    nesterov=nesterov)
    gen = _gen(85, _DEV)
    for step in range(2):
        opt.zero_grad()
        xin = torch.randn(4, 5, device=_DEV, generator=gen)
        model(xin).square().sum().backward()
        engine.finalize_backward()
        assert float(b.buffer.abs().max()) > 0        # grads are in the bucket
        p0, g, m0 = b.param_flat.clone(), b.buffer.clone(), opt._mom[0].clone()
        if step == 1:
            assert float(m0.abs().max()) > 0
        opt.step()
        _sgd_check("step {}".format(step + 1), b.param_flat, opt._mom[0],
                   p0, g, m0, 0.1, 0.9, 1e-4, nesterov)
        assert _params_are_views(b)


# ===========================================================================
# 4. adam_step
# ===========================================================================

_ADAM_VARIANTS = {          # wd, decoupled
    "plain": (0.0, False),
    "l2": (0.01, False),
    "decoupled": (0.01, True),
}


def _adam_formula(p, g, m, v, hp, sqrt):
    """One Adam step in the type of its arguments, operation by operation as
    the kernel writes it; ``hp`` holds typed scalars."""
    grad = g if hp["decoupled"] else g + hp["wd"] * p
    m2 = hp["b1"] * m + (hp["one"] - hp["b1"]) * grad
    v2 = hp["b2"] * v + (hp["one"] - hp["b2"]) * grad * grad
    upd = (m2 / hp["bc1"]) / (sqrt(v2 / hp["bc2"]) + hp["eps"])
    if hp["decoupled"]:
        upd = upd + hp["wd"] * p
    return p - hp["lr"] * upd, m2, v2


def _adam_hp(lr, b1, b2, eps, wd, step, decoupled, cast=float):
    """Hyperparameters as fp32 values; bias corrections 1 - b^step in double
    from the fp32 betas, then cast (float: kept in double; np.float32:
    rounded once, as the launcher passes them)."""
    b1, b2 = _f32(b1), _f32(b2)
    return {"lr": cast(_f32(lr)), "b1": cast(b1), "b2": cast(b2),
            "eps": cast(_f32(eps)), "wd": cast(_f32(wd)), "one": cast(1.0),
            "bc1": cast(1.0 - b1 ** step), "bc2": cast(1.0 - b2 ** step),
            "decoupled": decoupled}


def _adam_bounds(p0, g, m0, v0, hp):
    """(ref p, m, v), (bound p, m, v) in fp64 from fp32 state tensors or
    arrays; see the module docstring for the counts."""
    P, G, M0, V0 = (torch.as_tensor(t).double() for t in (p0, g, m0, v0))
    rp, rm, rv = _adam_formula(P, G, M0, V0, hp, torch.sqrt)
    l2 = (not hp["decoupled"]) and hp["wd"] != 0
    kg = 2 if l2 else 0
    aG = G.abs() + (hp["wd"] * P.abs() if l2 else 0)
    aM = hp["b1"] * M0.abs() + (1.0 - hp["b1"]) * aG
    aV = hp["b2"] * V0.abs() + (1.0 - hp["b2"]) * aG * aG
    if P.numel():
        assert float((aV / rv).max()) <= 1.1       # see docstring
    den = torch.sqrt(rv / hp["bc2"]) + hp["eps"]
    aU = (aM / hp["bc1"]) / den
    cnt = 2 * kg + 12
    if hp["decoupled"]:
        aU = aU + hp["wd"] * P.abs()
        cnt += 1
    bp = (cnt + 2) * U * (P.abs() + hp["lr"] * aU)
    return (rp, rm, rv), (bp, (kg + 3) * U * aM, (2 * kg + 4) * U * aV)


def _adam_inputs(n, seed, device=_DEV):
    """|p| ~ 1e-2 so that lr * |update| ~ 0.1 dominates p; |g| in [0.5, 1.5)
    with random sign."""
    gen = _gen(seed, device)
    p = 1e-2 * torch.randn(n, device=device, generator=gen)

    def grad():
        mag = 0.5 + torch.rand(n, device=device, generator=gen)
        sign = torch.randint(0, 2, (n,), device=device, generator=gen) * 2 - 1
        return mag * sign

    return p, grad


def test_adam_premise_cpu():
    """numpy fp32 emulation of the kernel's formulas, every operation rounded
    on its own, bias corrections formed in double and rounded once: inside
    the bounds at steps 1-5 for every variant.  The fp32 ``1 - b^step``
    variant is printed next to it."""
    n = 20000
    for name, (wd, decoupled) in _ADAM_VARIANTS.items():
        p, grad = _adam_inputs(n, 90, "cpu")
        p = p.numpy()
        m = np.zeros(n, np.float32)
        v = np.zeros(n, np.float32)
        for step in range(1, 6):
            g = grad().numpy()
            hp64 = _adam_hp(0.1, 0.9, 0.999, 1e-8, wd, step, decoupled)
            hp32 = _adam_hp(0.1, 0.9, 0.999, 1e-8, wd, step, decoupled,
                            cast=np.float32)
            (rp, rm, rv), (bp, bm, bv) = _adam_bounds(p, g, m, v, hp64)
            p2, m2, v2 = _adam_formula(p, g, m, v, hp32, np.sqrt)
            assert p2.dtype == np.float32 and v2.dtype == np.float32
            old = dict(hp32)
            old["bc1"] = np.float32(1) - np.power(hp32["b1"], np.float32(step))
            old["bc2"] = np.float32(1) - np.power(hp32["b2"], np.float32(step))
            p_old, _, _ = _adam_formula(p, g, m, v, old, np.sqrt)
            ratios = [float(((torch.as_tensor(a).double() - r).abs() / b).max())
                      for a, r, b in ((p2, rp, bp), (m2, rm, bm), (v2, rv, bv),
                                      (p_old, rp, bp))]
            print("  {:<9s} step {}  p {:.3f}  m {:.3f}  v {:.3f}   "
                  "p with fp32 corrections {:.3f}".format(name, step, *ratios))
            assert max(ratios[:3]) <= 1.0, (name, step, ratios)
            p, m, v = p2, m2, v2


def test_adam_state_premise_cpu():
    """b1 = 0.5, b2 = 0.75, integer g: m and v in fp32 equal fp64."""
    m = torch.zeros(4096)
    v = torch.zeros(4096)
    M, V = m.double(), v.double()
    p = torch.zeros(4096)
    for step in range(1, 4):
        g = _int_vec(4096, 91 + step, "cpu")
        hp = _adam_hp(0.125, 0.5, 0.75, 1e-8, 0.0, step, False)
        _, m, v = _adam_formula(p, g, m, v, hp, torch.sqrt)
        _, M, V = _adam_formula(p.double(), g.double(), M, V, hp, torch.sqrt)
        assert m.dtype == FP32 and v.dtype == FP32
        assert torch.equal(m.double(), M) and torch.equal(v.double(), V)


def _adam_check(what, p, m, v, p0, g, m0, v0, hp):
    (rp, rm, rv), (bp, bm, bv) = _adam_bounds(p0, g, m0, v0, hp)
    rm_ = _assert_within(what + " m", m, rm, bm)
    rv_ = _assert_within(what + " v", v, rv, bv)
    rp_ = _assert_within(what + " p", p, rp, bp)
    return max(rm_, rv_, rp_)


@gpu
@requires_gpu
@pytest.mark.parametrize("n", _OPT_SIZES)
def test_adam_state_exact(n):
    ext = _ext()
    p = 1e-2 * torch.randn(n, device=_DEV, generator=_gen(92, _DEV))
    m = torch.zeros(n, device=_DEV)
    v = torch.zeros(n, device=_DEV)
    M, V = m.double(), v.double()
    for step in range(1, 4):
        g = _int_vec(n, 92 + step)
        ext.adam_step(p, g, m, v, 0.125, 0.5, 0.75, 1e-8, 0.0, step, False)
        hp = _adam_hp(0.125, 0.5, 0.75, 1e-8, 0.0, step, False)
        _, M, V = _adam_formula(p.double(), g.double(), M, V, hp, torch.sqrt)
        _assert_bits("m step {}".format(step), m, M)
        _assert_bits("v step {}".format(step), v, V)
        assert bool(torch.isfinite(p).all())


@gpu
@requires_gpu
@pytest.mark.parametrize("variant", list(_ADAM_VARIANTS))
def test_adam_real(variant):
    """Steps 1-5, each from the kernel's own previous state.

    Measured on the MI355X, worst err/bound in p at steps 1-5:
      bias corrections as fp32 ``1.f - powf(b, step)`` (this test failed):
        plain 0.216 2.585 2.566 3.785 2.897, l2 0.186 2.033 1.921 2.914 2.295,
        decoupled 0.245 2.490 2.358 3.500 2.722
      both corrections formed in double (passes):
        plain 0.216 0.142 0.130 0.234 0.199, l2 0.186 0.128 0.111 0.170 0.155,
        decoupled 0.245 0.139 0.120 0.217 0.196"""
    ext = _ext()
    wd, decoupled = _ADAM_VARIANTS[variant]
    n = 10007
    p, grad = _adam_inputs(n, 93)
    m = torch.zeros(n, device=_DEV)
    v = torch.zeros(n, device=_DEV)
    worst = {"p": [], "m": [], "v": []}
    for step in range(1, 6):
        g = grad()
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        ext.adam_step(p, g, m, v, 0.1, 0.9, 0.999, 1e-8, wd, step, decoupled)
        hp = _adam_hp(0.1, 0.9, 0.999, 1e-8, wd, step, decoupled)
        refs, bounds = _adam_bounds(p0, g, m0, v0, hp)
        for key, got, ref, bound in zip("pmv", (p, m, v), refs, bounds):
            assert bool(torch.isfinite(got).all())
            worst[key].append(float(((got.double() - ref).abs() / bound).max()))
    for key in "pmv":            # all fifteen figures first, then the verdict
        print("  {} worst {} err/bound at steps 1-5: {}".format(
            variant, key, " ".join("{:.3f}".format(w) for w in worst[key])))
    for key in "pmv":
        assert max(worst[key]) <= 1.0, (key, worst[key])


@gpu
@requires_gpu
@pytest.mark.parametrize("n", _OPT_SIZES)
def test_adam_sizes(n):
    """Every size tier (vector body, tail, grid-stride), L2 variant, step 3
    on a nonzero state."""
    ext = _ext()
    p, grad = _adam_inputs(n, 94)
    m = 0.3 * grad()
    v = 0.2 * grad().square()
    g = grad()
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    ext.adam_step(p, g, m, v, 0.1, 0.9, 0.999, 1e-8, 0.01, 3, False)
    hp = _adam_hp(0.1, 0.9, 0.999, 1e-8, 0.01, 3, False)
    _adam_check("n={}".format(n), p, m, v, p0, g, m0, v0, hp)


@gpu
@requires_gpu
@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
def test_bucket_adam_wiring(decoupled):
    from tensorflowonspark_amd.ops.modules import BucketAdam
    model, engine, b = _tiny_engine()
    with torch.no_grad():
        b.param_flat.mul_(0.05)
    opt = BucketAdam(engine, lr=0.1, betas=(0.9, 0.999), eps=1e-8,
                     weight_decay=0.01, decoupled=decoupled)
    _, grad = _adam_inputs(b.param_flat.numel(), 95)
    for step in (1, 2, 3):
        b.buffer.copy_(grad())         # the bucket's flat gradient
        p0, g = b.param_flat.clone(), b.buffer.clone()
        m0, v0 = opt._m[0].clone(), opt._v[0].clone()
        opt.step()
        assert opt.step_count == step
        hp = _adam_hp(0.1, 0.9, 0.999, 1e-8, 0.01, step, decoupled)
        _adam_check("step {}".format(step), b.param_flat, opt._m[0],
                    opt._v[0], p0, g, m0, v0, hp)
        assert _params_are_views(b)


# ===========================================================================
# 5. pack_bf16 through PackPlan
# ===========================================================================

def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(view, want, what=""):
    want = want.to(BF16)
    assert view.numel() == want.numel(), what
    assert torch.equal(_bits(view).reshape(-1), _bits(want).reshape(-1)), what


def _eager(kind, w):
    """The eager transform each spec replaces (tests/test_packplan.py)."""
    if kind == "row":
        return w.reshape(w.shape[0], w.shape[1])
    if kind == "rowT":
        return w.reshape(w.shape[0], w.shape[1]).t()
    if kind == "w9":
        return w.permute(0, 2, 3, 1)
    if kind == "w9p":
        return w.flip(2, 3).permute(1, 2, 3, 0)
    if kind == "stem":
        out = w.new_zeros(w.shape[0], 7, 8, 4)
        out[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        return out
    raise KeyError(kind)


def _eager_class(w, rl, sl):
    wperm = w.flip(2, 3).permute(1, 2, 3, 0)          # [ci][r][s][co]
    return torch.stack([wperm[:, r, s, :] for r in rl for s in sl], dim=1)


def _add(plan, kind, w):
    from tensorflowonspark_amd.ops import packplan
    return {"row": packplan._gemm_row_spec, "rowT": packplan._gemm_rowT_spec,
            "w9": packplan._w9_spec, "w9p": packplan._w9p_spec,
            "stem": packplan._stem_spec}[kind](plan, w)


def _randw(*shape, seed=0):
    return torch.randn(*shape, device=_DEV, generator=_gen(100 + seed, _DEV))


def _run_plan(entries):
    """entries: (kind, weight) -> finalized, packed plan + expected tensors."""
    from tensorflowonspark_amd.ops import packplan
    plan = packplan.PackPlan(_DEV)
    want = []
    for kind, w in entries:
        i = _add(plan, kind, w)
        assert i == len(want)
        want.append(_eager(kind, w))
    plan.finalize()
    assert plan.run_if_stale() is True
    return plan, want


@gpu
@requires_gpu
def test_pack_every_spec():
    from tensorflowonspark_amd.ops import packplan
    plan = packplan.PackPlan(_DEV)
    w1 = _randw(8, 12, 1, 1, seed=1)
    w2 = _randw(6, 4, 3, 3, seed=2)
    ws = _randw(5, 3, 7, 7, seed=3)
    want = []
    for kind, w in (("row", w1), ("rowT", w1), ("w9", w2), ("w9p", w2)):
        _add(plan, kind, w)
        want.append((kind, _eager(kind, w)))
    for (ph, pw), (rl, sl) in packplan._class_taps(3, 1).items():
        packplan._w9p_class_spec(plan, w2, rl, sl)
        want.append(("class{}{}".format(ph, pw), _eager_class(w2, rl, sl)))
    _add(plan, "stem", ws)
    want.append(("stem", _eager("stem", ws)))
    plan.finalize()
    assert plan.run_if_stale() is True
    assert len(plan.views) == len(want) == 9
    assert sum(v.numel() for v in plan.views) == plan._arena.numel()
    for view, (what, ref) in zip(plan.views, want):
        assert view.dtype == BF16
        assert torch.equal(view.reshape(-1), ref.to(BF16).reshape(-1)), what
        _same_bits(view, ref, what)
    stem = plan.views[-1].reshape(5, 7, 8, 4)
    assert float(stem[:, :, 7, :].abs().max()) == 0.0
    assert float(stem[:, :, :, 3].abs().max()) == 0.0


def _bf16_edge_values():
    """fp32 bit patterns around every bf16 rounding decision."""
    pats = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x0001, 0x0000, 0x007F, 0x0080,
               0x7F7F, 0x7F00):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
            pats.append((hi << 16) | lo)
    pats = [b for b in pats if b < 0x7F800000]      # finite
    pats += [0x7F800000, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000]
    pats += [b | 0x80000000 for b in pats]          # negatives, -0, -inf
    t = torch.tensor(pats, dtype=torch.int64)
    t = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)
    return t.view(FP32)


def test_bf16_edge_values_premise_cpu():
    """The list holds +-0, +-inf, denormals, exact ties to an even and to an
    odd neighbour, and values one fp32 ulp either side of a tie."""
    v = _bf16_edge_values()
    assert not bool(torch.isnan(v).any())
    bits = v.view(torch.int32).long() & 0xFFFFFFFF
    low, odd = bits & 0xFFFF, (bits >> 16) & 1
    for want_low in (0x7FFF, 0x8000, 0x8001):
        for want_odd in (0, 1):
            assert bool(((low == want_low) & (odd == want_odd)).any())
    assert bool((bits == 0).any()) and bool((bits == 0x80000000).any())
    assert bool(torch.isinf(v).any())
    den = (v != 0) & (v.abs() < 2.0 ** -126)
    assert int(den.sum()) >= 8
    # ties go to even, as the eager cast does it
    r = v.to(BF16).view(torch.int16).long() & 0xFFFF
    tie = (low == 0x8000) & torch.isfinite(v)
    assert bool(((r[tie] & 1) == 0).all())
    assert bool((v[tie].double() != v[tie].to(BF16).double()).all())


@gpu
@requires_gpu
def test_pack_bit_patterns():
    vals = _bf16_edge_values()
    k = vals.numel()
    w = vals.repeat(6)[:5 * k].reshape(5, k).to(_DEV).contiguous()
    plan, want = _run_plan([("row", w), ("rowT", w)])
    cpu = w.cpu()
    _same_bits(plan.views[0].cpu(), cpu, "row")
    _same_bits(plan.views[1].cpu(), cpu.t(), "rowT")
    # -0 stays -0: the bit compare above would not pass on +0
    z = plan.views[0].reshape(-1)[(w.reshape(-1) == 0)]
    assert int((_bits(z) != 0).sum()) >= 1


@gpu
@requires_gpu
def test_pack_descriptor_table():
    # one descriptor
    w = _randw(7, 13, 1, 1, seed=4)
    plan, want = _run_plan([("rowT", w)])
    assert len(plan.specs) == 1
    _same_bits(plan.views[0], want[0], "ndesc=1")
    # a 1-element descriptor between two larger ones: the first and last
    # element of every descriptor sit on a ``cum`` boundary
    a, one, b = (_randw(9, 11, 1, 1, seed=5), _randw(1, 1, 1, 1, seed=6),
                 _randw(4, 5, 3, 3, seed=7))
    plan, want = _run_plan([("row", a), ("row", one), ("w9p", b)])
    assert [v.numel() for v in plan.views] == [99, 1, 180]
    for i, (v, r) in enumerate(zip(plan.views, want)):
        _same_bits(v, r, "desc {}".format(i))
        flat, ref = v.reshape(-1), r.to(BF16).reshape(-1)
        assert float(flat[0]) == float(ref[0])
        assert float(flat[-1]) == float(ref[-1])
    # 42 descriptors of assorted sizes, 1-element ones among them
    entries = []
    for i in range(14):
        co, ci = 1 + (i * 5) % 9, 1 + (i * 3) % 7
        w1 = _randw(co, ci, 1, 1, seed=10 + i)
        w2 = _randw(co, ci, 3, 3, seed=30 + i)
        entries += [("rowT", w1), ("w9", w2), ("w9p", w2)]
    plan, want = _run_plan(entries)
    assert len(plan.specs) == 42
    for i, (v, r) in enumerate(zip(plan.views, want)):
        _same_bits(v, r, "desc {}".format(i))


@gpu
@requires_gpu
def test_pack_grid_stride():
    """total just above 16384 x 256: the block cap of tfosr_pack_bf16 is
    reached and the first threads take a second element."""
    small0 = _randw(3, 5, 1, 1, seed=50)
    big = _randw(2048, 2048, 1, 1, seed=51)
    small1 = _randw(6, 4, 3, 3, seed=52)
    small2 = _randw(5, 3, 7, 7, seed=53)
    plan, want = _run_plan([("row", small0), ("row", big), ("w9p", small1),
                            ("stem", small2)])
    assert PACK_CAP_THREADS < plan._total < PACK_CAP_THREADS + 4096
    for i, (v, r) in enumerate(zip(plan.views, want)):
        _same_bits(v, r, "desc {}".format(i))


@gpu
@requires_gpu
def test_pack_staleness():
    w = torch.nn.Parameter(_randw(8, 12, 1, 1, seed=60))
    w2 = torch.nn.Parameter(_randw(6, 4, 3, 3, seed=61))
    plan, _ = _run_plan([("row", w), ("w9", w2)])
    assert plan.run_if_stale() is False
    assert plan.stale_pointers() is False
    with torch.no_grad():
        w.add_(1.0)                         # in place: version bump
    assert plan.stale_pointers() is False
    assert plan.run_if_stale() is True
    _same_bits(plan.views[0], _eager("row", w.detach()), "after update")
    _same_bits(plan.views[1], _eager("w9", w2.detach()), "untouched")
    assert plan.run_if_stale() is False
    w.data = w.data.clone()                 # storage replaced
    assert plan.stale_pointers() is True


@gpu
@requires_gpu
def test_pack_model_plan():
    """build_resnet_plan on a two-block toy (one stride-2 block with a
    downsample) plus the stem: every ``_tfos_packs`` view is its eager
    transform."""
    from tensorflowonspark_amd.models.resnet import Bottleneck, conv1x1
    from tensorflowonspark_amd.ops import packplan
    from tensorflowonspark_amd.ops.modules import FusedBN, StemConv7x7
    torch.manual_seed(13)

    def ds(cin, cout, stride):
        return torch.nn.Sequential(conv1x1(cin, cout, stride), FusedBN(cout))

    model = torch.nn.Sequential(
        StemConv7x7(3, 64),
        Bottleneck(64, 64, 1, ds(64, 256, 1)),
        Bottleneck(256, 64, 2, ds(256, 256, 2)),
    ).to(_DEV)
    blocks = [m for m in model if isinstance(m, Bottleneck)]
    assert all(b._block_fusable for b in blocks)
    plan = packplan.build_resnet_plan(model, _DEV)
    assert plan is not None and plan.run_if_stale() is True
    checked = 0
    for b in blocks:
        w1, w2, w3 = (b.conv1.weight.detach(), b.conv2.weight.detach(),
                      b.conv3.weight.detach())
        wd = b.downsample[0].weight.detach()
        want = {"w1b": _eager("row", w1), "w1bT": _eager("rowT", w1),
                "w3b": _eager("row", w3), "w3bT": _eager("rowT", w3),
                "w9": _eager("w9", w2), "wdb": _eager("row", wd),
                "wdbT": _eager("rowT", wd)}
        if b.stride == 1:
            want["w9p"] = _eager("w9p", w2)
        else:
            for (ph, pw), (rl, sl) in packplan._class_taps(3, 1).items():
                want["w9p_{}{}".format(ph, pw)] = _eager_class(w2, rl, sl)
        assert set(b._tfos_packs) == set(want)
        for k, ref in want.items():
            _same_bits(b._tfos_packs[k], ref, k)
            checked += 1
    _same_bits(model[0]._tfos_packs["w224"],
               _eager("stem", model[0].weight.detach()), "w224")
    assert checked == 8 + 11
    assert len(plan.specs) == checked + 1


# ===========================================================================
# 6. argument checks (each refused on the host, before any launch)
# ===========================================================================

def _rejects(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)
    torch.cuda.synchronize()


@gpu
@requires_gpu
def test_bindings_nhwc_pack():
    ext = _ext()
    x = torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device=_DEV)
    m = torch.zeros(3, device=_DEV)
    s = torch.ones(3, device=_DEV)
    ext.nhwc_pack(x, m, s, 1.0, False, False)
    six = torch.ones(6, device=_DEV)
    for bad in (m.cpu(), m.double(), m.half(), six[::2], six[:2], six[:4],
                torch.zeros(0, device=_DEV)):
        _rejects(ext.nhwc_pack, x, bad, s, 1.0, False, False)
        _rejects(ext.nhwc_pack, x, m, bad, 1.0, False, False)
    _rejects(ext.nhwc_pack, x.cpu(), m.cpu(), s.cpu(), 1.0, False, False)
    _rejects(ext.nhwc_pack, x.float(), m, s, 1.0, False, False)
    _rejects(ext.nhwc_pack, x[:, :, ::2], m, s, 1.0, False, False)
    _rejects(ext.nhwc_pack, x[0], m, s, 1.0, False, False)


@gpu
@requires_gpu
def test_bindings_sgd_step():
    ext = _ext()
    p, g, m = (torch.zeros(8, device=_DEV) for _ in range(3))
    ext.sgd_step(p, g, m, 0.1, 0.9, 0.0, False)
    wide = torch.zeros(16, device=_DEV)
    for bad in (wide[::2], wide[:7], wide[:9], p.cpu(), p.double(), p.bfloat16()):
        for i in range(3):
            args = [p, g, m]
            args[i] = bad
            _rejects(ext.sgd_step, *args, 0.1, 0.9, 0.0, False)
    _rejects(ext.sgd_step, p.cpu(), g.cpu(), m.cpu(), 0.1, 0.9, 0.0, False)


@gpu
@requires_gpu
def test_bindings_adam_step():
    ext = _ext()
    p, g, m, v = (torch.zeros(8, device=_DEV) for _ in range(4))
    tail = (0.1, 0.9, 0.999, 1e-8, 0.0)
    ext.adam_step(p, g, m, v, *tail, 1, False)
    wide = torch.zeros(16, device=_DEV)
    for bad in (wide[::2], wide[:7], wide[:9], p.cpu(), p.double(), p.bfloat16()):
        for i in range(4):
            args = [p, g, m, v]
            args[i] = bad
            _rejects(ext.adam_step, *args, *tail, 1, False)
    _rejects(ext.adam_step, p.cpu(), g.cpu(), m.cpu(), v.cpu(), *tail, 1, False)
    _rejects(ext.adam_step, p, g, m, v, *tail, 0, False)
    _rejects(ext.adam_step, p, g, m, v, *tail, -3, False)


@gpu
@requires_gpu
def test_bindings_maxpool_fwd():
    ext = _ext()
    x = _cl(torch.zeros(1, 8, 6, 6, device=_DEV, dtype=BF16))
    ext.maxpool_fwd(x, 3, 2, 1)
    _rejects(ext.maxpool_fwd, x.half(), 3, 2, 1)         # fp16 read as fp32
    _rejects(ext.maxpool_fwd, x.double(), 3, 2, 1)
    _rejects(ext.maxpool_fwd, x.cpu(), 3, 2, 1)
    _rejects(ext.maxpool_fwd, x.contiguous(), 3, 2, 1)   # not channels_last
    _rejects(ext.maxpool_fwd, x[0], 3, 2, 1)
    _rejects(ext.maxpool_fwd, _cl(x[:, :4]), 3, 2, 1)    # bf16 C % 8
    _rejects(ext.maxpool_fwd, _cl(x.float()[:, :6]), 3, 2, 1)  # fp32 C % 4
    _rejects(ext.maxpool_fwd, x, 0, 2, 0)                # K < 1
    _rejects(ext.maxpool_fwd, x, 3, 0, 1)                # S = 0
    _rejects(ext.maxpool_fwd, x, 3, -1, 1)
    _rejects(ext.maxpool_fwd, x, 3, 2, -1)               # P < 0
    _rejects(ext.maxpool_fwd, x, 3, 2, 2)                # P > K/2
    _rejects(ext.maxpool_fwd, x, 7, 2, 0)                # no output row
    big = _cl(torch.zeros(1, 8, 17, 17, device=_DEV, dtype=BF16))
    ext.maxpool_fwd(big, 16, 1, 8)                       # K*K = 256 fits
    _rejects(ext.maxpool_fwd, big, 17, 1, 8)             # K*K = 289


@gpu
@requires_gpu
def test_bindings_maxpool_bwd():
    ext = _ext()
    x = _cl(torch.zeros(2, 8, 7, 9, device=_DEV, dtype=BF16))
    y, idx = ext.maxpool_fwd(x, 3, 2, 1)
    dy = torch.ones_like(y)
    ext.maxpool_bwd(dy, idx, 7, 9, 3, 2, 1)
    ok = (7, 9, 3, 2, 1)
    _rejects(ext.maxpool_bwd, dy, idx.int(), *ok)
    _rejects(ext.maxpool_bwd, dy, idx.cpu(), *ok)
    _rejects(ext.maxpool_bwd, dy, idx.permute(0, 3, 1, 2), *ok)   # (N,C,OH,OW)
    _rejects(ext.maxpool_bwd, dy, idx[:1], *ok)
    _rejects(ext.maxpool_bwd, dy, idx[..., :4], *ok)
    _rejects(ext.maxpool_bwd, dy, idx.reshape(-1), *ok)
    wide = torch.zeros(2, 4, 5, 16, dtype=torch.uint8, device=_DEV)
    _rejects(ext.maxpool_bwd, dy, wide[..., ::2], *ok)            # strided
    _rejects(ext.maxpool_bwd, dy.half(), idx, *ok)
    _rejects(ext.maxpool_bwd, dy.cpu(), idx.cpu(), *ok)
    _rejects(ext.maxpool_bwd, dy[0], idx, *ok)
    _rejects(ext.maxpool_bwd, dy, idx, 9, 9, 3, 2, 1)     # OH would be 5
    _rejects(ext.maxpool_bwd, dy, idx, 7, 11, 3, 2, 1)    # OW would be 6
    _rejects(ext.maxpool_bwd, dy, idx, 7, 9, 3, 0, 1)
    _rejects(ext.maxpool_bwd, dy, idx, 7, 9, 0, 2, 0)
    _rejects(ext.maxpool_bwd, dy, idx, 7, 9, 3, 2, 2)
    _rejects(ext.maxpool_bwd, dy, idx, 7, 9, 3, 2, -1)
    _rejects(ext.maxpool_bwd, dy, idx, 7, 9, 17, 2, 8)
    # consistent geometry whose dx would need more threads than a u32 holds:
    # K = 1, S = 2^20 -> H = 3 * 2^20 + 1, W = 4 * 2^20 + 1 (refused before
    # dx is allocated)
    S = 1 << 20
    _rejects(ext.maxpool_bwd, dy, idx, 3 * S + 1, 4 * S + 1, 1, S, 0)


@gpu
@requires_gpu
def test_bindings_pack_bf16():
    ext = _ext()
    w = _randw(4, 6, 1, 1, seed=70)
    plan, want = _run_plan([("row", w), ("rowT", w)])
    d, c, a, n, t = (plan._descbuf, plan._cumbuf, plan._arena,
                     len(plan.specs), plan._total)
    assert d.numel() == 80 * n and c.numel() == n + 1 and a.numel() == t
    ext.pack_bf16(d, c, n, a, t)
    before = a.clone()
    ext.pack_bf16(d, c, n, a, 0)              # nothing to do, no launch
    ext.pack_bf16(d[:0], c[:1], 0, a, 0)
    assert torch.equal(_bits(a), _bits(before))
    _rejects(ext.pack_bf16, d[:0], c[:1], 0, a, t)       # ndesc 0, total > 0
    _rejects(ext.pack_bf16, d, c, n + 1, a, t)
    _rejects(ext.pack_bf16, d, c, n - 1, a, t)
    _rejects(ext.pack_bf16, d, c, -1, a, t)
    _rejects(ext.pack_bf16, d[:-1], c, n, a, t)
    _rejects(ext.pack_bf16, d.view(torch.int16), c, n, a, t)
    _rejects(ext.pack_bf16, d, c[:-1], n, a, t)
    _rejects(ext.pack_bf16, d, c.int(), n, a, t)
    _rejects(ext.pack_bf16, d, c, n, a[:-1], t)
    _rejects(ext.pack_bf16, d, c, n, a, t + 1)
    _rejects(ext.pack_bf16, d, c, n, a, -1)
    _rejects(ext.pack_bf16, d, c, n, a.float(), t)
    _rejects(ext.pack_bf16, d.cpu(), c, n, a, t)
    _rejects(ext.pack_bf16, d, c.cpu(), n, a, t)
    _rejects(ext.pack_bf16, d, c, n, a.cpu(), t)
    wide = torch.zeros(2 * t, dtype=BF16, device=_DEV)
    _rejects(ext.pack_bf16, d, c, n, wide[::2], t)
