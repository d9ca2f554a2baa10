"""MFMA GEMM, implicit-GEMM conv and wrw kernels vs plain fp64 arithmetic.

Every dispatch tier of ``csrc/gemm_mfma.hip``, ``csrc/conv3x3_mfma.hip`` and
``csrc/conv_wrw2.hip`` is driven directly through the extension entry points
and compared with an fp64 reference computed from exactly the bf16 values the
kernel sees.  Convolution references are an explicit zero-dilation + unfold +
fp64 matmul (``_conv_ref`` / ``_wrw_ref``); a CPU test pins those helpers to
``F.conv2d`` / ``F.conv_transpose2d`` in fp64.

Exact probes (the main instrument).  Inputs are integers in [-3, 3] stored in
bf16 (conv activations leave 0 out so that padding is visible), re-seeded per
case.  Every product is an integer and ``sum |a||b| <= 9 * 4100 < 2^24`` for
every output, so every partial sum in every order is exact in fp32 and no
tolerance is needed:

    fp32 outputs   == ref64.float()              bit for bit
    bf16 outputs   == ref64.float().bfloat16()   bit for bit (RNE)

Accumulating entry points start from an integer-valued bf16 ``old`` in
[-300, 300] and are pinned to the rounding model of their tier:

    conv_mfma_acc, conv_par(accum), gemm_bt_acc 256^2 tier
                                     bf16(old + S)
    gemm_bt_acc 128^2 and 256x64 tiers (accumulator staged through LDS as
    bf16, then added to the old value)
                                     bf16(float(bf16(S)) + old)

The two models differ only where |S| > 256 (S no longer a bf16 integer); each
tier has a case with such accumulators and the test asserts that the two
expectations differ there.  ``test_exact_probe_premise_cpu`` checks the
premise without a GPU: the abs-sum stays below 2^24 and the fp32 CPU result
equals the fp64 one bit for bit, for every exact case.

Real-valued probes (one or two per tier) catch precision loss integers cannot
show.  Inputs are randn/4 with a distinct scale per row / channel, rounded to
bf16.  The bound comes from the arithmetic alone and was fixed before the
first GPU run:

    |got - ref64| <= K * 2^-23 * (|A| |B|^T)_ij + half_ulp(out dtype, ref64)

K is the contraction length (taps * channels; for wrw the pixel count that
the split-M slices share).  Products of bf16 values are exact in fp32; the
first term is the standard any-order bound on fp32 accumulation error with
the unit roundoff doubled, so it holds whether the MFMA accumulator rounds or
truncates.  The two-rounding GEMM tiers get one more bf16 half-ulp (at S), and
every accumulating path 2^-24 |ref64| for the fp32 add of the old value.
"""

import functools
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

BF16 = torch.bfloat16
FP32 = torch.float32
FP64 = torch.float64
EXACT_LIMIT = 2 ** 24
OLD_MAX = 300          # |old| of the accumulating probes


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(gen, *shape, nonzero=False):
    """Integers in [-3, 3] (without 0 when ``nonzero``) as bf16."""
    if nonzero:
        mag = torch.randint(1, 4, shape, generator=gen)
        sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
        return (mag * sign).to(BF16)
    return torch.randint(-3, 4, shape, generator=gen).to(BF16)


def _old_ints(gen, *shape):
    """Integer-valued bf16 in [-300, 300] (above 256 bf16 keeps even ones)."""
    return torch.randint(-OLD_MAX, OLD_MAX + 1, shape, generator=gen).to(BF16)


def _scales(gen, n):
    """n distinct scales spread over [0.5, 2], shuffled."""
    frac = torch.randperm(n, generator=gen).double() / max(n - 1, 1)
    return (0.5 + 1.5 * frac).float()


def _real(gen, rows, *rest):
    """randn/4 with a distinct scale per leading index, rounded to bf16."""
    v = torch.randn(rows, *rest, generator=gen) / 4
    s = _scales(gen, rows).view(rows, *([1] * len(rest)))
    return (v * s).to(BF16)


def _half_ulp(ref64, dtype):
    """Half an ulp of ``dtype`` at |ref64|."""
    if dtype == BF16:
        # |ref| = m * 2^e with m in [0.5, 1): a bf16 ulp there is 2^(e-8)
        _, e = torch.frexp(ref64)
        half = torch.ldexp(torch.ones_like(ref64), e - 9)
        return torch.where(ref64 == 0, torch.zeros_like(ref64), half)
    return 2.0 ** -24 * ref64.abs()


def _to_bf16(ref64):
    return ref64.float().bfloat16()


def _assert_bits(what, got, exp):
    """got (device) and exp (CPU) hold the same bits."""
    got = got.detach().cpu().contiguous()
    exp = exp.contiguous()
    assert got.dtype == exp.dtype, "{}: dtype {} vs {}".format(
        what, got.dtype, exp.dtype)
    assert got.shape == exp.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(exp.shape))
    iv = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.view(iv) != exp.view(iv)
    nbad = int(bad.sum())
    if nbad:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(
            "{}: {} of {} elements differ; first at {}: got {} expected {}"
            .format(what, nbad, bad.numel(), idx, float(got[idx]),
                    float(exp[idx])))


def _assert_bound(what, got, ref64, absprod, K, out_dtype, extra=None):
    """|got - ref64| <= K 2^-23 absprod + half_ulp(out dtype) (+ extra)."""
    got = got.detach().double().cpu()
    ref64, absprod = ref64.cpu(), absprod.cpu()
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), "{}: non-finite values".format(what)
    tol = K * 2.0 ** -23 * absprod + _half_ulp(ref64, out_dtype)
    if extra is not None:
        tol = tol + extra.cpu()
    err = (got - ref64).abs()
    worst = (err - tol).argmax()
    print("  {:<22s} K {:<6d} err max {:.3e}  worst err/bound {:.3e}/{:.3e}"
          .format(what, K, err.max().item(), err.reshape(-1)[worst].item(),
                  tol.reshape(-1)[worst].item()))
    nbad = int((err > tol).sum())
    assert nbad == 0, "{}: {} of {} elements beyond the bound".format(
        what, nbad, err.numel())


# ---------------------------------------------------------------------------
# references: zero-dilation + unfold + matmul in the dtype of the arguments
# ---------------------------------------------------------------------------

def _dilate(x, D):
    if D == 1:
        return x
    N, C, H, W = x.shape
    xd = x.new_zeros(N, C, (H - 1) * D + 1, (W - 1) * D + 1)
    xd[:, :, ::D, ::D] = x
    return xd


def _natural(size, k, S, P, D=1):
    return ((size - 1) * D + 1 + 2 * P - k) // S + 1


def _conv_ref(x, wk, fh, fw, S, P, D, OH, OW, pad_value=0.0):
    """out[n,co,oh,ow] = sum wk[co][r][s][ci] * xv[n,ci,oh*S-P+r,ow*S-P+s]

    xv is x zero-dilated by D and ``pad_value`` outside; wk is
    [Cout, fh*fw*Cin] in the kernels' [Cout][r][s][Cin] order.  OH/OW may
    exceed the natural output size (the extra rows read beyond the image)."""
    N, Cin = x.shape[0], x.shape[1]
    Cout = wk.shape[0]
    xv = _dilate(x, D)
    HV, WV = xv.shape[2], xv.shape[3]
    pb = max(0, (OH - 1) * S + fh - P - HV)
    pr = max(0, (OW - 1) * S + fw - P - WV)
    xp = F.pad(xv, (P, pr, P, pb), value=pad_value)
    oh_n = (xp.shape[2] - fh) // S + 1
    ow_n = (xp.shape[3] - fw) // S + 1
    cols = F.unfold(xp, (fh, fw), stride=S)          # [N, Cin*fh*fw, L]
    w2 = wk.reshape(Cout, fh, fw, Cin).permute(0, 3, 1, 2) \
        .reshape(Cout, Cin * fh * fw)
    y = torch.matmul(w2, cols).reshape(N, Cout, oh_n, ow_n)
    return y[:, :, :OH, :OW]


def _wrw_ref(dy, x, R, Sf, stride, P):
    """dW[co][(r,s,ci)] = sum_m dy[m][co] * xpad[tap(m,r,s)][ci]"""
    N, Cin = x.shape[0], x.shape[1]
    Cout = dy.shape[1]
    cols = F.unfold(x, (R, Sf), padding=P, stride=stride)  # [N, Cin*R*Sf, L]
    L = cols.shape[2]
    assert L == dy.shape[2] * dy.shape[3]
    dw = torch.matmul(dy.reshape(N, Cout, L), cols.transpose(1, 2)).sum(0)
    return dw.reshape(Cout, Cin, R, Sf).permute(0, 2, 3, 1) \
        .reshape(Cout, R * Sf * Cin)


def _convT_ref(x, w, padding, output_padding):
    """ConvTranspose2d stride 2, w [Cin, Cout, k, k]: a stride-1 conv of the
    zero-dilated input with the flipped, channel-swapped weight."""
    k = w.shape[2]
    H, W = x.shape[2], x.shape[3]
    OH = (H - 1) * 2 - 2 * padding + k + output_padding
    OW = (W - 1) * 2 - 2 * padding + k + output_padding
    wperm = w.flip(2, 3).permute(1, 2, 3, 0)             # [Cout, k, k, Cin]
    return _conv_ref(x, wperm.reshape(wperm.shape[0], -1), k, k, 1,
                     k - 1 - padding, 2, OH, OW)


def _w4_to_wk(w4):
    """Conv2d weight [Cout, Cin, fh, fw] -> kernel layout [Cout, fh*fw*Cin]."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1)


# ---------------------------------------------------------------------------
# dispatch rules recomputed in Python (landing conditions)
# ---------------------------------------------------------------------------

T128, SKINNY, T256 = "t128", "skinny", "t256"


def _gemm_tier(M, N, K):
    """tfosr_gemm_bt_acc's dispatch -> (tier, workgroups)."""
    cdiv = lambda a, b: (a + b - 1) // b
    if M >= 1024 and N >= 192 and K >= 1024:
        return T256, cdiv(M, 256) * cdiv(N, 256)
    if N % 128 != 0 and (N % 64 == 0 or N <= 64):
        return SKINNY, cdiv(M, 256) * cdiv(N, 64)
    return T128, cdiv(M, 128) * cdiv(N, 128)


def _conv_tier(M, Cout):
    """launch_conv / tfosr_conv_par dispatch -> (tier, workgroups)."""
    cdiv = lambda a, b: (a + b - 1) // b
    if Cout >= 192:
        return T256, cdiv(M, 256) * cdiv(Cout, 256)
    return T128, cdiv(M, 256) * cdiv(Cout, 128)


def _wrw2_split(Cout, Cin, M):
    """tfosr_wrw2_split."""
    ntiles = ((Cout + 63) // 64) * ((Cin + 63) // 64)
    split = max(1, 1024 // ntiles)
    steps = (M + 31) // 32
    while split * 8 > steps and split > 1:
        split //= 2
    return split


def _wrw2_empty_slices(taps, split, M):
    """Split-M slices of tfosr_conv_wrw2 that receive no K-step."""
    px = 64 if taps == 1 else 32
    steps = (M + px - 1) // px
    spw = (steps + split - 1) // split
    return sum(1 for sp in range(split) if sp * spw * px >= M)


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------

# (tier, M, N, K, what); "big" cases have |S| > 256 so the one- and
# two-rounding models of gemm_bt_acc differ
GEMM_EXACT = [
    (T128, 128, 128, 32, "nkt1"),
    (T128, 128, 128, 64, "nkt2"),
    (T128, 130, 256, 96, "raggedM-4wg"),
    (T128, 300, 200, 64, "raggedN-6wg"),
    (T128, 70, 99, 64, "oddN-unaligned-rows"),
    (T128, 1, 128, 32, "M1"),
    (T128, 128, 128, 2048, "big"),
    (SKINNY, 256, 64, 32, "nkt1"),
    (SKINNY, 257, 192, 64, "ntn3"),
    (SKINNY, 50, 40, 32, "N40"),
    (SKINNY, 9, 1, 32, "N1"),
    (SKINNY, 256, 64, 2048, "big"),
    (T256, 1024, 192, 1024, "raggedN-big"),
    (T256, 1030, 264, 1056, "ragged-nkt33-10wg-big"),
]


def _gemm_id(c):
    return "{}-{}x{}x{}-{}".format(*c)


def _conv_case(name, N, Cin, H, W, Cout, fh, fw, S, P, D=1, OH=None, OW=None):
    if OH is None:
        OH, OW = _natural(H, fh, S, P, D), _natural(W, fw, S, P, D)
    return dict(name=name, N=N, Cin=Cin, H=H, W=W, Cout=Cout, fh=fh, fw=fw,
                S=S, P=P, D=D, OH=OH, OW=OW)


# name = <tile tier>-<filter>-...; nkt = fh*fw*Cin/32
CONV_EXACT = [
    _conv_case("t128-1x1-nkt1-c32-m25", 1, 32, 5, 5, 32, 1, 1, 1, 0),
    _conv_case("t128-1x1-nkt2-c72-m297", 3, 64, 9, 11, 72, 1, 1, 1, 0),
    _conv_case("t128-1x1-nkt3-c72-s2", 3, 96, 9, 11, 72, 1, 1, 2, 0),
    _conv_case("t128-1x1-nkt4-c32-m25", 1, 128, 5, 5, 32, 1, 1, 1, 0),
    _conv_case("t256-1x1-nkt1-c192-m25", 1, 32, 5, 5, 192, 1, 1, 1, 0),
    _conv_case("t256-1x1-nkt2-c200-m297", 3, 64, 9, 11, 200, 1, 1, 1, 0),
    _conv_case("t256-1x1-nkt3-c264-m297", 3, 96, 9, 11, 264, 1, 1, 1, 0),
    _conv_case("t256-1x1-nkt4-c200-s2", 3, 128, 9, 11, 200, 1, 1, 2, 0),
    _conv_case("t128-3x3-nkt9-p1-c72-m297", 3, 32, 9, 11, 72, 3, 3, 1, 1),
    _conv_case("t256-3x3-p1-c264-m1083-10wg", 3, 32, 19, 19, 264, 3, 3, 1, 1),
    _conv_case("t128-3x3-s2-p1-c32", 3, 32, 9, 11, 32, 3, 3, 2, 1),
    _conv_case("t256-3x3-s2-p0-c200", 3, 32, 9, 11, 200, 3, 3, 2, 0),
    _conv_case("t128-4x4-s2-p1-c72", 3, 32, 9, 11, 72, 4, 4, 2, 1),
    _conv_case("t256-2x3-p1-c192", 1, 32, 5, 5, 192, 2, 3, 1, 1),
    _conv_case("t128-2x3-s2-p1-c72", 3, 32, 9, 11, 72, 2, 3, 2, 1),
    # D=2: the stride-2 dgrad / transposed-conv formulation.  The first one
    # asks for an output one row and column larger than the natural size, as
    # the Conv3x3 stride-2 dgrad of an even-sized input does.
    _conv_case("t128-3x3-d2-p1-c72-explicit", 3, 32, 5, 6, 72, 3, 3, 1, 1,
               D=2, OH=10, OW=12),
    _conv_case("t256-4x4-d2-p2-c200", 3, 32, 5, 6, 200, 4, 4, 1, 2, D=2),
    _conv_case("t128-4x4-d2-p2-c32-2wgm", 3, 64, 5, 6, 32, 4, 4, 1, 2, D=2),
]

# parity-decomposed launches: x [N,KC,h,w] stored input, out [N,OC,OH,OW];
# k, pp as _conv_parity takes them
PAR_EXACT = [
    # Conv3x3 stride-2 dgrad: odd x even output, class sizes 5x4/5x4/4x4/4x4
    dict(name="t128-k3-pp1-9x8", N=2, KC=32, h=5, w=4, OC=72, k=3, pp=1,
         OH=9, OW=8, accum=False),
    # ConvTranspose2d k4 p1
    dict(name="t256-k4-pp2-10x6", N=2, KC=32, h=5, w=3, OC=200, k=4, pp=2,
         OH=10, OW=6, accum=False),
    # ConvTranspose2d k3 p1 output_padding 1: last row/col beyond the natural
    dict(name="t128-k3-pp1-op1-10x8", N=2, KC=64, h=5, w=4, OC=32, k=3,
         pp=1, OH=10, OW=8, accum=False),
    # bottleneck downsample dgrad: only the even-even class has a tap
    dict(name="t256-k1-pp0-acc-7x6", N=2, KC=64, h=4, w=3, OC=264, k=1, pp=0,
         OH=7, OW=6, accum=True),
    dict(name="t256-k3-pp1-acc-9x7", N=2, KC=32, h=5, w=4, OC=200, k=3, pp=1,
         OH=9, OW=7, accum=True),
]

# (name, N, Cin, H, W, Cout, k, stride, P, split, empty slices expected)
WRW_EXACT = [
    ("taps9-2x64x8x8-64-split1", 2, 64, 8, 8, 64, 3, 1, 1, 1, False),
    ("taps9-3x72x13x9-88-ragged", 3, 72, 13, 9, 88, 3, 1, 1, 1, False),
    ("taps9-2x64x9x9-64-s2", 2, 64, 9, 9, 64, 3, 2, 1, 1, False),
    ("taps1-2x128x8x8-128", 2, 128, 8, 8, 128, 1, 1, 0, 1, False),
    ("taps1-1x136x7x5-72-m35", 1, 136, 7, 5, 72, 1, 1, 0, 1, False),
    ("taps1-2x64x9x9-128-s2", 2, 64, 9, 9, 128, 1, 2, 0, 1, False),
    ("taps9-1x64x50x82-64-emptyslice", 1, 64, 50, 82, 64, 3, 1, 1, 16, True),
    ("taps1-1x64x50x82-64-emptyslice", 1, 64, 50, 82, 64, 1, 1, 0, 16, True),
]

STEM = dict(N=2, H=32, W=32, Cout=64)


def _par_as_conv(c):
    return _conv_case(c["name"], c["N"], c["KC"], c["h"], c["w"], c["OC"],
                      c["k"], c["k"], 1, c["pp"], D=2, OH=c["OH"], OW=c["OW"])


@functools.lru_cache(maxsize=None)
def _gemm_inputs(key, M, N, K, real=False):
    g = _gen("gemm-" + key)
    if real:
        return _real(g, M, K), _real(g, N, K), _real(g, M, N)
    return _ints(g, M, K), _ints(g, N, K), _old_ints(g, M, N)


def _gemm_contract(a, b, dt):
    return a.to(dt) @ b.to(dt).t()


@functools.lru_cache(maxsize=None)
def _gemm_ref(key, M, N, K, real=False):
    """(S64, |A||B|^T) on the CPU; computed once per case, read-only."""
    a, b, _ = _gemm_inputs(key, M, N, K, real)
    return _gemm_contract(a, b, FP64), _gemm_contract(a.abs(), b.abs(), FP64)


@functools.lru_cache(maxsize=None)
def _conv_inputs(name, N, Cin, H, W, Cout, fh, fw, OH, OW, real=False):
    g = _gen("conv-" + name)
    if real:
        x = _real(g, Cin, N, H, W).permute(1, 0, 2, 3).contiguous()
        return x, _real(g, Cout, fh * fw * Cin), _real(g, Cout, N, OH, OW) \
            .permute(1, 0, 2, 3).contiguous()
    return (_ints(g, N, Cin, H, W, nonzero=True),
            _ints(g, Cout, fh * fw * Cin), _old_ints(g, N, Cout, OH, OW))


def _conv_args(c, real=False):
    return _conv_inputs(c["name"], c["N"], c["Cin"], c["H"], c["W"],
                        c["Cout"], c["fh"], c["fw"], c["OH"], c["OW"], real)


def _conv_contract(c, x, wk, dt, pad_value=0.0):
    return _conv_ref(x.to(dt), wk.to(dt), c["fh"], c["fw"], c["S"], c["P"],
                     c["D"], c["OH"], c["OW"], pad_value)


_conv_ref_cache = {}


def _conv_refs(c, real=False):
    """(S64, abs-sum) on the CPU; computed once per case, read-only."""
    key = (c["name"], real)
    if key not in _conv_ref_cache:
        x, wk, _ = _conv_args(c, real)
        _conv_ref_cache[key] = (_conv_contract(c, x, wk, FP64),
                                _conv_contract(c, x.abs(), wk.abs(), FP64))
    return _conv_ref_cache[key]


@functools.lru_cache(maxsize=None)
def _wrw_inputs(name, N, Cin, H, W, Cout, k, stride, P, real=False):
    g = _gen("wrw-" + name)
    OH, OW = _natural(H, k, stride, P), _natural(W, k, stride, P)
    if real:
        x = _real(g, Cin, N, H, W).permute(1, 0, 2, 3).contiguous()
        dy = _real(g, Cout, N, OH, OW).permute(1, 0, 2, 3).contiguous()
        return x, dy
    return _ints(g, N, Cin, H, W, nonzero=True), _ints(g, N, Cout, OH, OW)


@functools.lru_cache(maxsize=None)
def _wrw_refs(name, N, Cin, H, W, Cout, k, stride, P, real=False):
    x, dy = _wrw_inputs(name, N, Cin, H, W, Cout, k, stride, P, real)
    return (_wrw_ref(dy.double(), x.double(), k, k, stride, P),
            _wrw_ref(dy.double().abs(), x.double().abs(), k, k, stride, P))


@functools.lru_cache(maxsize=None)
def _stem_inputs():
    g = _gen("stem")
    N, H, W, Cout = STEM["N"], STEM["H"], STEM["W"], STEM["Cout"]
    OH, OW = _natural(H, 7, 2, 3), _natural(W, 7, 2, 3)
    return (_ints(g, N, 3, H, W, nonzero=True), _ints(g, Cout, 3, 7, 7),
            _ints(g, N, Cout, OH, OW))


def _stem_contract(dt, absval=False):
    """(y, dw[Cout,3,7,7]) of the stem in dtype dt."""
    x, w, dy = (t.abs() if absval else t for t in _stem_inputs())
    x, w, dy = x.to(dt), w.to(dt), dy.to(dt)
    y = _conv_ref(x, _w4_to_wk(w), 7, 7, 2, 3, 1, dy.shape[2], dy.shape[3])
    dw = _wrw_ref(dy, x, 7, 7, 2, 3).reshape(w.shape[0], 7, 7, 3) \
        .permute(0, 3, 1, 2)
    return y, dw


# ---------------------------------------------------------------------------
# CPU: the premise of the exact probes, and the reference helpers themselves
# ---------------------------------------------------------------------------

def _exact_contractions():
    """(name, fn(dtype, absval) -> contraction) for every exact case."""
    out = []
    for c in GEMM_EXACT + [(T128, 70, 99, 40, "Kpad"),
                           (T128, 70, 99, 64, "gemm_bf16")]:
        key = _gemm_id(c)
        a, b, _ = _gemm_inputs(key, c[1], c[2], c[3])
        out.append(("gemm-" + key, lambda dt, av, a=a, b=b: _gemm_contract(
            a.abs() if av else a, b.abs() if av else b, dt)))
    for c in CONV_EXACT + [_par_as_conv(p) for p in PAR_EXACT]:
        x, wk, _ = _conv_args(c)
        out.append(("conv-" + c["name"], lambda dt, av, c=c, x=x, wk=wk:
                    _conv_contract(c, x.abs() if av else x,
                                   wk.abs() if av else wk, dt)))
    for c in WRW_EXACT:
        x, dy = _wrw_inputs(*c[:9])
        out.append(("wrw-" + c[0], lambda dt, av, c=c, x=x, dy=dy: _wrw_ref(
            (dy.abs() if av else dy).to(dt), (x.abs() if av else x).to(dt),
            c[6], c[6], c[7], c[8])))
    out.append(("stem-fwd", lambda dt, av: _stem_contract(dt, av)[0]))
    out.append(("stem-wrw", lambda dt, av: _stem_contract(dt, av)[1]))
    return out


def test_exact_probe_premise_cpu():
    """For every exact case: sum |a||b| (+ |old|) < 2^24, so each partial sum
    in any order is exact in fp32 — and the fp32 CPU result does equal the
    fp64 reference bit for bit."""
    for name, fn in _exact_contractions():
        s64 = fn(FP64, False)
        abs_sum = fn(FP64, True)
        assert abs_sum.max().item() + OLD_MAX < EXACT_LIMIT, name
        assert (s64.abs() <= abs_sum).all(), name
        s32 = fn(FP32, False)
        assert s32.dtype == FP32 and s64.dtype == FP64, name
        assert torch.equal(s32.contiguous().view(torch.int32),
                           s64.float().contiguous().view(torch.int32)), name
        assert torch.equal(s32.double(), s64), name


def test_reference_helpers_match_library_cpu():
    """_conv_ref / _wrw_ref / _convT_ref against F.conv2d, its weight
    gradient and F.conv_transpose2d in fp64 on integer inputs (exact)."""
    g = _gen("helpers")
    for (fh, fw, S, P) in [(1, 1, 1, 0), (3, 3, 1, 1), (3, 3, 2, 1),
                           (4, 4, 2, 1), (2, 3, 1, 1), (7, 7, 2, 3)]:
        x = _ints(g, 2, 3, 9, 11).double()
        w4 = _ints(g, 5, 3, fh, fw).double().requires_grad_(True)
        y = F.conv2d(x, w4, stride=S, padding=P)
        got = _conv_ref(x, _w4_to_wk(w4.detach()), fh, fw, S, P, 1,
                        y.shape[2], y.shape[3])
        assert torch.equal(got, y.detach())
        dy = _ints(g, *y.shape).double()
        y.backward(dy)
        if fh == fw:
            assert torch.equal(_wrw_ref(dy, x, fh, fw, S, P),
                               _w4_to_wk(w4.grad))
    for (k, p, op) in [(4, 1, 0), (3, 1, 1), (3, 1, 0)]:
        x = _ints(g, 2, 3, 5, 4).double()
        w = _ints(g, 3, 6, k, k).double()
        y = F.conv_transpose2d(x, w, stride=2, padding=p, output_padding=op)
        assert torch.equal(_convT_ref(x, w, p, op), y)
    # zero-dilated conv (the D=2 / conv_par formulation) larger than natural
    x = _ints(g, 1, 2, 3, 3).double()
    wk = _ints(g, 4, 3 * 3 * 2).double()
    w4 = wk.reshape(4, 3, 3, 2).permute(0, 3, 1, 2)
    xd = F.pad(_dilate(x, 2), (0, 1, 0, 1))
    assert torch.equal(_conv_ref(x, wk, 3, 3, 1, 1, 2, 6, 6),
                       F.conv2d(xd, w4, padding=1))


def test_landing_conditions_cpu():
    """Each case lands in the tier its id names (dispatch rules recomputed
    from the launchers)."""
    for c in GEMM_EXACT:
        tier, nwg = _gemm_tier(c[1], c[2], c[3])
        assert tier == c[0], _gemm_id(c)
        if "wg" in c[4]:
            want = int(c[4].split("wg")[0].split("-")[-1])
            assert nwg == want, _gemm_id(c)
    assert _gemm_tier(1030, 264, 1056)[1] % 8 != 0
    seen = set()
    for c in CONV_EXACT + [_par_as_conv(p) for p in PAR_EXACT]:
        M = c["N"] * c["OH"] * c["OW"]
        tier, nwg = _conv_tier(M, c["Cout"])
        assert c["name"].startswith(tier), c["name"]
        assert c["Cin"] % 32 == 0
        seen.add((tier, min(c["fh"] * c["fw"] * c["Cin"] // 32, 4)))
        if "10wg" in c["name"]:
            assert nwg == 10
    # prologue depths nkt = 1, 2, 3 and >= 4 in both tile shapes
    assert seen == {(t, n) for t in (T128, T256) for n in (1, 2, 3, 4)}
    for c in WRW_EXACT:
        name, N, Cin, H, W, Cout, k, stride, P, split, empty = c
        M = N * _natural(H, k, stride, P) * _natural(W, k, stride, P)
        assert _wrw2_split(Cout, Cin, M) == split, name
        assert (_wrw2_empty_slices(k * k, split, M) > 0) == empty, name
    assert _wrw2_empty_slices(9, 16, 4100) == 1
    assert _wrw2_empty_slices(1, 16, 4100) == 3


# ---------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------

def _gemm_expect_acc(tier, S64, old):
    one = _to_bf16(old.double() + S64)
    two = _to_bf16(_to_bf16(S64).double() + old.double())
    return (one, two) if tier == T256 else (two, one)


def _run_gemm(mode, a, b, old):
    ext = _ext()
    a, b = a.cuda(), b.cuda()
    if mode == "f32":
        return ext.gemm_bt(a, b, False)
    if mode == "bf16":
        return ext.gemm_bt(a, b, True)
    c = old.cuda().clone()
    out = ext.gemm_bt_acc(a, b, c)
    assert out.data_ptr() == c.data_ptr()
    return c


@gpu
@requires_gpu
@pytest.mark.parametrize("mode", ["f32", "bf16", "acc"])
@pytest.mark.parametrize("case", GEMM_EXACT, ids=_gemm_id)
def test_gemm_exact(case, mode):
    """gemm_bt (fp32 / bf16 out) and gemm_bt_acc, bit-exact per tier."""
    tier, M, N, K, what = case
    assert _gemm_tier(M, N, K)[0] == tier
    assert os.environ.get("TFOS_GEMM256") != "off"
    key = _gemm_id(case)
    a, b, old = _gemm_inputs(key, M, N, K)
    S64, _ = _gemm_ref(key, M, N, K)
    got = _run_gemm(mode, a, b, old)
    if mode == "f32":
        _assert_bits("gemm_bt fp32", got, S64.float())
    elif mode == "bf16":
        _assert_bits("gemm_bt bf16", got, _to_bf16(S64))
    else:
        exp, other = _gemm_expect_acc(tier, S64, old)
        if "big" in what:
            assert S64.abs().max() > 256 and not torch.equal(exp, other), \
                "case cannot tell the two rounding models apart"
        _assert_bits("gemm_bt_acc " + tier, got, exp)


@gpu
@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True], ids=["f32", "bf16"])
def test_gemm_bt_k_padding_exact(out_bf16):
    """K = 40 is zero-padded to 64 by the binding."""
    M, N, K = 70, 99, 40
    key = _gemm_id((T128, M, N, K, "Kpad"))
    a, b, _ = _gemm_inputs(key, M, N, K)
    S64, _ = _gemm_ref(key, M, N, K)
    got = _ext().gemm_bt(a.cuda(), b.cuda(), out_bf16)
    _assert_bits("gemm_bt Kpad", got,
                 _to_bf16(S64) if out_bf16 else S64.float())


@gpu
@requires_gpu
def test_gemm_bf16_exact():
    """gemm_bf16: A[M,K] @ B[K,N], fp32 out (module-level wrapper too)."""
    from tensorflowonspark_amd.ops.modules import gemm_bf16
    M, N, K = 70, 99, 64
    key = _gemm_id((T128, M, N, K, "gemm_bf16"))
    a, b, _ = _gemm_inputs(key, M, N, K)
    S64, _ = _gemm_ref(key, M, N, K)
    bt = b.t().contiguous().cuda()                       # [K, N]
    _assert_bits("ext.gemm_bf16", _ext().gemm_bf16(a.cuda(), bt), S64.float())
    _assert_bits("gemm_bf16", gemm_bf16(a.cuda(), b.cuda().t()), S64.float())


@gpu
@requires_gpu
def test_gemm_bt_acc_unaligned_rows_exact():
    """N % 8 == 0 takes the 16 B vector read-modify-write for every chunk; a
    contiguous c that starts 8 bytes into its storage makes every row of it
    16 B-unaligned (the 128^2 tile, 6 workgroups)."""
    tier, M, N, K, what = GEMM_EXACT[3]
    assert N % 8 == 0 and _gemm_tier(M, N, K)[0] == T128
    key = _gemm_id(GEMM_EXACT[3])
    a, b, old = _gemm_inputs(key, M, N, K)
    S64, _ = _gemm_ref(key, M, N, K)
    buf = torch.full((M * N + 8,), 5.0, dtype=BF16, device="cuda")
    c = buf[4:4 + M * N].view(M, N)
    c.copy_(old)
    assert c.is_contiguous() and c.data_ptr() % 16 == 8
    _ext().gemm_bt_acc(a.cuda(), b.cuda(), c)
    _assert_bits("gemm_bt_acc unaligned c", c,
                 _gemm_expect_acc(tier, S64, old)[0])
    assert (buf[:4] == 5).all() and (buf[4 + M * N:] == 5).all()


GEMM_REAL = [(T128, 300, 200, 256), (SKINNY, 257, 192, 256),
             (T256, 1030, 264, 1056)]


@gpu
@requires_gpu
@pytest.mark.parametrize("mode", ["f32", "bf16", "acc"])
@pytest.mark.parametrize("case", GEMM_REAL,
                         ids=lambda c: "{}-{}x{}x{}".format(*c))
def test_gemm_real(case, mode):
    """Real-valued inputs, derived bound (module docstring)."""
    tier, M, N, K = case
    assert _gemm_tier(M, N, K)[0] == tier
    key = "real-{}x{}x{}".format(M, N, K)
    a, b, old = _gemm_inputs(key, M, N, K, True)
    S64, absprod = _gemm_ref(key, M, N, K, True)
    got = _run_gemm(mode, a, b, old)
    if mode == "acc":
        ref = old.double() + S64
        extra = 2.0 ** -24 * ref.abs()
        if tier != T256:
            extra = extra + _half_ulp(S64, BF16)
        _assert_bound("gemm_bt_acc " + tier, got, ref, absprod, K, BF16, extra)
    else:
        _assert_bound("gemm_bt " + mode, got, S64, absprod, K,
                      BF16 if mode == "bf16" else FP32)


@gpu
@requires_gpu
def test_gemm_bt_acc_rejects_bad_arguments():
    """gemm_bt_acc is bf16-only: an fp32 c used to be overwritten silently."""
    ext = _ext()
    a = torch.ones(64, 32, device="cuda", dtype=BF16)
    b = torch.ones(64, 32, device="cuda", dtype=BF16)
    c = torch.ones(64, 64, device="cuda", dtype=BF16)
    ext.gemm_bt_acc(a, b, c)
    torch.cuda.synchronize()
    assert torch.equal(c.cpu(), torch.full((64, 64), 33.0, dtype=BF16))
    for bad_c in (c.float(), c.cpu(), c.half(), c.view(1, 64, 64), c[:, :32],
                  c.t()):
        with pytest.raises(RuntimeError):
            ext.gemm_bt_acc(a, b, bad_c)
    for bad_a in (a.cpu(), a.float(), a.view(1, 64, 32), a[:, :16]):
        with pytest.raises(RuntimeError):
            ext.gemm_bt_acc(bad_a, b, c)
    with pytest.raises(RuntimeError):
        ext.gemm_bt_acc(a, b.view(2, 32, 32), c)
    with pytest.raises(RuntimeError):
        ext.gemm_bt_acc(a, b.cpu(), c)


# ---------------------------------------------------------------------------
# implicit-GEMM conv
# ---------------------------------------------------------------------------

def _assert_padding_visible(c, x, wk, S64):
    """With P > 0 the first output row and column read padding, and their
    reference changes when the padding holds 1 instead of 0."""
    if c["P"] == 0:
        return
    assert (x != 0).all()
    alt = _conv_contract(c, x, wk, FP64, pad_value=1.0)
    assert (alt[:, :, 0, :] != S64[:, :, 0, :]).any()
    assert (alt[:, :, :, 0] != S64[:, :, :, 0]).any()
    assert (alt[:, :, -1, :] != S64[:, :, -1, :]).any() or \
        (c["OH"] - 1) * c["S"] - c["P"] + c["fh"] <= (c["H"] - 1) * c["D"] + 1


def _run_conv(c, x, wk, old, acc, explicit=True):
    ext = _ext()
    xg, wg = _cl(x.cuda()), wk.cuda()
    if acc:
        out = _cl(old.cuda().clone())
        ret = ext.conv_mfma_acc(xg, wg, out, c["fh"], c["fw"], c["S"], c["P"],
                                c["D"])
        assert ret.data_ptr() == out.data_ptr()
        return out
    oh, ow = (c["OH"], c["OW"]) if explicit else (-1, -1)
    return ext.conv_mfma(xg, wg, c["Cout"], c["fh"], c["fw"], c["S"], c["P"],
                         c["D"], oh, ow)


@gpu
@requires_gpu
@pytest.mark.parametrize("acc", [False, True],
                         ids=["conv_mfma", "conv_mfma_acc"])
@pytest.mark.parametrize("c", CONV_EXACT, ids=lambda c: c["name"])
def test_conv_exact(c, acc):
    """conv_mfma (explicit and derived OH/OW) and conv_mfma_acc, bit-exact."""
    M = c["N"] * c["OH"] * c["OW"]
    assert c["name"].startswith(_conv_tier(M, c["Cout"])[0])
    x, wk, old = _conv_args(c)
    S64, _ = _conv_refs(c)
    _assert_padding_visible(c, x, wk, S64)
    got = _run_conv(c, x, wk, old, acc)
    assert got.is_contiguous(memory_format=torch.channels_last)
    if acc:
        _assert_bits("conv_mfma_acc", got, _to_bf16(old.double() + S64))
        return
    _assert_bits("conv_mfma explicit OH/OW", got, _to_bf16(S64))
    natural = (_natural(c["H"], c["fh"], c["S"], c["P"], c["D"]),
               _natural(c["W"], c["fw"], c["S"], c["P"], c["D"]))
    if natural == (c["OH"], c["OW"]):
        got = _run_conv(c, x, wk, old, False, explicit=False)
        _assert_bits("conv_mfma derived OH/OW", got, _to_bf16(S64))


CONV_REAL = [
    _conv_case("t128-3x3-p1-c72", 3, 32, 9, 11, 72, 3, 3, 1, 1),
    _conv_case("t256-3x3-s2-p1-c200", 3, 64, 9, 11, 200, 3, 3, 2, 1),
    _conv_case("t256-4x4-d2-p2-c200", 3, 32, 5, 6, 200, 4, 4, 1, 2, D=2),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("acc", [False, True],
                         ids=["conv_mfma", "conv_mfma_acc"])
@pytest.mark.parametrize("c", CONV_REAL, ids=lambda c: c["name"])
def test_conv_real(c, acc):
    """Real-valued inputs, derived bound (module docstring)."""
    x, wk, old = _conv_args(c, True)
    S64, absprod = _conv_refs(c, True)
    K = c["fh"] * c["fw"] * c["Cin"]
    got = _run_conv(c, x, wk, old, acc)
    if acc:
        ref = old.double() + S64
        _assert_bound("conv_mfma_acc", got, ref, absprod, K, BF16,
                      2.0 ** -24 * ref.abs())
    else:
        _assert_bound("conv_mfma", got, S64, absprod, K, BF16)


def _class_taps(k, pp, ph, pw):
    return [(r, s) for r in range(k) for s in range(k)
            if (ph - pp + r) % 2 == 0 and (pw - pp + s) % 2 == 0]


def _written_mask(c):
    """Pixels of the real output that belong to a class with taps."""
    m = torch.zeros(c["OH"], c["OW"], dtype=torch.bool)
    for ph in (0, 1):
        for pw in (0, 1):
            if _class_taps(c["k"], c["pp"], ph, pw):
                m[ph::2, pw::2] = True
    return m


@gpu
@requires_gpu
@pytest.mark.parametrize("c", PAR_EXACT, ids=lambda c: c["name"])
def test_conv_par_exact(c):
    """_conv_parity (four conv_par class launches) against the conv over the
    explicitly zero-dilated input; pixels of tap-less classes keep their
    prior contents."""
    from tensorflowonspark_amd.ops.modules import _conv_parity
    cc = _par_as_conv(c)
    x, wk, old = _conv_args(cc)
    S64, _ = _conv_refs(cc)
    _assert_padding_visible(cc, x, wk, S64)
    sizes = {(len(range(ph, c["OH"], 2)), len(range(pw, c["OW"], 2)))
             for ph in (0, 1) for pw in (0, 1)}
    if c["OH"] % 2 and not c["OW"] % 2:
        assert len(sizes) == 2          # odd x even: the classes differ
    written = _written_mask(c)
    if c["k"] == 1:
        assert int(written.sum()) == \
            ((c["OH"] + 1) // 2) * ((c["OW"] + 1) // 2)
    else:
        assert written.all()
    exp = _to_bf16(old.double() + S64) if c["accum"] else _to_bf16(S64)
    exp = torch.where(written, exp, old)
    out = _cl(old.cuda().clone())
    wperm = wk.reshape(c["OC"], c["k"], c["k"], c["KC"]).cuda()
    _conv_parity(_cl(x.cuda()), wperm, out, c["k"], c["pp"], c["accum"])
    _assert_bits("_conv_parity", out, exp)


@gpu
@requires_gpu
@pytest.mark.parametrize("accum", [False, True], ids=["store", "accum"])
def test_conv_par_single_class_exact(accum):
    """One hand-built class call: k=3, pp=1, class (1, 1) has the four corner
    taps; every pixel of the other three classes keeps its prior contents."""
    c = PAR_EXACT[0]
    cc = _par_as_conv(c)
    x, wk, old = _conv_args(cc)
    S64, _ = _conv_refs(cc)
    taps = [(0, 0), (0, 2), (2, 0), (2, 2)]
    assert taps == _class_taps(3, 1, 1, 1)
    w4 = wk.reshape(c["OC"], 3, 3, c["KC"])
    wcls = torch.stack([w4[:, r, s, :] for r, s in taps], dim=1) \
        .reshape(c["OC"], 4 * c["KC"]).contiguous()
    mask = torch.zeros(c["OH"], c["OW"], dtype=torch.bool)
    mask[1::2, 1::2] = True
    exp = _to_bf16(old.double() + S64) if accum else _to_bf16(S64)
    exp = torch.where(mask, exp, old)
    out = _cl(old.cuda().clone())
    _ext().conv_par(_cl(x.cuda()), wcls.cuda(), out, [r for r, _ in taps],
                    [s for _, s in taps], 1, accum)
    _assert_bits("conv_par class (1,1)", out, exp)


@gpu
@requires_gpu
@pytest.mark.parametrize("c", [PAR_EXACT[0], PAR_EXACT[4]],
                         ids=lambda c: c["name"])
def test_conv_parity_packed_exact(c):
    """_conv_parity_packed (the fused-bottleneck dgrad route) with per-class
    weights laid out as the pack plan does: [OC, nr, ns, KC] over the
    Cartesian (r, s) lists of each class."""
    from tensorflowonspark_amd.ops.modules import _conv_parity_packed
    from tensorflowonspark_amd.ops.packplan import _class_taps as plan_taps
    cc = _par_as_conv(c)
    x, wk, old = _conv_args(cc)
    S64, _ = _conv_refs(cc)
    w4 = wk.reshape(c["OC"], c["k"], c["k"], c["KC"])
    packs = {}
    for (ph, pw), (rl, sl) in plan_taps(c["k"], c["pp"]).items():
        assert [(r, s) for r in rl for s in sl] == \
            _class_taps(c["k"], c["pp"], ph, pw)
        packs["w_{}{}".format(ph, pw)] = torch.stack(
            [w4[:, r, s, :] for r in rl for s in sl], dim=1) \
            .reshape(c["OC"], len(rl), len(sl), c["KC"]).contiguous().cuda()
    exp = _to_bf16(old.double() + S64) if c["accum"] else _to_bf16(S64)
    out = _cl(old.cuda().clone())
    _conv_parity_packed(_cl(x.cuda()), packs, "w", out, c["k"], c["pp"],
                        c["accum"])
    _assert_bits("_conv_parity_packed", out, exp)


@gpu
@requires_gpu
def test_conv_par_real():
    """_conv_parity k=3 pp=1 on real-valued inputs, derived bound."""
    from tensorflowonspark_amd.ops.modules import _conv_parity
    c = dict(name="real-k3-pp1-9x8", N=2, KC=64, h=5, w=4, OC=72, k=3, pp=1,
             OH=9, OW=8)
    cc = _par_as_conv(c)
    x, wk, old = _conv_args(cc, True)
    S64, absprod = _conv_refs(cc, True)
    out = _cl(old.cuda().clone())
    wperm = wk.reshape(c["OC"], 3, 3, c["KC"]).cuda()
    _conv_parity(_cl(x.cuda()), wperm, out, 3, 1)
    _assert_bound("_conv_parity", out, S64, absprod, 9 * c["KC"], BF16)


# ---------------------------------------------------------------------------
# wrw
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("c", WRW_EXACT, ids=lambda c: c[0])
def test_conv_wrw2_exact(c):
    """conv_wrw2 (fp32 dW) bit-exact, including split-M slices that receive
    no K-step and must contribute zeros."""
    name, N, Cin, H, W, Cout, k, stride, P, split, empty = c
    M = N * _natural(H, k, stride, P) * _natural(W, k, stride, P)
    assert _wrw2_split(Cout, Cin, M) == split
    assert (_wrw2_empty_slices(k * k, split, M) >= 1) == empty
    x, dy = _wrw_inputs(*c[:9])
    S64, _ = _wrw_refs(*c[:9])
    ext = _ext()
    # leave non-zero bytes where the allocator is likely to put the split-M
    # workspace (at::empty): an empty slice has to write its zeros itself
    junk = torch.full((split, Cout * k * k * Cin), 7.0, device="cuda")
    del junk
    got = ext.conv_wrw2(_cl(dy.cuda()), _cl(x.cuda()), k, k, stride, P)
    _assert_bits("conv_wrw2", got, S64.float())


@gpu
@requires_gpu
@pytest.mark.parametrize("c", [WRW_EXACT[1], WRW_EXACT[6], WRW_EXACT[7]],
                         ids=lambda c: c[0])
def test_conv_wrw2_real(c):
    """Real-valued inputs; K of the bound is the whole pixel count M."""
    name, N, Cin, H, W, Cout, k, stride, P, split, empty = c
    M = N * _natural(H, k, stride, P) * _natural(W, k, stride, P)
    args = c[:9] + (True,)
    x, dy = _wrw_inputs(*args)
    S64, absprod = _wrw_refs(*args)
    got = _ext().conv_wrw2(_cl(dy.cuda()), _cl(x.cuda()), k, k, stride, P)
    _assert_bound("conv_wrw2", got, S64, absprod, M, FP32)


@gpu
@requires_gpu
def test_stem_conv7x7_exact():
    """StemConv7x7 forward (conv_stem) and weight gradient (conv_stem_wrw)
    on an integer image, bit-exact against the fp64 7x7/s2/p3 conv."""
    from tensorflowonspark_amd.ops.modules import StemConv7x7
    x, w, dy = _stem_inputs()
    y64, dw64 = _stem_contract(FP64)
    m = StemConv7x7(3, STEM["Cout"]).cuda()
    with torch.no_grad():
        m.weight.copy_(w.float())
    y = m(_cl(x.cuda()))
    assert type(y.grad_fn).__name__ == "_StemConvFnBackward"
    _assert_bits("stem fwd", y, _to_bf16(y64))
    y.backward(_cl(dy.cuda()))
    assert m.weight.grad.dtype == FP32
    _assert_bits("stem wgrad", m.weight.grad, dw64.float())


# ---------------------------------------------------------------------------
# module wiring (derived bound; y, dx, dw against fp64)
# ---------------------------------------------------------------------------

_BACKEND_ENV = ("TFOS_CONV1X1", "TFOS_CONV3X3", "TFOS_CONVT", "TFOS_STEM",
                "TFOS_ALLOW_EAGER_FALLBACK")


def _set_real_weight(param, gen):
    """randn/4 with a scale per leading index, already bf16-representable:
    the module's own .to(bfloat16) is then exact."""
    w = _real(gen, *param.shape).float()
    with torch.no_grad():
        param.copy_(w)
    return w.double()


def _grads64(fn, x, w, dy):
    """fn(x, w), d/dx and d/dw for upstream dy, in fp64 by autograd."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = fn(x, w)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


WIRING = [
    # name, module ctor args, expected autograd node, taps
    ("conv1x1-s1", "Conv1x1", dict(stride=1), "_Conv1x1FnBackward", 1),
    ("conv1x1-s2", "Conv1x1", dict(stride=2), "_Conv1x1S2FnBackward", 1),
    ("conv3x3-s1", "Conv3x3", dict(stride=1), "_Conv3x3FnBackward", 9),
    ("conv3x3-s2", "Conv3x3", dict(stride=2), "_Conv3x3FnBackward", 9),
    ("convT-k4-p1-op0", "ConvTranspose2dMFMA",
     dict(kernel_size=4, stride=2, padding=1, output_padding=0),
     "_ConvT2dFnBackward", 16),
    ("convT-k3-p1-op1", "ConvTranspose2dMFMA",
     dict(kernel_size=3, stride=2, padding=1, output_padding=1),
     "_ConvT2dFnBackward", 9),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("case", WIRING, ids=lambda c: c[0])
def test_module_wiring(case, monkeypatch):
    """Conv1x1 / Conv3x3 / ConvTranspose2dMFMA forward and backward on a
    2x64x64x64 input with 96 output channels: the in-tree autograd Function
    must have run, and y, dx, dw stay within the derived bound of fp64.

    The reference is the unfold + fp64 matmul helper on the device (no fp64
    library convolution).  TFOS_WRW=mfma2 routes the Conv1x1 / Conv3x3 weight
    gradient to conv_wrw2 (fp32 dW); ConvTranspose2dMFMA takes its weight
    gradient from the library in bf16 — compared with a bf16 half-ulp, and no
    part of the tier table."""
    from tensorflowonspark_amd.ops import modules
    name, cls, kw, node, taps = case
    for k in _BACKEND_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TFOS_WRW", "mfma2")
    N, Cin, H, W, Cout = 2, 64, 64, 64, 96
    g = _gen("wiring-" + name)
    m = getattr(modules, cls)(Cin, Cout, **kw).cuda()
    w64 = _set_real_weight(m.weight, g).cuda()
    x = _real(g, Cin, N, H, W).permute(1, 0, 2, 3)
    xg = _cl(x.cuda()).requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == node
    assert y.dtype == BF16
    dy = _real(g, Cout, N, y.shape[2], y.shape[3]).permute(1, 0, 2, 3)
    dyg = _cl(dy.cuda())
    y.backward(dyg)

    if cls == "ConvTranspose2dMFMA":
        fn = lambda a, b: _convT_ref(a, b, kw["padding"], kw["output_padding"])
        pixels, dw_dtype = N * H * W, BF16
    else:
        S, P = kw["stride"], (1 if taps == 9 else 0)
        kk = 3 if taps == 9 else 1
        fn = lambda a, b: _conv_ref(a, _w4_to_wk(b), kk, kk, S, P, 1,
                                    y.shape[2], y.shape[3])
        pixels, dw_dtype = N * y.shape[2] * y.shape[3], FP32
    x64, dy64 = xg.detach().double(), dyg.double()
    y64, dx64, dw64 = _grads64(fn, x64, w64, dy64)
    ya, dxa, dwa = _grads64(fn, x64.abs(), w64.abs(), dy64.abs())
    assert y64.shape == y.shape
    _assert_bound(name + " y", y, y64, ya, taps * Cin, BF16)
    _assert_bound(name + " dx", xg.grad, dx64, dxa, taps * Cout, BF16)
    _assert_bound(name + " dw", m.weight.grad, dw64, dwa, pixels, dw_dtype)


@gpu
@requires_gpu
def test_dense_mfma_module():
    """DenseMFMA forward (256x64 tile) and backward (dx through the K-padding
    path on the 128^2 tile; dw from the library fp32 matmul, rounded to bf16)
    within the derived bound."""
    from tensorflowonspark_amd.ops.modules import DenseMFMA
    g = _gen("dense")
    M, K, N = 50, 96, 40
    assert _gemm_tier(M, N, K)[0] == SKINNY and _gemm_tier(M, K, 64)[0] == T128
    m = DenseMFMA(K, N).cuda()
    w64 = _set_real_weight(m.weight, g)
    assert float(m.bias.detach().abs().max()) == 0.0
    x = _real(g, M, K)
    dy = _real(g, M, N)
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    y.backward(dy.cuda())
    x64, dy64 = x.double(), dy.double()
    _assert_bound("dense y", y, x64 @ w64.t(), x64.abs() @ w64.abs().t(),
                  K, BF16)
    _assert_bound("dense dx", xg.grad, dy64 @ w64, dy64.abs() @ w64.abs(),
                  N, BF16)
    _assert_bound("dense dw", m.weight.grad, dy64.t() @ x64,
                  dy64.abs().t() @ x64.abs(), M, BF16)


@gpu
@requires_gpu
def test_conv2d_im2col_module():
    """Conv2dIm2colMFMA (K = 18 padded to 32) forward and weight gradient
    within the derived bound; the input is the network's first layer and
    carries no gradient."""
    from tensorflowonspark_amd.ops.modules import Conv2dIm2colMFMA
    g = _gen("im2col")
    N, Cin, H, W, Cout, k = 2, 2, 9, 9, 32, 3
    m = Conv2dIm2colMFMA(Cin, Cout, k).cuda()
    w64 = _set_real_weight(m.weight, g)
    x = _real(g, Cin, N, H, W).permute(1, 0, 2, 3).contiguous()
    y = m(x.cuda())
    dy = _real(g, Cout, N, y.shape[2], y.shape[3]).permute(1, 0, 2, 3) \
        .contiguous()
    y.backward(dy.cuda())
    fn = lambda a, b: F.conv2d(a, b)
    y64, _, dw64 = _grads64(fn, x.double(), w64, dy.double())
    ya, _, dwa = _grads64(fn, x.double().abs(), w64.abs(), dy.double().abs())
    _assert_bound("im2col y", y, y64, ya, Cin * k * k, BF16)
    _assert_bound("im2col dw", m.weight.grad, dw64, dwa,
                  N * y.shape[2] * y.shape[3], BF16)
