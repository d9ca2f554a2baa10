"""The tail of the in-tree weight-gradient path: the parallel split-M reduce,
the 32-channel-tile stem wrw kernel, the per-device zero guard and the
channels_last allocation helper.

Exact cases use small integers (bf16-exact, every product and every partial
sum far below 2^24), so ANY summation order reproduces the fp64 CPU reference
with zero error: that pins the reduce whatever tree it uses.  The real-valued
case uses the bound of tests/test_gpu_mfma.py::test_conv_wrw2_real,

    |got - ref64| <= M 2^-23 sum|dy||x| + 2^-24 |ref64|

(M the pixel count the split slices share).
"""

import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

BF16 = torch.bfloat16
CL = torch.channels_last


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _cl(t):
    return t.contiguous(memory_format=CL)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).to(BF16)


def _wrw2_split(Cout, Cin, M):
    """tfosr_wrw2_split."""
    ntiles = ((Cout + 63) // 64) * ((Cin + 63) // 64)
    split = max(1, 1024 // ntiles)
    steps = (M + 31) // 32
    while split * 8 > steps and split > 1:
        split //= 2
    return split


def _wgrad64(dy, x, kh, kw, stride, pad, fd=1):
    """fp64 weight gradient [Cout, Cin, kh, kw] of conv2d on the CPU."""
    w = torch.zeros(dy.shape[1], x.shape[1], kh, kw, dtype=torch.float64,
                    requires_grad=True)
    y = F.conv2d(x.double(), w, None, stride, pad, fd)
    assert y.shape == dy.shape, (tuple(y.shape), tuple(dy.shape))
    y.backward(dy.double())
    return w.grad


def _assert_equal(what, got, ref64):
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    err = (got - ref64).abs()
    print("  {:<28s} max |err| {:.3e}  max |ref| {:.0f}".format(
        what, err.max().item(), ref64.abs().max().item()))
    nbad = int((err != 0).sum())
    assert nbad == 0, "{}: {} of {} elements differ from fp64".format(
        what, nbad, err.numel())


# ---------------------------------------------------------------------------
# split-M reduce through conv_wrw2
# ---------------------------------------------------------------------------

# (name, N, H, W, Cin, Cout, k, pad, fd, split).  Splits up to 64 take the
# one-level reduce; the last two take two levels (chunks of 64 slices): 128
# is two whole chunks, 341 is five chunks and a ragged sixth of 21.
REDUCE = [
    ("3x3-split2", 2, 16, 16, 64, 64, 3, 1, 1, 2),
    ("3x3-split16", 4, 32, 32, 64, 64, 3, 1, 1, 16),
    ("3x3-192-split10", 4, 32, 32, 64, 192, 3, 1, 1, 10),
    ("3x3-192-split21", 6, 32, 32, 64, 192, 3, 1, 1, 21),
    ("3x3-24to40-n8640", 4, 32, 32, 24, 40, 3, 1, 1, 16),
    ("1x1-tn-64to96", 4, 32, 32, 64, 96, 1, 0, 1, 16),
    ("3x3-fd2", 4, 32, 32, 64, 64, 3, 2, 2, 16),
    ("3x3-8to8-split128", 8, 64, 64, 8, 8, 3, 1, 1, 128),
    ("3x3-8to136-split341", 6, 128, 120, 8, 136, 3, 1, 1, 341),
]


@functools.lru_cache(maxsize=None)
def _reduce_case(name):
    c = next(c for c in REDUCE if c[0] == name)
    _, N, H, W, Cin, Cout, k, pad, fd, _ = c
    g = _gen("wrwtail-" + name)
    x = _ints(g, N, Cin, H, W)
    dy = _ints(g, N, Cout, H, W)       # every case keeps the image size
    ref = _wgrad64(dy, x, k, k, 1, pad, fd)
    return x, dy, ref.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin)


@gpu
@requires_gpu
@pytest.mark.parametrize("c", REDUCE, ids=lambda c: c[0])
def test_reduce_exact(c):
    """conv_wrw2 over split counts 2..341, one- and two-level reduce, a
    column count that is no multiple of the block, the 1x1 TN kernel and a
    dilated filter: zero error against fp64."""
    name, N, H, W, Cin, Cout, k, pad, fd, split = c
    assert _wrw2_split(Cout, Cin, N * H * W) == split
    x, dy, ref = _reduce_case(name)
    assert ref.abs().max() < 2 ** 24
    got = _ext().conv_wrw2(_cl(dy.cuda()), _cl(x.cuda()), k, k, 1, pad, fd)
    _assert_equal("conv_wrw2 " + name, got, ref)
    again = _ext().conv_wrw2(_cl(dy.cuda()), _cl(x.cuda()), k, k, 1, pad, fd)
    assert torch.equal(got, again)


# ---------------------------------------------------------------------------
# stem wrw through conv_stem_wrw
# ---------------------------------------------------------------------------

STEM_COUT = 64


@functools.lru_cache(maxsize=None)
def _stem_case(HW, real=False):
    g = _gen("wrwtail-stem-{}-{}".format(HW, real))
    N, OHW = 2, (HW + 6 - 7) // 2 + 1
    if real:
        x = (torch.randn(N, 3, HW, HW, generator=g) / 4).to(BF16)
        dy = (torch.randn(N, STEM_COUT, OHW, OHW, generator=g) / 4).to(BF16)
    else:
        x, dy = _ints(g, N, 3, HW, HW), _ints(g, N, STEM_COUT, OHW, OHW)
    return x, dy


def _stem_x4(x):
    """The padded NHWC4 image as _StemConvFn.forward builds it."""
    from tensorflowonspark_amd.ops.modules import _cl_alloc
    N, _, H, W = x.shape
    x4 = _cl_alloc((N, 4, H + 6, W + 6), x.device, zero=True)
    x4[:, :3, 3:H + 3, 3:W + 3] = x
    return x4


def _stem_unpack(dw224):
    """[Cout, 224] -> [Cout, 3, 7, 7] as _StemConvFn.backward unpacks it."""
    return dw224.view(-1, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2)


@gpu
@requires_gpu
@pytest.mark.parametrize("HW", [32, 38])
def test_stem_wrw_exact(HW):
    """conv_stem_wrw at M = 512 and at M = 722 (no multiple of the K-step,
    odd row length): zero error on the 64x3x7x7 real entries and exact zeros
    in the 4th (pad) channel.

    The 8th pixel of a filter row is a pad column of the WEIGHT only: its
    gradient pairs dy with the image pixel one past the 7-wide row and is not
    zero (the module drops it).  It is therefore held to its own fp64 value,
    the weight gradient of a 7x8 filter over the padded image, instead of to
    zero; that reference covers all 224 columns."""
    x, dy = _stem_case(HW)
    OHW = dy.shape[2]
    assert 2 * OHW * OHW == {32: 512, 38: 722}[HW]
    x4 = _stem_x4(x.cuda())
    got = _ext().conv_stem_wrw(_cl(dy.cuda()), x4)
    assert got.shape == (STEM_COUT, 224) and got.dtype == torch.float32
    _assert_equal("stem dw[64,3,7,7]", _stem_unpack(got),
                  _wgrad64(dy, x, 7, 7, 2, 3))
    g4 = got.view(STEM_COUT, 7, 8, 4)
    assert int((g4[..., 3] != 0).sum()) == 0, "4th channel must be zero"
    full = _wgrad64(dy, x4.cpu(), 7, 8, 2, 0)          # [Cout, 4, 7, 8]
    _assert_equal("stem dw[64,7,8,4]", g4, full.permute(0, 2, 3, 1))


@gpu
@requires_gpu
def test_stem_wrw_real():
    """Random data at M = 512 under test_conv_wrw2_real's bound."""
    x, dy = _stem_case(32, True)
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    got = _stem_unpack(_ext().conv_stem_wrw(_cl(dy.cuda()),
                                            _stem_x4(x.cuda())))
    ref = _wgrad64(dy, x, 7, 7, 2, 3)
    absprod = _wgrad64(dy.abs(), x.abs(), 7, 7, 2, 3)
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    tol = M * 2.0 ** -23 * absprod + 2.0 ** -24 * ref.abs()
    err = (got - ref).abs()
    print("  stem wrw real: err max {:.3e}, smallest bound {:.3e}".format(
        err.max().item(), tol.min().item()))
    assert int((err > tol).sum()) == 0


# ---------------------------------------------------------------------------
# zero guard
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
def test_guard_streams():
    """A padded 3x3 conv_mfma three times on the current stream, once on a
    side stream and at once again on the default stream: every result is the
    fp64 reference rounded once to bf16, border pixels included."""
    g = _gen("wrwtail-guard")
    x = _ints(g, 2, 64, 8, 8)
    w = _ints(g, 64, 64, 3, 3)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1).float().bfloat16()
    ext = _ext()
    xd = _cl(x.cuda())
    wk = w.permute(0, 2, 3, 1).reshape(64, 9 * 64).contiguous().cuda()

    def run():
        return ext.conv_mfma(xd, wk, 64, 3, 3, 1, 1, 1, -1, -1)
    outs = [run() for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs.append(run())
    outs.append(run())
    torch.cuda.synchronize()
    for i, y in enumerate(outs):
        assert y.is_contiguous(memory_format=CL)
        assert torch.equal(y.cpu(), ref), "run {}".format(i)


# ---------------------------------------------------------------------------
# channels_last allocation
# ---------------------------------------------------------------------------

def test_cl_alloc_cpu():
    """_cl_alloc: the strides of empty(shape).contiguous(channels_last), the
    requested dtype, zeros when asked."""
    from tensorflowonspark_amd.ops.modules import _cl_alloc
    for shape in [(2, 64, 16, 16), (3, 4, 38, 38), (2, 8, 1, 7), (1, 8, 1, 1),
                  (3, 1, 5, 5)]:
        old = torch.empty(shape, dtype=BF16).contiguous(memory_format=CL)
        t = _cl_alloc(shape, "cpu")
        assert t.shape == old.shape and t.stride() == old.stride(), shape
        assert t.dtype == BF16 and t.is_contiguous(memory_format=CL)
        z = _cl_alloc(torch.Size(shape), "cpu", dtype=torch.float32,
                      zero=True)
        assert z.dtype == torch.float32 and z.stride() == old.stride()
        assert int((z != 0).sum()) == 0


@gpu
@requires_gpu
def test_conv3x3_s2_dx_layout():
    """Conv3x3 stride 2 backward: x.grad is channels_last-contiguous and
    bit-identical to conv_par run into a buffer allocated the old way."""
    from tensorflowonspark_amd.ops.modules import Conv3x3, _conv_parity
    from tensorflowonspark_amd.ops.packplan import flipped
    g = _gen("wrwtail-dx")
    m = Conv3x3(64, 96, stride=2).cuda()
    with torch.no_grad():
        m.weight.copy_((torch.randn(96, 64, 3, 3, generator=g) / 16)
                       .to(BF16).float())
    x = _cl((torch.randn(2, 64, 16, 16, generator=g) / 4).to(BF16).cuda()) \
        .requires_grad_(True)
    dy = _cl((torch.randn(2, 96, 8, 8, generator=g) / 4).to(BF16).cuda())
    y = m(x)
    assert type(y.grad_fn).__name__ == "_Conv3x3FnBackward"
    y.backward(dy)
    assert x.grad.is_contiguous(memory_format=CL)
    assert x.grad.stride() == x.stride() and x.grad.dtype == BF16
    old = torch.empty(x.shape, device=x.device, dtype=BF16) \
        .contiguous(memory_format=CL)
    _conv_parity(dy, flipped(m.weight.detach()), old, 3, 1)
    assert torch.equal(x.grad.view(torch.int16), old.view(torch.int16))
