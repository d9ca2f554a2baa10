"""Cases, inputs and fp64 references shared by test_atrous_cpu.py and
test_gpu_atrous.py (atrous = filter-dilated convolution).

The method is that of test_gpu_mfma.py.  Exact probes use integers in [-3, 3]
stored in bf16 (activations leave 0 out so that padding is visible), for which
every product is an integer and sum |a||b| < 2^24, so every fp32 partial sum
in every order is exact: fp32 outputs equal the fp64 reference bit for bit and
bf16 outputs equal its round-to-nearest-even.  Real-valued probes use the
derived bound

    |got - ref64| <= K * 2^-23 * (|A| |B|^T) + half_ulp(out dtype, ref64)

with K the contraction length.  The fp64 reference is ``F.conv2d`` with
``dilation=fd`` in fp64 and, for gradients, fp64 autograd on the CPU; each is
computed once per case and never modified.
"""

import functools
import zlib

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
FP32 = torch.float32
FP64 = torch.float64
EXACT_LIMIT = 2 ** 24


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, *shape, nonzero=False):
    """Integers in [-3, 3] (without 0 when ``nonzero``) as bf16."""
    if nonzero:
        mag = torch.randint(1, 4, shape, generator=g)
        sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
        return (mag * sign).to(BF16)
    return torch.randint(-3, 4, shape, generator=g).to(BF16)


def real(g, rows, *rest):
    """randn/4 with a distinct scale in [0.5, 2] per leading index, as bf16."""
    v = torch.randn(rows, *rest, generator=g) / 4
    frac = torch.randperm(rows, generator=g).double() / max(rows - 1, 1)
    s = (0.5 + 1.5 * frac).float().view(rows, *([1] * len(rest)))
    return (v * s).to(BF16)


def real_nchw(g, N, C, H, W):
    """Real-valued [N, C, H, W] with a distinct scale per channel."""
    return real(g, C, N, H, W).permute(1, 0, 2, 3).contiguous()


def half_ulp(ref64, dtype):
    """Half an ulp of ``dtype`` at |ref64|."""
    if dtype == BF16:
        _, e = torch.frexp(ref64)
        half = torch.ldexp(torch.ones_like(ref64), e - 9)
        return torch.where(ref64 == 0, torch.zeros_like(ref64), half)
    return 2.0 ** -24 * ref64.abs()


def to_bf16(ref64):
    return ref64.float().bfloat16()


def assert_bits(what, got, exp):
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


def assert_bound(what, got, ref64, absprod, K, out_dtype):
    """|got - ref64| <= K 2^-23 absprod + half_ulp(out dtype)."""
    got = got.detach().double().cpu()
    ref64, absprod = ref64.cpu(), absprod.cpu()
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), "{}: non-finite values".format(what)
    tol = K * 2.0 ** -23 * absprod + half_ulp(ref64, out_dtype)
    err = (got - ref64).abs()
    worst = (err - tol).argmax()
    print("  {:<26s} K {:<6d} err max {:.3e}  worst err/bound {:.3e}/{:.3e}"
          .format(what, K, err.max().item(), err.reshape(-1)[worst].item(),
                  tol.reshape(-1)[worst].item()))
    nbad = int((err > tol).sum())
    assert nbad == 0, "{}: {} of {} elements beyond the bound".format(
        what, nbad, err.numel())


def w4_to_wk(w4):
    """Conv2d weight [Cout, Cin, fh, fw] -> kernel layout [Cout, fh*fw*Cin]."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1).contiguous()


def out_size(size, k, S, P, fd):
    return (size + 2 * P - fd * (k - 1) - 1) // S + 1


def conv_tier(M, Cout):
    """launch_conv's dispatch -> (tile name, workgroups)."""
    cdiv = lambda a, b: (a + b - 1) // b
    if Cout >= 192:
        return "t256", cdiv(M, 256) * cdiv(Cout, 256)
    return "t128", cdiv(M, 256) * cdiv(Cout, 128)


def wrw2_split(Cout, Cin, M):
    """tfosr_wrw2_split."""
    ntiles = ((Cout + 63) // 64) * ((Cin + 63) // 64)
    split = max(1, 1024 // ntiles)
    steps = (M + 31) // 32
    while split * 8 > steps and split > 1:
        split //= 2
    return split


# ---------------------------------------------------------------------------
# forward cases (the kernel's view: Cin = contraction channels)
# ---------------------------------------------------------------------------

def _fwd(name, N, Cin, H, W, Cout, fh, fw, fd, P, S):
    return dict(name=name, N=N, Cin=Cin, H=H, W=W, Cout=Cout, fh=fh, fw=fw,
                fd=fd, P=P, S=S, OH=out_size(H, fh, S, P, fd),
                OW=out_size(W, fw, S, P, fd))


FWD_EXACT = [
    _fwd("t128-d2", 2, 32, 12, 11, 72, 3, 3, 2, 2, 1),
    _fwd("t128-d3-rect", 1, 64, 9, 7, 64, 3, 3, 3, 3, 1),
    _fwd("t256-d2", 2, 32, 12, 11, 200, 3, 3, 2, 2, 1),
    _fwd("pad0", 1, 32, 9, 9, 64, 3, 3, 2, 0, 1),
    _fwd("pad1", 1, 32, 9, 9, 64, 3, 3, 2, 1, 1),
    _fwd("s2", 1, 32, 9, 9, 64, 3, 3, 2, 2, 2),
    _fwd("f2x3", 1, 32, 8, 9, 64, 2, 3, 2, 2, 1),
    _fwd("aspp", 1, 32, 16, 16, 64, 3, 3, 12, 12, 1),
    _fwd("dead-5", 1, 32, 5, 5, 64, 3, 3, 5, 5, 1),
    _fwd("dead-7", 1, 32, 5, 5, 64, 3, 3, 7, 7, 1),
]
FWD_BY_NAME = {c["name"]: c for c in FWD_EXACT}
DGRAD_NAMES = ["t128-d2", "t128-d3-rect", "t256-d2", "aspp"]
# the regression guard: the fd = 1 path of the same entry points
FD1_CASE = _fwd("fd1-t128", 2, 32, 9, 11, 72, 3, 3, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def fwd_inputs(name, is_real=False):
    """(x [N,Cin,H,W], w4 [Cout,Cin,fh,fw]) as bf16."""
    c = FWD_BY_NAME.get(name, FD1_CASE)
    g = gen("atrous-fwd-" + name + ("-real" if is_real else ""))
    if is_real:
        return (real_nchw(g, c["N"], c["Cin"], c["H"], c["W"]),
                real(g, c["Cout"], c["Cin"], c["fh"], c["fw"]))
    return (ints(g, c["N"], c["Cin"], c["H"], c["W"], nonzero=True),
            ints(g, c["Cout"], c["Cin"], c["fh"], c["fw"]))


def fwd_contract(c, x, w4, dt):
    return F.conv2d(x.to(dt), w4.to(dt), stride=c["S"], padding=c["P"],
                    dilation=c["fd"])


@functools.lru_cache(maxsize=None)
def fwd_refs(name, is_real=False):
    """(y64, sum |x||w|) on the CPU."""
    c = FWD_BY_NAME.get(name, FD1_CASE)
    x, w4 = fwd_inputs(name, is_real)
    return fwd_contract(c, x, w4, FP64), fwd_contract(c, x.abs(), w4.abs(),
                                                      FP64)


# ---------------------------------------------------------------------------
# dgrad form of a forward case: the kernel reads dy (case Cin channels) and
# writes dx (case Cout channels), i.e. the underlying conv maps
# x [N, c.Cout, H, W] -> y [N, c.Cin, H, W] with weight [c.Cin, c.Cout, 3, 3],
# stride 1 and padding = dilation = fd (output size H x W).
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dgrad_inputs(name, is_real=False):
    """(dy [N,c.Cin,H,W], w4 [c.Cin,c.Cout,3,3]) as bf16."""
    c = FWD_BY_NAME[name]
    assert c["S"] == 1 and c["P"] == c["fd"] and c["fh"] == c["fw"] == 3
    g = gen("atrous-dgrad-" + name + ("-real" if is_real else ""))
    if is_real:
        return (real_nchw(g, c["N"], c["Cin"], c["H"], c["W"]),
                real(g, c["Cin"], c["Cout"], 3, 3))
    return (ints(g, c["N"], c["Cin"], c["H"], c["W"], nonzero=True),
            ints(g, c["Cin"], c["Cout"], 3, 3))


def dgrad_weight(w4):
    """W'[cin][r][s][cout] = W[cout][2-r][2-s][cin] as [cin, 9*cout]."""
    return w4.flip(2, 3).permute(1, 2, 3, 0).reshape(w4.shape[1], -1) \
        .contiguous()


def dgrad_contract(c, dy, w4, dt):
    """fp autograd gradient of conv2d(x, w4, dilation=fd) wrt x."""
    x = torch.zeros(c["N"], c["Cout"], c["H"], c["W"], dtype=dt,
                    requires_grad=True)
    y = F.conv2d(x, w4.to(dt), padding=c["fd"], dilation=c["fd"])
    y.backward(dy.to(dt))
    return x.grad.detach()


@functools.lru_cache(maxsize=None)
def dgrad_refs(name, is_real=False):
    c = FWD_BY_NAME[name]
    dy, w4 = dgrad_inputs(name, is_real)
    return dgrad_contract(c, dy, w4, FP64), dgrad_contract(c, dy.abs(),
                                                           w4.abs(), FP64)


# ---------------------------------------------------------------------------
# wrw cases: 3x3, stride 1, padding P, filter dilation fd
# ---------------------------------------------------------------------------

def _wrw(name, N, Cin, Cout, H, W, fd, P):
    return dict(name=name, N=N, Cin=Cin, Cout=Cout, H=H, W=W, fd=fd, P=P,
                OH=out_size(H, 3, 1, P, fd), OW=out_size(W, 3, 1, P, fd))


WRW_EXACT = [
    _wrw("ragged-40-24-d2", 2, 40, 24, 7, 6, 2, 2),
    _wrw("64-64-d3-rect", 1, 64, 64, 9, 7, 3, 3),
    _wrw("split2-d2", 1, 64, 64, 24, 23, 2, 2),
    _wrw("dead-d5", 1, 32, 32, 5, 5, 5, 5),
]
WRW_BY_NAME = {c["name"]: c for c in WRW_EXACT}
WRW_SPLIT_CASE = "split2-d2"
WRW_DEAD_CASE = "dead-d5"
WRW_REAL = _wrw("real-72-88-d2", 2, 72, 88, 10, 9, 2, 2)
WRW_FD1 = _wrw("fd1-64-64", 2, 64, 64, 8, 8, 1, 1)


def _wrw_case(name):
    for c in (WRW_REAL, WRW_FD1):
        if c["name"] == name:
            return c
    return WRW_BY_NAME[name]


@functools.lru_cache(maxsize=None)
def wrw_inputs(name, is_real=False):
    """(x [N,Cin,H,W], dy [N,Cout,OH,OW]) as bf16."""
    c = _wrw_case(name)
    g = gen("atrous-wrw-" + name)
    if is_real:
        return (real_nchw(g, c["N"], c["Cin"], c["H"], c["W"]),
                real_nchw(g, c["N"], c["Cout"], c["OH"], c["OW"]))
    return (ints(g, c["N"], c["Cin"], c["H"], c["W"], nonzero=True),
            ints(g, c["N"], c["Cout"], c["OH"], c["OW"]))


def wrw_contract(c, x, dy, dt):
    """fp autograd gradient of conv2d(x, w, dilation=fd) wrt w, in the
    kernel's [Cout, 9*Cin] layout."""
    w = torch.zeros(c["Cout"], c["Cin"], 3, 3, dtype=dt, requires_grad=True)
    y = F.conv2d(x.to(dt), w, padding=c["P"], dilation=c["fd"])
    y.backward(dy.to(dt))
    return w4_to_wk(w.grad.detach())


@functools.lru_cache(maxsize=None)
def wrw_refs(name, is_real=False):
    c = _wrw_case(name)
    x, dy = wrw_inputs(name, is_real)
    return wrw_contract(c, x, dy, FP64), wrw_contract(c, x.abs(), dy.abs(),
                                                      FP64)


def exact_contractions():
    """(name, fn(dtype, absval) -> contraction) for every exact case."""
    out = []
    for c in FWD_EXACT + [FD1_CASE]:
        x, w4 = fwd_inputs(c["name"])
        out.append(("fwd-" + c["name"], lambda dt, av, c=c, x=x, w4=w4:
                    fwd_contract(c, x.abs() if av else x,
                                 w4.abs() if av else w4, dt)))
    for name in DGRAD_NAMES:
        c = FWD_BY_NAME[name]
        dy, w4 = dgrad_inputs(name)
        out.append(("dgrad-" + name, lambda dt, av, c=c, dy=dy, w4=w4:
                    dgrad_contract(c, dy.abs() if av else dy,
                                   w4.abs() if av else w4, dt)))
    for c in WRW_EXACT + [WRW_FD1]:
        x, dy = wrw_inputs(c["name"])
        out.append(("wrw-" + c["name"], lambda dt, av, c=c, x=x, dy=dy:
                    wrw_contract(c, x.abs() if av else x,
                                 dy.abs() if av else dy, dt)))
    return out
