"""The halo-staged 3x3 stride-1 kernel (``csrc/conv3x3_halo.hip``) against
plain fp64 arithmetic, and the routing between it and the im2col kernel.

Every GPU test sets ``TFOS_CONV3X3_TILE=halo``, asks ``conv3x3_halo_plan``
which kernel ``conv_mfma`` will launch, and then calls ``conv_mfma``.  Probes,
references and bounds are those of ``test_gpu_mfma.py`` (imported): integer
inputs in [-3, 3] without zeros in the activations are exact in fp32 in any
summation order, so the chunk-major K order of this kernel has to give the
bits of ``bf16(ref64)``; real-valued inputs stay within
``K 2^-23 |A||B|^T + half ulp``.

Shapes are the smallest at which the kernel can go wrong: spans clamped at
either end of the tensor, tile edges in the middle of a row and of an image,
row wrap (W = 1) and image wrap (H = 1), one to four channel chunks, ragged
and full column tiles, the widest row the LDS budget takes and one wider
(which has to fall back), both tile heights (``TFOS_CONV3X3_HALO_BM``).
"""

import copy

import pytest
import torch
import torch.nn.functional as F

from test_gpu_bn_dual import _make_block, _rel_l2
from test_gpu_mfma import (BF16, CONV_EXACT, CONV_REAL, EXACT_LIMIT, FP32,
                           FP64, _assert_bits, _assert_bound,
                           _assert_padding_visible, _cl, _conv_args,
                           _conv_case, _conv_contract, _conv_refs, _ext, _gen,
                           _grads64, _conv_ref, _real, _set_real_weight,
                           _to_bf16, _w4_to_wk, gpu, requires_gpu)

MAX_W = 223        # (704 span rows - 256 - 2) / 2; asserted against the plan


def _halo_case(name, N, Cin, H, W, Cout):
    return _conv_case("halo-" + name, N, Cin, H, W, Cout, 3, 3, 1, 1)


HALO_EXACT = [
    _halo_case("m25-c64", 1, 32, 5, 5, 64),
    _halo_case("m297-c72", 3, 32, 9, 11, 72),
    _halo_case("m256-2chunks", 1, 64, 16, 16, 64),
    _halo_case("m512-2chunks", 2, 64, 16, 16, 64),
    _halo_case("m297-3chunks-c128", 3, 96, 9, 11, 128),
    _halo_case("m297-4chunks-c128", 3, 128, 9, 11, 128),
    _halo_case("h1-w7", 5, 32, 1, 7, 64),
    _halo_case("h6-w1", 4, 32, 6, 1, 64),
    _halo_case("widest", 2, 32, 3, MAX_W, 64),
    # 19 workgroups at BM 256 and 10 at BM 512: the XCD remap of the
    # workgroup id with a quotient >= 1 and a remainder (3 and 2)
    _halo_case("m4800-grid19", 3, 32, 40, 40, 64),
]
TOO_WIDE = _halo_case("too-wide", 2, 32, 3, MAX_W + 1, 64)
HALO_REAL = [
    _halo_case("real-m297-3chunks", 3, 96, 9, 11, 128),
    _halo_case("real-m512-2chunks", 2, 64, 16, 16, 64),
]


def _plan(c, **kw):
    return _ext().conv3x3_halo_plan(c["N"], c["H"], c["W"], c["Cin"],
                                    c["Cout"], **kw)


def _run(c, x, wk):
    return _ext().conv_mfma(_cl(x.cuda()), wk.cuda(), c["Cout"], 3, 3, 1, 1,
                            1, -1, -1)


def _set_halo(mp, bm=None):
    mp.setenv("TFOS_CONV3X3_TILE", "halo")
    if bm is None:
        mp.delenv("TFOS_CONV3X3_HALO_BM", raising=False)
    else:
        mp.setenv("TFOS_CONV3X3_HALO_BM", str(bm))


def test_halo_exact_probe_premise_cpu():
    """sum |a||b| < 2^24 for every exact case, and the fp32 CPU result equals
    the fp64 one bit for bit."""
    for c in HALO_EXACT + [TOO_WIDE]:
        x, wk, _ = _conv_args(c)
        s64, abs_sum = _conv_refs(c)
        assert abs_sum.max().item() < EXACT_LIMIT, c["name"]
        assert (s64.abs() <= abs_sum).all(), c["name"]
        s32 = _conv_contract(c, x, wk, FP32)
        assert s32.dtype == FP32 and s64.dtype == FP64
        assert torch.equal(s32.contiguous().view(torch.int32),
                           s64.float().contiguous().view(torch.int32)), \
            c["name"]


@gpu
@requires_gpu
@pytest.mark.parametrize("bm", [512, 256])
@pytest.mark.parametrize("c", HALO_EXACT, ids=lambda c: c["name"])
def test_halo_exact(c, bm, monkeypatch):
    """Bit-exact under both tile heights, and the same bits as im2col."""
    _set_halo(monkeypatch, bm)
    plan = _plan(c)
    assert plan["max_w"] == MAX_W
    assert plan["kernel"] == "halo" and plan["BN"] == 64
    # the span of a 512-pixel tile fits up to W = 95
    assert plan["BM"] == (bm if c["W"] <= 95 else 256)
    M = c["N"] * c["H"] * c["W"]
    assert plan["tiles"] == -(-M // plan["BM"]) * -(-c["Cout"] // 64)
    if "grid" in c["name"]:
        assert plan["grid"] == {256: 19, 512: 10}[bm]
    x, wk, _ = _conv_args(c)
    S64, _ = _conv_refs(c)
    _assert_padding_visible(c, x, wk, S64)
    got = _run(c, x, wk)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _assert_bits("conv_mfma halo", got, _to_bf16(S64))
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "im2col")
    assert _plan(c)["kernel"] == "im2col"
    _assert_bits("halo vs im2col", got, _run(c, x, wk).cpu())


@gpu
@requires_gpu
def test_halo_too_wide_falls_back_exact(monkeypatch):
    """One column past the LDS limit the plan says im2col, and the result is
    still exact."""
    _set_halo(monkeypatch)
    c = TOO_WIDE
    assert _plan(c)["kernel"] == "im2col"
    x, wk, _ = _conv_args(c)
    _assert_bits("conv_mfma too wide", _run(c, x, wk),
                 _to_bf16(_conv_refs(c)[0]))


@gpu
@requires_gpu
def test_halo_persistent_second_tile(monkeypatch):
    """A workgroup that takes more than one tile (M just above BM x grid)."""
    _set_halo(monkeypatch)
    c = _halo_case("persistent", 8, 32, 96, 96, 64)
    plan = _plan(c)
    assert plan["kernel"] == "halo"
    if plan["grid"] == plan["tiles"]:
        pytest.skip("the halo kernel is not persistent: one workgroup per "
                    "tile, overlap comes from two resident workgroups per CU")
    x, wk, _ = _conv_args(c)
    _assert_bits("conv_mfma halo", _run(c, x, wk), _to_bf16(_conv_refs(c)[0]))


@gpu
@requires_gpu
@pytest.mark.parametrize("bm", [512, 256])
@pytest.mark.parametrize("c", HALO_REAL, ids=lambda c: c["name"])
def test_halo_real(c, bm, monkeypatch):
    """Real-valued inputs, the derived bound of test_gpu_mfma."""
    _set_halo(monkeypatch, bm)
    assert _plan(c)["kernel"] == "halo" and _plan(c)["BM"] == bm
    x, wk, _ = _conv_args(c, True)
    S64, absprod = _conv_refs(c, True)
    _assert_bound("conv_mfma halo", _run(c, x, wk), S64, absprod,
                  9 * c["Cin"], BF16)


@gpu
@requires_gpu
def test_halo_conv3x3_module_wiring(monkeypatch):
    """Conv3x3(64, 64) forward and backward at 4x64x16x16 under halo: y and dx
    (the flipped pack through the same kernel) and dw within the derived bound
    of fp64, as test_module_wiring does."""
    from tensorflowonspark_amd.ops import modules
    for k in ("TFOS_CONV1X1", "TFOS_CONV3X3", "TFOS_CONVT", "TFOS_STEM",
              "TFOS_ALLOW_EAGER_FALLBACK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TFOS_WRW", "mfma2")
    _set_halo(monkeypatch)
    N, C, H, W = 4, 64, 16, 16
    assert _ext().conv3x3_halo_plan(N, H, W, C, C)["kernel"] == "halo"
    g = _gen("halo-wiring")
    m = modules.Conv3x3(C, C, stride=1).cuda()
    w64 = _set_real_weight(m.weight, g).cuda()
    x = _real(g, C, N, H, W).permute(1, 0, 2, 3)
    xg = _cl(x.cuda()).requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == "_Conv3x3FnBackward"
    dy = _real(g, C, N, H, W).permute(1, 0, 2, 3)
    dyg = _cl(dy.cuda())
    y.backward(dyg)
    fn = lambda a, b: _conv_ref(a, _w4_to_wk(b), 3, 3, 1, 1, 1, H, W)
    x64, dy64 = xg.detach().double(), dyg.double()
    y64, dx64, dw64 = _grads64(fn, x64, w64, dy64)
    ya, dxa, dwa = _grads64(fn, x64.abs(), w64.abs(), dy64.abs())
    _assert_bound("halo y", y, y64, ya, 9 * C, BF16)
    _assert_bound("halo dx", xg.grad, dx64, dxa, 9 * C, BF16)
    _assert_bound("halo dw", m.weight.grad, dw64, dwa, N * H * W, FP32)


def _block_ref64(blk, x, dy):
    """The Bottleneck in fp64 from plain ops on the CPU: conv weights as the
    kernels see them (rounded to bf16), BatchNorm on batch statistics.
    Returns y, dx and the parameter gradients by name."""
    P = {n: (p.detach().to(BF16) if p.dim() == 4 else p.detach())
         .double().cpu().requires_grad_(True)
         for n, p in blk.named_parameters()}

    def bn(t, name, eps):
        m = t.mean((0, 2, 3), keepdim=True)
        v = t.var((0, 2, 3), unbiased=False, keepdim=True)
        return (t - m) * torch.rsqrt(v + eps) \
            * P[name + ".weight"].view(1, -1, 1, 1) \
            + P[name + ".bias"].view(1, -1, 1, 1)

    eps = blk.bnrelu1.eps
    x64 = x.detach().double().cpu().requires_grad_(True)
    o = F.relu(bn(F.conv2d(x64, P["conv1.weight"]), "bnrelu1", eps))
    o = F.relu(bn(F.conv2d(o, P["conv2.weight"], padding=1), "bnrelu2", eps))
    o = bn(F.conv2d(o, P["conv3.weight"]), "bn3", eps)
    idn = bn(F.conv2d(x64, P["downsample.0.weight"]), "downsample.1", eps)
    y = F.relu(o + idn)
    y.backward(dy.double().cpu())
    return y.detach(), x64.grad, {n: p.grad for n, p in P.items()}


@gpu
@requires_gpu
def test_halo_bottleneck_wiring(monkeypatch):
    """The fused stride-1 Bottleneck (64 -> 64 -> 256, the block of
    test_gpu_bn_dual.py) forward + backward at 4x64x16x16: under
    TFOS_CONV3X3_TILE=halo its conv2 forward and conv2 dgrad are the two 3x3
    conv_mfma calls and both plan to halo.

    Against fp64 (plain ops, bf16-rounded conv weights): y, dx and every
    parameter gradient within rel L2 0.1, the tolerance the block-level tests
    of test_gpu_bn_epilogue.py / test_gpu_bn_dual.py use between two routings
    of this block.

    Against im2col, with two im2col runs (which differ from each other at
    times: the BatchNorm reductions use float atomics).  The two kernels
    differ in the order of one fp32 sum per output before a single rounding
    to bf16, so a conv2 output moves by at most one bf16 ulp, 2^-8 relative.
    The forward maps behind it (BatchNorm with a batch deviation of order 1,
    1x1 convs, ReLU) are continuous, so y may be farther from the nearer
    im2col run than the two are from each other by 2^-8 in rel L2 at the
    most.  The backward is not continuous in that perturbation: a ReLU gate
    whose pre-activation moves across 0 switches a whole gradient path (two
    im2col runs were seen 8.6e-3 apart in dx from that alone), so gradients
    are held to the rel L2 0.1 that the existing block tests allow between
    two routings."""
    for k in ("TFOS_BN_EPI", "TFOS_BN_DUAL", "TFOS_FUSED_BLOCK", "TFOS_WRW",
              "TFOS_CONV3X3", "TFOS_CONV1X1", "TFOS_PACK_PLAN"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("TFOS_CONV3X3_HALO_BM", raising=False)
    ext = _ext()
    blk = _make_block(1, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(4, 64, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    dy = torch.randn(4, 256, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)

    def run(mode):
        monkeypatch.setenv("TFOS_CONV3X3_TILE", mode)
        b = copy.deepcopy(blk)
        calls = []
        orig = ext.conv_mfma

        def rec(*a, **kw):
            if a[3] == 3:
                xs = a[0].shape
                calls.append(ext.conv3x3_halo_plan(
                    xs[0], xs[2], xs[3], xs[1], a[2], a[3], a[4], a[5], a[6],
                    a[7], a[8], a[9])["kernel"])
            return orig(*a, **kw)

        monkeypatch.setattr(ext, "conv_mfma", rec)
        xg = x.clone().requires_grad_(True)
        y = b(xg)
        assert type(y.grad_fn).__name__ == "_BottleneckFnBackward"
        y.backward(dy)
        torch.cuda.synchronize()
        monkeypatch.setattr(ext, "conv_mfma", orig)
        out = {"y": y.detach(), "dx": xg.grad}
        out.update({"grad " + n: p.grad for n, p in b.named_parameters()})
        return out, calls

    a, ca = run("im2col")
    b2, _ = run("im2col")
    h, ch = run("halo")
    assert ca == ["im2col", "im2col"], ca
    assert ch == ["halo", "halo"], ch       # conv2 forward, conv2 dgrad
    y64, dx64, g64 = _block_ref64(blk, x, dy)
    ref = {"y": y64, "dx": dx64}
    ref.update({"grad " + n: g for n, g in g64.items()})
    assert set(ref) == set(h)
    bad = []
    for what in sorted(h):
        assert torch.isfinite(h[what]).all(), what
        r64 = _rel_l2(h[what].cpu(), ref[what])
        r_im = _rel_l2(a[what].cpu(), ref[what])
        pair = _rel_l2(b2[what], a[what])
        cross = min(_rel_l2(h[what], a[what]), _rel_l2(h[what], b2[what]))
        print("  {:<28s} rel L2 vs fp64: halo {:.3e} im2col {:.3e} | halo vs "
              "nearer im2col {:.3e}, im2col vs im2col {:.3e}".format(
                  what, r64, r_im, cross, pair))
        if r64 > 0.1:
            bad.append("{}: rel L2 {:.3e} against fp64".format(what, r64))
        if cross > (pair + 2.0 ** -8 if what == "y" else 0.1):
            bad.append("{}: halo vs im2col {:.3e}, im2col pair {:.3e}".format(
                what, cross, pair))
    assert not bad, bad


@gpu
@requires_gpu
def test_halo_bm_knob(monkeypatch):
    """TFOS_CONV3X3_HALO_BM is read under halo only, and a value other than
    256 or 512 is an error there."""
    ext = _ext()
    args = (64, 56, 56, 64, 64)
    monkeypatch.setenv("TFOS_CONV3X3_HALO_BM", "256")
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "auto")
    p = ext.conv3x3_halo_plan(*args)
    assert (p["kernel"], p["BM"]) == ("halo", 512)
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "halo")
    assert ext.conv3x3_halo_plan(*args)["BM"] == 256
    monkeypatch.setenv("TFOS_CONV3X3_HALO_BM", "384")
    with pytest.raises(RuntimeError):
        ext.conv3x3_halo_plan(*args)
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "auto")
    assert ext.conv3x3_halo_plan(*args)["BM"] == 512
    # below the class's minimum M auto stays on im2col
    assert ext.conv3x3_halo_plan(8, 56, 56, 64, 64)["kernel"] == "im2col"


@gpu
@requires_gpu
def test_halo_dispatch(monkeypatch):
    """auto keeps every small 3x3 stride-1 launch of the pinned suites on the
    im2col kernel; halo takes eligible launches only; a bad value raises."""
    ext = _ext()
    monkeypatch.delenv("TFOS_CONV3X3_HALO_BM", raising=False)
    small = [c for c in CONV_EXACT + CONV_REAL
             if (c["fh"], c["fw"], c["S"], c["D"]) == (3, 3, 1, 1)]
    assert small
    # the calltrace cases: Conv3x3 64 -> 96 and its dgrad, the blocks' 64 -> 64
    trace = [(2, 16, 16, 64, 96), (2, 16, 16, 96, 64), (4, 16, 16, 64, 64)]
    for mode in (None, "auto"):
        if mode is None:
            monkeypatch.delenv("TFOS_CONV3X3_TILE", raising=False)
        else:
            monkeypatch.setenv("TFOS_CONV3X3_TILE", mode)
        for c in small:
            assert _plan(c, P=c["P"])["kernel"] == "im2col", c["name"]
        for t in trace:
            assert ext.conv3x3_halo_plan(*t)["kernel"] == "im2col", t
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "halo")
    args = (4, 16, 16, 64, 64)
    assert ext.conv3x3_halo_plan(*args)["kernel"] == "halo"
    for kw in (dict(S=2), dict(fd=2, P=2), dict(D=2), dict(out_f32=True),
               dict(OH=17, OW=17), dict(P=0), dict(fh=1, fw=1, P=0)):
        assert ext.conv3x3_halo_plan(*args, **kw)["kernel"] == "im2col", kw
    monkeypatch.setenv("TFOS_CONV3X3_TILE", "wide")
    with pytest.raises(RuntimeError):
        ext.conv3x3_halo_plan(*args)
    x = torch.ones(1, 32, 4, 4, device="cuda", dtype=BF16) \
        .contiguous(memory_format=torch.channels_last)
    wk = torch.ones(64, 9 * 32, device="cuda", dtype=BF16)
    with pytest.raises(RuntimeError):
        ext.conv_mfma(x, wk, 64, 3, 3, 1, 1, 1, -1, -1)
