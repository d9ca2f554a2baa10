"""BatchNorm batch statistics from the GEMM / conv epilogues
(``gemm_bt_stats`` / ``conv_mfma_stats`` -> ``bn_fwd_train_pre`` /
``bn_dual_fwd_train_pre``; csrc/mfma_stats_epilogue.h and the tile merge in
csrc/bn_relu.hip) vs the plain kernels and a plain fp64 reference.

The STATS kernels must store exactly what the plain kernels store (bit-equal,
which pins their output through tests/test_gpu_mfma.py), and the statistics
merged from their tile partials must be the fp64 statistics of that bf16
tensor within the bound of tests/test_gpu_bn.py,

    bound(q) = 16 * max|ref32(q) - ref64(q)| + half_ulp(dtype) * |ref64(q)|

derived from the reference alone. Inputs: bf16 A[M, K], B[N, K] with
A[:, K-1] = 1 and B[c, K-1] = mu_c, so that every output channel has its own
mean (|mean| / sigma <= 8, sigma from 0.5 to 2, as in test_gpu_bn.py); one
channel has all other weights zero, so its output is constant and var = 0.
For the convs the ones column is input channel Cin-1 and mu_c sits on the
centre tap, which no padding cuts off. M is ragged against the 128- and
256-row tiles: the kernels clamp the source rows past M, so an unmasked tail
row is a duplicate of a real row and, through the ones column, shifts the mean
visibly.

Block level: the fused Bottleneck under TFOS_BN_EPI=force reaches the _pre
entries and agrees with TFOS_BN_EPI=off at the level the dual block test uses;
under the default auto the small test tensors stay on the existing entries
and a 51 MB join (the smallest size auto routes) takes the dual _pre entry. A
block whose widths are off the NHWC fast path (96, 384) keeps the existing
entries and the plain conv kernels even under force.
"""

import copy

import pytest
import torch

from test_gpu_bn import (BF16, EPS, FP32, NHWC, _bits_equal, _bn_ref, _bound,
                         _check, _ext, _memory_order, _per_channel, gpu,
                         requires_gpu)
from test_gpu_bn_dual import _make_block, _rel_l2

CONST = 5          # the constant channel


def _channel_params(C, seed):
    gen = torch.Generator().manual_seed(seed)
    w = _per_channel(C, 0.5, 2.0, gen)
    w[torch.arange(C, device="cuda") % 5 == 3] *= -1.0
    return {"mu": _per_channel(C, -4.0, 4.0, gen),
            "sigma": _per_channel(C, 0.5, 2.0, gen), "w": w,
            "b": _per_channel(C, -1.0, 1.0, gen),
            "rm0": _per_channel(C, -2.0, 2.0, gen),
            "rv0": _per_channel(C, 0.5, 3.0, gen)}


def _gemm_inputs(M, N, K, seed):
    """A[M, K], B[N, K] bf16 and the per-channel vectors."""
    p = _channel_params(N, seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=gen)
    b = torch.randn(N, K, device="cuda", generator=gen) \
        * (p["sigma"] / max(K - 1, 1) ** 0.5)[:, None]
    b[CONST] = 0
    a[:, K - 1] = 1
    b[:, K - 1] = p["mu"]
    return a.to(BF16), b.to(BF16), p


def _conv_inputs(Cin, Cout, k, seed, n=3, hw=7):
    """x[n, Cin, hw, hw] channels_last, wk[Cout, k*k*Cin] bf16."""
    p = _channel_params(Cout, seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, Cin, hw, hw, device="cuda", generator=gen)
    x[:, Cin - 1] = 1
    w = torch.randn(Cout, k * k, Cin, device="cuda", generator=gen) \
        * (p["sigma"] / (k * k * (Cin - 1)) ** 0.5)[:, None, None]
    w[CONST] = 0
    w[:, :, Cin - 1] = 0
    w[:, (k * k) // 2, Cin - 1] = p["mu"]          # centre tap
    x = x.to(BF16).contiguous(memory_format=torch.channels_last)
    return x, w.reshape(Cout, k * k * Cin).to(BF16), p


def _as4d(t2d):
    """[M, C] row-major as a channels_last (1, C, M, 1) tensor."""
    M, C = t2d.shape
    t = t2d.view(1, M, 1, C).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t


def _check_pre(t, part, rows, p, relu=True, res=None, momentum=0.1):
    """bn_fwd_train_pre on (t, part) vs the fp64 statistics and forward of the
    bf16 tensor t itself."""
    ext = _ext()
    C = t.shape[1]
    M = t.numel() // C
    assert part.dtype == FP32 and part.is_contiguous()
    assert tuple(part.shape) == ((M + rows - 1) // rows, 2, C)
    rm, rv = p["rm0"].clone(), p["rv0"].clone()
    y, mean, rstd, mask = ext.bn_fwd_train_pre(t, res, part, rows, p["w"],
                                               p["b"], rm, rv, momentum, EPS,
                                               relu)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and y.stride() == t.stride()
    kw = dict(x=t, w=p["w"], b=p["b"], res=res, relu=relu, rm0=p["rm0"],
              rv0=p["rv0"], momentum=momentum)
    r64, r32 = _bn_ref(torch.float64, **kw), _bn_ref(torch.float32, **kw)
    # the inputs are what the docstring says: distinct means, one var == 0
    assert r64["var"][CONST] == 0 and (r64["var"] > 0).sum() == C - 1
    keep = torch.arange(C, device="cuda") != CONST
    _check("save_mean", mean, r64["mean"], r32["mean"], FP32)
    _check("save_rstd", rstd, r64["rstd"], r32["rstd"], FP32, keep)
    _check("running_mean", rm, r64["running_mean"], r32["running_mean"], FP32)
    _check("running_var", rv, r64["running_var"], r32["running_var"], FP32)
    assert not torch.equal(rm, p["rm0"]) and not torch.equal(rv, p["rv0"])
    assert torch.isfinite(rstd).all()
    assert rstd[CONST].item() <= EPS ** -0.5 * (1 + 2.0 ** -20)
    _check("y", y, r64["y"], r32["y"], BF16)
    # constant channel: y = b (+ res)(relu) there
    expect = torch.full_like(r64["y"][:, CONST], float(p["b"][CONST]))
    if res is not None:
        expect = expect + res[:, CONST].double()
    if relu:
        expect = expect.clamp_min(0)
    tol = _bound(r64["y"], r32["y"], BF16)[:, CONST]
    assert ((y[:, CONST].double() - expect).abs() <= tol).all(), \
        "constant channel y"
    if relu:
        assert mask.dtype == torch.uint8 and mask.numel() == t.numel() // 8
        bits = (mask.to(torch.int32)[:, None]
                >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1
        assert torch.equal(bits.reshape(-1).bool(),
                           _memory_order(y, NHWC) > 0), "bitmask != (y > 0)"
        disagree = (y > 0) != (r64["pre"] > 0)
        frac = disagree.double().mean().item()
        print("  gate disagreements with fp64: {} ({:.4%})".format(
            int(disagree.sum()), frac))
        ytol = _bound(r64["y"], r32["y"], BF16)
        assert (r64["pre"].abs()[disagree] <= ytol[disagree]).all(), \
            "gate differs from fp64 away from 0"
        assert frac <= 1e-3
    else:
        assert mask.numel() == 0
    return y, mean, rstd, mask


GEMM_SHAPES = [
    pytest.param(421, 128, 64, 128, id="421x128x64-tile128"),
    pytest.param(421, 64, 32, 256, id="421x64x32-tile256x64-one-kstep"),
    pytest.param(147, 256, 64, 128, id="147x256x64-two-ntiles"),
    pytest.param(1100, 256, 1024, None, id="1100x256x1024-route256"),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("M,N,K,rows_expected", GEMM_SHAPES)
def test_gemm_stats(M, N, K, rows_expected):
    ext = _ext()
    a, b, p = _gemm_inputs(M, N, K, seed=3)
    print("\ngemm_bt_stats {}x{}x{}".format(M, N, K))
    c, part, rows = ext.gemm_bt_stats(a, b)
    assert _bits_equal(c, ext.gemm_bt(a, b, True)), "stored tile changed"
    if rows_expected is None and part is None:
        assert rows == 0
        return
    if rows_expected is not None:
        assert part is not None and rows == rows_expected
    _check_pre(_as4d(c), part, rows, p)
    # determinism: same partials, same outputs, bit for bit
    c2, part2, rows2 = ext.gemm_bt_stats(a, b)
    assert rows2 == rows and torch.equal(part, part2) and _bits_equal(c, c2)


CONV_CASES = [
    pytest.param(32, 64, 3, 1, 7, id="3x3s1-32to64"),
    pytest.param(64, 256, 3, 1, 7, id="3x3s1-64to256"),
    pytest.param(64, 64, 3, 2, 7, id="3x3s2-64to64"),
    pytest.param(32, 256, 3, 2, 7, id="3x3s2-32to256"),
    pytest.param(64, 256, 1, 2, 7, id="1x1s2-64to256"),
    pytest.param(32, 64, 1, 2, 7, id="1x1s2-32to64"),
    # M = 3 * 11 * 11 = 363: a second, ragged M tile on each conv tile shape
    pytest.param(32, 64, 3, 1, 11, id="3x3s1-32to64-two-mtiles"),
    pytest.param(32, 256, 3, 1, 11, id="3x3s1-32to256-two-mtiles"),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("Cin,Cout,k,stride,hw", CONV_CASES)
def test_conv_stats(Cin, Cout, k, stride, hw):
    ext = _ext()
    x, wk, p = _conv_inputs(Cin, Cout, k, seed=4, hw=hw)
    args = (x, wk, Cout, k, k, stride, k // 2, 1, -1, -1)
    print("\nconv_mfma_stats {}->{} k{} s{} @{}".format(Cin, Cout, k, stride,
                                                        hw))
    y, part, rows = ext.conv_mfma_stats(*args)
    assert _bits_equal(y, ext.conv_mfma(*args)), "stored tile changed"
    oh = (hw - 1) // stride + 1
    assert tuple(y.shape) == (3, Cout, oh, oh)
    assert part is not None and rows == 256
    assert part.shape[0] == (3 * oh * oh + 255) // 256
    _check_pre(y, part, rows, p)
    y2, part2, _ = ext.conv_mfma_stats(*args)
    assert torch.equal(part, part2) and _bits_equal(y, y2)


@gpu
@requires_gpu
def test_conv_stats_none_without_epilogue():
    """Input dilation 2 and fp32 output have no epilogue: plain result."""
    ext = _ext()
    x, wk, _ = _conv_inputs(32, 64, 3, seed=4)
    for kw, args in (({}, (x, wk, 64, 3, 3, 1, 1, 2, 13, 13)),
                     ({"out_f32": True}, (x, wk, 64, 3, 3, 1, 1, 1, -1, -1))):
        y, part, rows = ext.conv_mfma_stats(*args, **kw)
        assert part is None and rows == 0
        assert torch.equal(y, ext.conv_mfma(*args, **kw))


@gpu
@requires_gpu
@pytest.mark.parametrize("relu,add", [(True, True), (False, False)],
                         ids=["relu-res", "plain"])
def test_pre_forward_variants(relu, add):
    """The apply variants behind bn_fwd_train_pre: residual + ReLU, and none."""
    ext = _ext()
    a, b, p = _gemm_inputs(421, 128, 64, seed=8)
    c, part, rows = ext.gemm_bt_stats(a, b)
    t = _as4d(c)
    gen = torch.Generator(device="cuda").manual_seed(9)
    res = None
    if add:
        res = torch.randn(t.shape, device="cuda", generator=gen).to(BF16) \
            .contiguous(memory_format=torch.channels_last)
    out1 = _check_pre(t, part, rows, p, relu=relu, res=res, momentum=0.3)
    out2 = _check_pre(t, part, rows, p, relu=relu, res=res, momentum=0.3)
    for u, v in zip(out1, out2):
        assert torch.equal(u, v), "two runs on the same partials differ"


@gpu
@requires_gpu
@pytest.mark.parametrize("which", ["both", "a", "b"])
def test_dual_pre(which):
    """bn_dual_fwd_train_pre vs the chained fp64 reference of
    test_gpu_bn_dual.py; a branch passed without partials gets the pass."""
    ext = _ext()
    a1, b1, pa = _gemm_inputs(421, 128, 64, seed=11)
    a2, b2, pb = _gemm_inputs(421, 128, 32, seed=23)
    ca, part_a, rows_a = ext.gemm_bt_stats(a1, b1)
    cb, part_b, rows_b = ext.gemm_bt_stats(a2, b2)
    xa, xb = _as4d(ca), _as4d(cb)
    if which == "a":
        part_b, rows_b = None, 0
    if which == "b":
        part_a, rows_a = None, 0
    rma, rva = pa["rm0"].clone(), pa["rv0"].clone()
    rmb, rvb = pb["rm0"].clone(), pb["rv0"].clone()
    print("\ndual pre, partials for {}".format(which))
    outs = [ext.bn_dual_fwd_train_pre(
        xa, xb, part_a, rows_a, part_b, rows_b, pa["w"], pa["b"],
        rma if i == 0 else pa["rm0"].clone(),
        rva if i == 0 else pa["rv0"].clone(), pb["w"], pb["b"],
        rmb if i == 0 else pb["rm0"].clone(),
        rvb if i == 0 else pb["rv0"].clone(), 0.1, EPS) for i in range(2)]
    y, mean_a, rstd_a, mean_b, rstd_b, mask = outs[0]
    torch.cuda.synchronize()
    ref = {}
    for dt in (torch.float64, torch.float32):
        rb = _bn_ref(dt, xb, pb["w"], pb["b"], rm0=pb["rm0"], rv0=pb["rv0"])
        ra = _bn_ref(dt, xa, pa["w"], pa["b"], res=rb["pre"], relu=True,
                     rm0=pa["rm0"], rv0=pa["rv0"])
        ref[dt] = (ra, rb)
    (a64, b64), (a32, b32) = ref[torch.float64], ref[torch.float32]
    keep = torch.arange(128, device="cuda") != CONST
    _check("y", y, a64["y"], a32["y"], BF16)
    _check("mean_a", mean_a, a64["mean"], a32["mean"], FP32)
    _check("mean_b", mean_b, b64["mean"], b32["mean"], FP32)
    _check("rstd_a", rstd_a, a64["rstd"], a32["rstd"], FP32, keep)
    _check("rstd_b", rstd_b, b64["rstd"], b32["rstd"], FP32, keep)
    for what, got, r64, r32 in (
            ("running_mean", rma, a64, a32), ("running_var", rva, a64, a32),
            ("running_mean", rmb, b64, b32), ("running_var", rvb, b64, b32)):
        _check(what, got, r64[what], r32[what], FP32)
    assert torch.isfinite(rstd_a).all() and torch.isfinite(rstd_b).all()
    bits = (mask.to(torch.int32)[:, None]
            >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1
    assert torch.equal(bits.reshape(-1).bool(),
                       _memory_order(y, NHWC) > 0), "bitmask != (y > 0)"
    disagree = (y > 0) != (a64["pre"] > 0)
    ytol = _bound(a64["y"], a32["y"], BF16)
    assert (a64["pre"].abs()[disagree] <= ytol[disagree]).all()
    assert disagree.double().mean().item() <= 1e-3
    if which == "both":      # no atomics on this route: reproducible
        for u, v in zip(outs[0], outs[1]):
            assert torch.equal(u, v)


# ---------------------------------------------------------------------------
# block level: _BottleneckFn under TFOS_BN_EPI
# ---------------------------------------------------------------------------

def _run_block(blk, x, dy, monkeypatch, epi, dual="on"):
    if epi is None:
        monkeypatch.delenv("TFOS_BN_EPI", raising=False)
    else:
        monkeypatch.setenv("TFOS_BN_EPI", epi)
    monkeypatch.setenv("TFOS_BN_DUAL", dual)
    ext = _ext()
    calls = {"bn_fwd_train_pre": 0, "bn_dual_fwd_train_pre": 0}
    orig = {n: getattr(ext, n) for n in calls}

    def wrap(name):
        def f(*a):
            calls[name] += 1
            return orig[name](*a)
        return f

    for n in calls:
        monkeypatch.setattr(ext, n, wrap(n))
    x = x.clone().requires_grad_(True)
    y = blk(x)
    y.backward(dy)
    torch.cuda.synchronize()
    for n in calls:
        monkeypatch.setattr(ext, n, orig[n])
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    bufs = {n: b.clone() for n, b in blk.named_buffers()}
    return y.detach(), x.grad.clone(), grads, bufs, calls


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [2, 1])
def test_bottleneck_epilogue_routes(stride, monkeypatch):
    blk = _make_block(stride, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(4, 64, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    oh = 16 // stride
    dy = torch.randn(4, 256, oh, oh, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    before = dict(blk.named_buffers())

    def run(epi, dual="on"):
        return _run_block(copy.deepcopy(blk), x, dy, monkeypatch, epi, dual)

    y0, dx0, g0, b0, c0 = run("off")
    assert c0 == {"bn_fwd_train_pre": 0, "bn_dual_fwd_train_pre": 0}, \
        "TFOS_BN_EPI=off reached the _pre entries"
    _ya, _dxa, _ga, _ba, ca = run(None)
    assert ca == {"bn_fwd_train_pre": 0, "bn_dual_fwd_train_pre": 0}, \
        "default auto routed a 0.5 MB tensor to the epilogue"
    for dual, expect in (("on", {"bn_fwd_train_pre": 2,
                                 "bn_dual_fwd_train_pre": 1}),
                         ("off", {"bn_fwd_train_pre": 4,
                                  "bn_dual_fwd_train_pre": 0})):
        y1, dx1, g1, b1, c1 = run("force", dual)
        assert c1 == expect, "force, dual {}: {}".format(dual, c1)
        yr, dxr, gr, br, _ = (y0, dx0, g0, b0, c0) if dual == "on" \
            else run("off", dual)
        assert set(g1) == set(gr)
        for what, u, v in [("dx", dx1, dxr), ("y", y1, yr)] + \
                [("grad " + n, g1[n], gr[n]) for n in sorted(gr)]:
            assert torch.isfinite(u).all()
            rel = _rel_l2(u, v)
            print("  dual {} {:<28s} rel L2 {:.3e}".format(dual, what, rel))
            assert rel <= 0.1, "{}: rel L2 {:.3e}".format(what, rel)
        moved = 0
        for n, v in br.items():
            if not v.is_floating_point():
                assert torch.equal(b1[n], v)
                continue
            scale = v.abs().max().item()
            e = (b1[n] - v).abs().max().item()
            print("  dual {} {:<28s} max diff {:.3e}  scale {:.3e}".format(
                dual, n, e, scale))
            assert e <= 2.0 ** -14 * scale, "buffer {} differs".format(n)
            assert not torch.equal(b1[n], before[n]), n + " not updated"
            moved += 1
        assert moved == 8       # running mean and var of the four BNs


def _make_block_w(cin, width, stride, seed):
    """_make_block of test_gpu_bn_dual.py at another width."""
    from tensorflowonspark_amd.models.resnet import Bottleneck, conv1x1
    from tensorflowonspark_amd.ops.modules import FusedBN
    torch.manual_seed(seed)
    down = torch.nn.Sequential(conv1x1(cin, 4 * width, stride),
                               FusedBN(4 * width))
    blk = Bottleneck(cin, width, stride, down).cuda().to(
        memory_format=torch.channels_last)
    blk.train()
    assert blk._block_fusable
    return blk


def _count_entries(blk, x, monkeypatch, names):
    """Forward + backward of blk with the named extension entries counted."""
    ext = _ext()
    calls = {n: 0 for n in names}
    orig = {n: getattr(ext, n) for n in names}

    def wrap(name):
        def f(*a):
            calls[name] += 1
            return orig[name](*a)
        return f

    for n in names:
        monkeypatch.setattr(ext, n, wrap(n))
    x = x.clone().requires_grad_(True)
    y = blk(x)
    y.float().sum().backward()
    torch.cuda.synchronize()
    for n in names:
        monkeypatch.setattr(ext, n, orig[n])
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    return calls


ENTRIES = ("bn_fwd_train", "bn_dual_fwd_train", "bn_fwd_train_pre",
           "bn_dual_fwd_train_pre", "gemm_bt_stats", "conv_mfma_stats")


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_bottleneck_ineligible_width_keeps_existing_entries(stride,
                                                            monkeypatch):
    """Width 96 (C = 96 and 384: neither divides 2048) is off the NHWC fast
    path, which the _pre entries require: even under force the block stays on
    bn_fwd_train and its generic kernels, as before, and the convs on the
    plain kernels (no partials that nobody could use)."""
    ext = _ext()
    assert ext.bn_fast_blocks(4 * 16 * 16 * 96, 96, True, True) == 0
    blk = _make_block_w(96, 96, stride, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(4, 96, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    monkeypatch.setenv("TFOS_BN_DUAL", "on")
    monkeypatch.setenv("TFOS_BN_EPI", "off")
    ref = _count_entries(copy.deepcopy(blk), x, monkeypatch, ENTRIES)
    assert ref["bn_fwd_train"] == 4 and ref["bn_dual_fwd_train"] == 0
    monkeypatch.setenv("TFOS_BN_EPI", "force")
    got = _count_entries(copy.deepcopy(blk), x, monkeypatch, ENTRIES)
    assert got == ref, "force changed the calls of an ineligible block"
    assert got["bn_fwd_train_pre"] == got["bn_dual_fwd_train_pre"] == 0
    assert got["gemm_bt_stats"] == got["conv_mfma_stats"] == 0


@gpu
@requires_gpu
def test_bottleneck_auto_routes_a_large_tensor(monkeypatch):
    """The default route on a tensor of the size auto was measured at:
    x = 32 x 64 x 56 x 56 makes t3 and td 32 x 256 x 56 x 56 bf16 = 51.4 MB,
    the smallest size routed, both on gemm_bt, so the join takes
    bn_dual_fwd_train_pre; t1 and t2 (64 channels, 12.8 MB) stay below it."""
    from tensorflowonspark_amd.ops import modules
    assert 32 * 56 * 56 * 256 * 2 == modules._BN_EPI_MIN_BYTES
    blk = _make_block(1, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(32, 64, 56, 56, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    monkeypatch.setenv("TFOS_BN_DUAL", "on")
    monkeypatch.delenv("TFOS_BN_EPI", raising=False)
    got = _count_entries(blk, x, monkeypatch, ENTRIES)
    assert got == {"bn_fwd_train": 2, "bn_dual_fwd_train": 0,
                   "bn_fwd_train_pre": 0, "bn_dual_fwd_train_pre": 1,
                   "gemm_bt_stats": 2, "conv_mfma_stats": 0}, got


def test_auto_rule_keeps_small_tensors():
    from tensorflowonspark_amd.ops import modules
    # the block test's largest conv output: 4 x 256 x 16 x 16 bf16 = 0.5 MB
    for kind, M, K, cout in (("gemm", 1024, 64, 64), ("gemm", 1024, 64, 256),
                             ("conv", 1024, 576, 64), ("conv", 256, 64, 256)):
        assert not modules._bn_epi_route("auto", kind, M, K, cout)
        assert modules._bn_epi_route("force", kind, M, K, cout)
        assert not modules._bn_epi_route("off", kind, M, K, cout)
    assert modules._BN_EPI_MIN_BYTES >= 12 << 20


@gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    ext = _ext()
    a, b, p = _gemm_inputs(421, 128, 64, seed=3)
    c, part, rows = ext.gemm_bt_stats(a, b)
    t = _as4d(c)
    v = [p["w"], p["b"], p["rm0"].clone(), p["rv0"].clone()]

    def pre(t_, part_, rows_):
        return ext.bn_fwd_train_pre(t_, None, part_, rows_, *v, 0.1, EPS, True)

    pre(t, part, rows)                                   # the good call
    bad = [
        (t, part.double(), rows),                        # dtype
        (t, part.cpu(), rows),                           # device
        (t, part[:-1].contiguous(), rows),               # tile rows
        (t, part[:, :1].contiguous(), rows),             # not [.., 2, ..]
        (t, part[:, :, :64].contiguous(), rows),         # channels
        (t, part.transpose(1, 2), rows),                 # not contiguous
        (t, part, 256),                                  # other tile height
        (t, part, 0),
        (t.cpu(), part, rows),                           # CPU input
        (t.float(), part, rows),                         # fp32 input
        (t.contiguous(), part, rows),                    # NCHW
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            pre(*args)
    with pytest.raises(RuntimeError):
        ext.bn_dual_fwd_train_pre(t, t.clone(), part.double(), rows, part,
                                  rows, *v, *v, 0.1, EPS)
    with pytest.raises(RuntimeError):
        ext.bn_dual_fwd_train_pre(t, t.clone(), part, rows, part[:-1], rows,
                                  *v, *v, 0.1, EPS)
    with pytest.raises(RuntimeError):
        ext.gemm_bt_stats(a.cpu(), b.cpu())
    with pytest.raises(RuntimeError):
        ext.gemm_bt_stats(a, b.cpu())
    with pytest.raises(RuntimeError):
        ext.gemm_bt_stats(a.float(), b.float())
    x, wk, _ = _conv_inputs(32, 64, 3, seed=4)
    with pytest.raises(RuntimeError):
        ext.conv_mfma_stats(x.cpu(), wk.cpu(), 64, 3, 3, 1, 1, 1, -1, -1)
