"""Fused BatchNorm + ReLU + max-pool (csrc/bn_pool.hip) vs fp64 references.

``bn_relu_pool_fwd`` / ``bn_relu_pool_bwd`` are driven directly and compared
with textbook arithmetic in fp64 on the values the kernels see. The error model
is the one of test_gpu_bn.py: for each compared quantity

    bound = 16 * max|ref32 - ref64| + half_ulp(output dtype) at |ref64|

with ref32 / ref64 the same reference run in fp32 / fp64. Nothing is tuned to
what the kernels give.

Forward: p against max(relu(bn(x))) over the window; per window, an index
other than 0xFF names an in-bounds tap within 2 bounds of the window maximum
whose value p has, and 0xFF stands only where the maximum is within the bound
of 0. The statistics are those of ``bn_fwd_train``: bit for bit where those
kernels repeat themselves bit for bit, to their run-to-run freedom elsewhere
(``_same_statistics``). p and the index are those of the BN apply kernel +
``maxpool_fwd`` on the same statistics, bit for bit (the index wherever
p > 0).

Backward: the reference routes dp to the taps the returned index names (the
index is validated by the forward checks), then does the BN backward in fp64.
"""

import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_bn import (BF16, EPS, FP32, _bits_equal, _bn_ref, _bound,
                         _check, _ext, _make_inputs, gpu, requires_gpu)
from test_gpu_stream import _rejects

NO_OWNER = 0xFF

# (shape, (K, S, P), channel whose bias is -50 or None)
CASES = [
    pytest.param((2, 8, 13, 11), (3, 2, 1), None, id="c8-13x11-k3s2p1"),
    pytest.param((2, 64, 13, 11), (3, 2, 1), 5, id="c64-13x11-k3s2p1-dead5"),
    # 2/2/0 on odd sizes: the last row and column belong to no window
    pytest.param((2, 8, 13, 11), (2, 2, 0), None, id="c8-13x11-k2s2p0"),
    pytest.param((2, 64, 13, 11), (2, 2, 0), None, id="c64-13x11-k2s2p0"),
    # one or two adds per LDS address: statistics reproducible bit for bit
    pytest.param((2, 1024, 5, 7), (3, 2, 1), None, id="c1024-5x7-k3s2p1"),
    # the reductions stride over their grid more than once
    pytest.param((3, 64, 114, 114), (3, 2, 1), 9, id="c64-114x114-k3s2p1"),
    # more pooled vectors than 2048 * 256 threads: forward and dx stride too
    pytest.param((6, 64, 232, 232), (3, 2, 1), None, id="c64-232x232-k3s2p1"),
]


def _windows(t, K, S, P, fill):
    """(N, C, OH, OW, K*K) taps of every pooling window, padding = fill."""
    t = F.pad(t, (P, P, P, P), value=fill)
    t = t.unfold(2, K, S).unfold(3, K, S)
    return t.reshape(*t.shape[:4], K * K)


def _route(dp, idx, shape, K, S, P):
    """fp64 gradient at the pool's input: dp added to the tap idx names."""
    N, C, H, W = shape
    OH, OW = dp.shape[2], dp.shape[3]
    dev = dp.device
    own = idx != NO_OWNER
    tap = torch.where(own, idx, torch.zeros_like(idx)).long()
    oh = torch.arange(OH, device=dev)[None, None, :, None]
    ow = torch.arange(OW, device=dev)[None, None, None, :]
    ih = (oh * S - P + tap // K).clamp(0, H - 1)
    iw = (ow * S - P + tap % K).clamp(0, W - 1)
    n = torch.arange(N, device=dev)[:, None, None, None]
    c = torch.arange(C, device=dev)[None, :, None, None]
    flat = ((n * C + c) * H + ih) * W + iw
    out = torch.zeros(N * C * H * W, dtype=torch.float64, device=dev)
    out.index_put_((flat[own],), dp.double()[own], accumulate=True)
    return out.view(N, C, H, W)


def _inputs(shape, ksp, dead, seed=3):
    K, S, P = ksp
    N, C, H, W = shape
    d = _make_inputs(BF16, shape, "nhwc", seed)
    if dead is not None:
        d["b"][dead] = -50.0
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    dp = torch.randn(N, C, OH, OW, device="cuda", generator=gen)
    dp[torch.rand(dp.shape, device="cuda", generator=gen) < 0.2] = 0.0
    d["dp"] = dp.to(BF16).contiguous(memory_format=torch.channels_last)
    return d


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,ksp,dead", CASES)
def test_fused_stem_tail(shape, ksp, dead):
    ext = _ext()
    K, S, P = ksp
    N, C, H, W = shape
    d = _inputs(shape, ksp, dead)
    x, w, b, dp = d["x"], d["w"], d["b"], d["dp"]
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    assert ext.bn_relu_pool_eligible(x, K, S, P)
    p, idx, mean, rstd = ext.bn_relu_pool_fwd(x, w, b, rm, rv, 0.1, EPS,
                                              K, S, P)
    dx, dgamma, dbeta = ext.bn_relu_pool_bwd(x, dp, idx, w, mean, rstd,
                                             K, S, P)
    torch.cuda.synchronize()
    OH, OW = dp.shape[2], dp.shape[3]
    assert p.shape == dp.shape and p.dtype == BF16
    assert p.is_contiguous(memory_format=torch.channels_last)
    assert idx.shape == (N, OH, OW, C) and idx.dtype == torch.uint8
    assert dx.shape == x.shape and dx.dtype == BF16
    assert dx.stride() == x.stride()

    # the statistics of bn_fwd_train on the same input
    rm2, rv2 = d["rm0"].clone(), d["rv0"].clone()
    _, mean2, rstd2, _ = ext.bn_fwd_train(x, None, w, b, rm2, rv2, 0.1, EPS,
                                          True)
    print("\ncase {} {}: max |mean - mean2| {:.3e}, |rstd - rstd2| {:.3e}"
          .format(shape, ksp, (mean - mean2).abs().max().item(),
                  (rstd - rstd2).abs().max().item()))
    _same_statistics(C, (mean, rstd, rm, rv), (mean2, rstd2, rm2, rv2), rstd)
    # the pooled values and the owners of the two-op path, replayed from the
    # fused entry's own statistics: the apply kernel, then maxpool_fwd
    y2 = torch.empty_like(x)
    mask2 = torch.empty(x.numel() // 8, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ext.bn_fast_blocks(x.numel(), C, True, True) * 2 * C,
                     device="cuda")
    ext.bn_stage(1, x, None, y2, mask2, ws, [mean, rstd, w, b], True, None)
    p2, idx2 = ext.maxpool_fwd(y2, K, S, P)
    assert _bits_equal(p, p2), "p differs from bn apply + maxpool_fwd"
    pos = (p2 > 0).permute(0, 2, 3, 1)
    assert torch.equal(idx[pos], idx2[pos])
    assert (idx[~pos] == NO_OWNER).all()
    del y2, p2, idx2

    kw = dict(x=x, w=w, b=b, relu=True, rm0=d["rm0"], rv0=d["rv0"])
    r64 = _bn_ref(torch.float64, **kw)
    r32 = _bn_ref(torch.float32, **kw)
    _check("save_mean", mean, r64["mean"], r32["mean"], FP32)
    _check("save_rstd", rstd, r64["rstd"], r32["rstd"], FP32)
    _check("running_mean", rm, r64["running_mean"], r32["running_mean"], FP32)
    _check("running_var", rv, r64["running_var"], r32["running_var"], FP32)
    # bn_fwd_train's own, within the same bounds: the two runs are then
    # within twice the bound of each other
    _check("save_mean 2", mean2, r64["mean"], r32["mean"], FP32)
    _check("save_rstd 2", rstd2, r64["rstd"], r32["rstd"], FP32)
    _check("running_mean2", rm2, r64["running_mean"], r32["running_mean"],
           FP32)
    _check("running_var 2", rv2, r64["running_var"], r32["running_var"], FP32)

    # forward: p against the window maximum of the reference
    inf = float("inf")
    t64 = _windows(r64["y"], K, S, P, -inf)
    t32 = _windows(r32["y"], K, S, P, -inf)
    max64, max32 = t64.max(-1).values, t32.max(-1).values
    _check("p", p, max64, max32, BF16)

    # per window: the owner, or why there is none
    ref_err = (r32["y"].double() - r64["y"]).abs().max()
    sel = idx.permute(0, 3, 1, 2)
    own = sel != NO_OWNER
    assert (sel[own] < K * K).all(), "tap index outside the window"
    tap = torch.where(own, sel, torch.zeros_like(sel)).long()
    val = t64.gather(-1, tap[..., None])[..., 0]
    assert torch.isfinite(val[own]).all(), "owner is a padding tap"
    tol_max = _bound(max64, max32, BF16)
    assert (val[own] >= (max64 - 2 * tol_max)[own]).all(), \
        "owner is not a maximum of its window"
    tol_val = 16.0 * ref_err + _half_ulp_of(val)
    assert ((p.double() - val).abs()[own] <= tol_val[own]).all(), \
        "p is not its owner's value"
    assert (max64[~own] <= tol_max[~own]).all(), \
        "a window with a positive maximum has no owner"
    print("  windows without owner: {:.2%}".format(
        (~own).double().mean().item()))

    # backward: dp routed by the returned index, BN backward in fp64
    g = _route(dp, sel, shape, K, S, P)
    kb = dict(x=x, w=w, b=b, dy=g, relu=False)
    b64 = _bn_ref(torch.float64, **kb)
    b32 = _bn_ref(torch.float32, **kb)
    _check("dx", dx, b64["dx"], b32["dx"], BF16)
    _check("dgamma", dgamma, b64["dgamma"], b32["dgamma"], FP32)
    _check("dbeta", dbeta, b64["dbeta"], b32["dbeta"], FP32)

    if dead is not None:
        assert not own[:, dead].any(), "a window of the dead channel has an owner"
        assert (p[:, dead] == 0).all()
        assert (dx[:, dead] == 0).all()
        assert dgamma[dead] == 0 and dbeta[dead] == 0


def _same_statistics(C, got, want, rstd):
    """(mean, rstd, running_mean, running_var) of two launches of the same
    statistics kernels on the same input. A block's 256 threads add into its
    2C LDS floats with float atomics in the order the waves arrive: where one
    address gets at most two adds per block (C >= 1024: a + b is commutative)
    the result is the same bits in every run, and that is asserted; below, the
    last bit moves between two runs of bn_fwd_train itself (seen on the
    MI355X: rstd of 2x8x13x11 off by one ulp, of 3x64x114x114 by 2.1e-6 in
    one channel), and the caller holds both runs to the fp64 reference's
    bound instead, which puts them within twice that bound of each other."""
    if C >= 1024:
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def _half_ulp_of(ref64):
    from test_gpu_bn import _half_ulp
    return _half_ulp(ref64, BF16)


@gpu
@requires_gpu
def test_argument_checks():
    """Every refusal is on the host: nothing is left on the device."""
    ext = _ext()
    K, S, P = 3, 2, 1

    def args(shape, dtype=BF16, nhwc=True):
        N, C, H, W = shape
        x = torch.randn(shape, device="cuda").to(dtype)
        if nhwc:
            x = x.contiguous(memory_format=torch.channels_last)
        v = [torch.ones(C, device="cuda") for _ in range(4)]
        return x, v

    for shape, dtype, nhwc in (((2, 24, 13, 11), BF16, True),
                               ((2, 8, 13, 11), FP32, True),
                               ((2, 8, 13, 11), BF16, False)):
        x, v = args(shape, dtype, nhwc)
        assert not ext.bn_relu_pool_eligible(x, K, S, P)
        _rejects(ext.bn_relu_pool_fwd, x, v[0], v[1], v[2], v[3], 0.1, EPS,
                 K, S, P)
        dp = torch.zeros(shape[0], shape[1], 7, 6, device="cuda", dtype=dtype)
        if nhwc:
            dp = dp.contiguous(memory_format=torch.channels_last)
        idx = torch.zeros(shape[0], 7, 6, shape[1], device="cuda",
                          dtype=torch.uint8)
        _rejects(ext.bn_relu_pool_bwd, x, dp, idx, v[0], v[1], v[2], K, S, P)
    assert not ext.bn_relu_pool_eligible(torch.zeros(2, 8, 13, 11), K, S, P)

    x, v = args((2, 8, 13, 11))
    assert ext.bn_relu_pool_eligible(x, K, S, P)
    p, idx, mean, rstd = ext.bn_relu_pool_fwd(x, v[0], v[1], v[2], v[3], 0.1,
                                              EPS, K, S, P)
    dp = torch.ones_like(p)
    for bad in (idx[:, :-1], idx[..., :4], idx.reshape(-1), idx.int(),
                idx.cpu(), idx.permute(0, 3, 1, 2)):
        _rejects(ext.bn_relu_pool_bwd, x, dp, bad, v[0], mean, rstd, K, S, P)
    _rejects(ext.bn_relu_pool_bwd, x, dp[:, :, :-1], idx, v[0], mean, rstd,
             K, S, P)
    _rejects(ext.bn_relu_pool_bwd, x, dp, idx, v[0][:4], mean, rstd, K, S, P)
    # a 16 x 16 window would need tap index 255, the no-owner byte
    big, vb = args((1, 8, 16, 16))
    assert not ext.bn_relu_pool_eligible(big, 16, 1, 0)
    _rejects(ext.bn_relu_pool_fwd, big, vb[0], vb[1], vb[2], vb[3], 0.1, EPS,
             16, 1, 0)
    ext.bn_relu_pool_bwd(x, dp, idx, v[0], mean, rstd, K, S, P)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# wiring: the models' stem helper
# ---------------------------------------------------------------------------

def _record(mp, fn):
    """Names of the extension entries fn() reaches, in order."""
    ext = _ext()
    names = [n for n in dir(ext)
             if not n.startswith("_") and callable(getattr(ext, n))]
    trace = []

    def wrap(name, orig):
        def f(*a, **kw):
            trace.append(name)
            return orig(*a, **kw)
        return f

    with mp.context() as m:
        for n in names:
            m.setattr(ext, n, wrap(n, getattr(ext, n)))
        out = fn()
        torch.cuda.synchronize()
    return trace, out


def _small_resnet():
    from tensorflowonspark_amd.models.resnet import Bottleneck, ResNet
    return ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10)


def _backbone():
    from tensorflowonspark_amd.models.segmentation import DilatedResNet50
    return DilatedResNet50()


def _stem_run(mp, make, mode, dtype=BF16, nhwc=True, width=None):
    """One training step of the stem helper under TFOS_STEM_POOL=mode."""
    from tensorflowonspark_amd.models.resnet import _stem_forward
    mp.setenv("TFOS_STEM_POOL", mode)
    if width is None:
        mp.delenv("TFOS_STEM", raising=False)
    else:
        # the in-tree stem conv is built for the stem's own width
        mp.setenv("TFOS_STEM", "miopen")
    torch.manual_seed(5)
    model = make()
    if width is not None:
        from tensorflowonspark_amd.ops.modules import (
            FusedBNReLU, FusedMaxPool2d, StemConv7x7)
        model.stem = torch.nn.Sequential(
            StemConv7x7(3, width), FusedBNReLU(width), FusedMaxPool2d(3, 2, 1))
    with torch.no_grad():
        bn = model.stem[1]
        bn.weight.copy_(torch.linspace(0.5, 1.5, bn.num_features))
        bn.bias.copy_(torch.linspace(-0.5, 0.5, bn.num_features))
    model = model.cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(2, 3, 64, 64, device="cuda", generator=gen).to(dtype)
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)

    def run():
        y = _stem_forward(model, x)
        dy = torch.randn(y.shape, device="cuda", generator=gen).to(y.dtype)
        y.backward(dy.contiguous(memory_format=torch.channels_last))
        return y

    trace, y = _record(mp, run)
    return trace, y.detach(), model


def _same_output(y_on, y_off):
    """Both sides compute y with the same arithmetic and round it to the
    output dtype; the statistics come from LDS float atomics, whose last bit
    may move between two runs (2^-20 relative covers that, as in
    test_gpu_bn_dual.py): half an ulp of each side plus that."""
    from test_gpu_bn import _half_ulp
    a, b_ = y_on.double(), y_off.double()
    tol = (_half_ulp(a, y_on.dtype) + _half_ulp(b_, y_off.dtype)
           + 2.0 ** -20 * (a.abs() + 8.0))
    print("  y max diff {:.3e}".format((a - b_).abs().max().item()))
    assert y_on.shape == y_off.shape and y_on.dtype == y_off.dtype
    assert ((a - b_).abs() <= tol).all()


@gpu
@requires_gpu
@pytest.mark.parametrize("make", [_small_resnet, _backbone],
                         ids=["resnet", "deeplab-backbone"])
def test_stem_wiring(make, monkeypatch):
    t_on, y_on, m_on = _stem_run(monkeypatch, make, "on")
    t_off, y_off, m_off = _stem_run(monkeypatch, make, "off")
    print("\n  on :", t_on, "\n  off:", t_off)
    assert t_on == ["conv_stem", "bn_relu_pool_eligible", "bn_relu_pool_fwd",
                    "bn_relu_pool_bwd", "conv_stem_wrw"]
    assert t_off == ["conv_stem", "bn_fwd_train", "maxpool_fwd", "maxpool_bwd",
                     "bn_bwd", "conv_stem_wrw"]
    bn_on, bn_off = m_on.stem[1], m_off.stem[1]
    assert int(bn_on.num_batches_tracked) == 1
    assert int(bn_off.num_batches_tracked) == 1
    # two runs of the same statistics kernels: see _same_statistics
    assert ((bn_on.running_mean - bn_off.running_mean).abs()
            <= 2.0 ** -20 * (bn_off.running_mean.abs() + 1)).all()
    assert ((bn_on.running_var - bn_off.running_var).abs()
            <= 2.0 ** -20 * (bn_off.running_var + 1)).all()
    assert not torch.equal(bn_on.running_var, torch.ones_like(bn_on.running_var))
    _same_output(y_on, y_off)

    # Gradients: 'off' rounds the pool's input gradient (a sum of <= 4 bf16
    # values) to bf16, 'on' keeps it in fp32; both are within the bf16 half
    # ulp of the exact sum, per element. dgamma / dbeta / dweight are sums of
    # those over M = N * 32 * 32 pixels, so they differ by at most
    # sum |err| <= 2^-9 * sum |g| per term: bound them by 2^-8 of the 'off'
    # gradient's own absolute-value scale plus the fp32 reduction noise.
    for name in ("weight", "bias"):
        g_on = getattr(bn_on, name).grad.double()
        g_off = getattr(bn_off, name).grad.double()
        scale = g_off.abs().max()
        print("  d{} max diff {:.3e} (scale {:.3e})".format(
            name, (g_on - g_off).abs().max().item(), scale.item()))
        assert ((g_on - g_off).abs() <= 2.0 ** -7 * scale).all(), name
    w_on = m_on.stem[0].weight.grad.double()
    w_off = m_off.stem[0].weight.grad.double()
    scale = w_off.abs().max()
    print("  dconv max diff {:.3e} (scale {:.3e})".format(
        (w_on - w_off).abs().max().item(), scale.item()))
    assert torch.isfinite(w_on).all()
    assert ((w_on - w_off).abs() <= 2.0 ** -6 * scale).all()


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,nhwc,width", [
    (FP32, True, None), (BF16, False, None), (BF16, True, 24)],
    ids=["fp32", "nchw", "c24"])
def test_stem_fallback(dtype, nhwc, width, monkeypatch):
    """Inputs the fused entries do not take give the two-module result."""
    t_on, y_on, m_on = _stem_run(monkeypatch, _small_resnet, "on", dtype,
                                 nhwc, width)
    t_off, y_off, m_off = _stem_run(monkeypatch, _small_resnet, "off", dtype,
                                    nhwc, width)
    assert "bn_relu_pool_fwd" not in t_on and "bn_relu_pool_bwd" not in t_on
    assert "bn_fwd_train" in t_on
    assert [n for n in t_on if n != "bn_relu_pool_eligible"] == t_off
    _same_output(y_on, y_off)
    g_on, g_off = m_on.stem[1].weight.grad, m_off.stem[1].weight.grad
    # the same kernels on both sides: sums in another order at most
    assert ((g_on - g_off).abs() <= 2.0 ** -10 * g_off.abs().max()).all()
    assert int(m_on.stem[1].num_batches_tracked) == 1


@gpu
@requires_gpu
def test_eval_and_bad_switch(monkeypatch):
    from tensorflowonspark_amd.models.resnet import _stem_forward
    model = _small_resnet().cuda().eval()
    x = torch.randn(2, 3, 64, 64, device="cuda").to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    monkeypatch.setenv("TFOS_STEM_POOL", "on")
    with torch.no_grad():
        trace, y = _record(monkeypatch, lambda: _stem_forward(model, x))
    assert "bn_relu_pool_fwd" not in trace and "bn_fwd_eval" in trace
    assert int(model.stem[1].num_batches_tracked) == 0
    monkeypatch.setenv("TFOS_STEM_POOL", "yes")
    with pytest.raises(ValueError, match="TFOS_STEM_POOL"):
        _stem_forward(model, x)
    assert os.environ["TFOS_STEM_POOL"] == "yes"
