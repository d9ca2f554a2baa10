"""Depthwise 3x3 kernels (csrc/dwconv3x3.hip) against fp64.

The reference is fp64 ``F.conv2d(groups=C)`` and its autograd on the values
the kernel sees (dwconv_cases.dw_ref).

Exact probes (integers in [-3, 3], a different filter per channel) must match
bit for bit: forward, dgrad and wrw, bf16 and fp32, stride 1 and 2; why they
are exact is argued in dwconv_cases and asserted in test_dwconv_cpu.

Real-valued probes are held to

    fwd, dgrad   9 * 2^-23 * (|x| * |w|) + half_ulp(out dtype)
    wrw          M * 2^-23 * sum |dy||x|,  M = N*Ho*Wo  (any summation order)

the GEMM suites' form with K = 9: each of the 9 fused multiply-adds rounds
once, relative 2^-24, on a partial sum bounded by the absolute sum, and the
factor 2 covers the growth of (1 + u)^9; the output is rounded once more to
its dtype. The real-valued wrw cases keep M <= 512 so the bound means
something; dropped terms are the exact probes' job.

Tiers and the case that reaches each are listed in docs/components.md
("Depthwise coverage").
"""

import pytest
import torch

from dwconv_cases import (SMALL, channels, dw_ref, exact_inputs, out_size,
                          real_inputs, seen_weight)
from test_gpu_bn import (BF16, FP32, _DEV, _bits_equal, _ext, _half_ulp, _vec,
                         gpu, requires_gpu)

CL = torch.channels_last


def _canon(t):
    """-0 -> +0: the sign of an exact zero depends on the summation's start
    value, which is not the kernels' business."""
    return t + torch.zeros((), dtype=t.dtype, device=t.device)


def _run(ext, x, dy, w, stride):
    y = ext.dwconv3x3_fwd(x, w, stride)
    dx = ext.dwconv3x3_dgrad(dy, w, stride, x.shape[2], x.shape[3])
    dw = ext.dwconv3x3_wrw(dy, x, stride)
    torch.cuda.synchronize()
    N, C, H, W = x.shape
    assert y.shape == dy.shape and y.dtype == x.dtype
    assert dx.shape == x.shape and dx.dtype == x.dtype
    assert y.is_contiguous(memory_format=CL)
    assert dx.is_contiguous(memory_format=CL)
    assert dw.shape == (C, 1, 3, 3) and dw.dtype == FP32 and dw.is_contiguous()
    return y, dx, dw


def _assert_exact(ext, N, C, H, W, stride, dtype, what=("fwd", "dgrad", "wrw")):
    x, dy, w = exact_inputs(N, C, H, W, stride, dtype, _DEV)
    M = N * out_size(H, stride) * out_size(W, stride)
    assert 9 * M < 2 ** 24
    ry, rdx, rdw = dw_ref(x, seen_weight(w, dtype), dy, stride)
    if "fwd" in what:
        y = ext.dwconv3x3_fwd(x, w, stride)
        assert _bits_equal(_canon(y), _canon(ry.to(dtype))), "fwd"
    if "dgrad" in what:
        dx = ext.dwconv3x3_dgrad(dy, w, stride, H, W)
        assert _bits_equal(_canon(dx), _canon(rdx.to(dtype))), "dgrad"
    if "wrw" in what:
        dw = ext.dwconv3x3_wrw(dy, x, stride)
        assert _bits_equal(_canon(dw), _canon(rdw.to(FP32))), "wrw"


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_exact(shape, dtype, stride):
    N, c, H, W = shape
    _assert_exact(_ext(), N, channels(c, dtype), H, W, stride, dtype)


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_real(shape, dtype, stride):
    ext = _ext()
    N, c, H, W = shape
    C = channels(c, dtype)
    M = N * out_size(H, stride) * out_size(W, stride)
    assert M <= 512
    x, dy, w = real_inputs(N, C, H, W, stride, dtype, _DEV)
    y, dx, dw = _run(ext, x, dy, w, stride)
    ws = seen_weight(w, dtype)
    ry, rdx, rdw = dw_ref(x, ws, dy, stride)
    ay, adx, adw = dw_ref(x.abs(), ws.abs(), dy.abs(), stride)
    u = 2.0 ** -23
    for name, got, ref, mag, k, out_dtype in (
            ("fwd", y, ry, ay, 9, dtype), ("dgrad", dx, rdx, adx, 9, dtype),
            ("wrw", dw, rdw, adw, M, None)):
        tol = k * u * mag
        if out_dtype is not None:
            tol = tol + _half_ulp(ref, out_dtype)
        err = (got.double() - ref).abs()
        print("{} max err {:.3e} max tol {:.3e}".format(
            name, err.max().item(), tol.max().item()))
        bad = err > tol
        assert not bad.any(), "{}: {} of {} outside the bound".format(
            name, int(bad.sum()), bad.numel())


# ---------------------------------------------------------------------------
# launcher tiers
# ---------------------------------------------------------------------------

def _past_cap(info, per_row_items, cv):
    """Smallest square side whose (side * per_row_items(side) * cv) work
    items exceed the capped grid, so the stride loop runs a second, ragged
    pass."""
    cap = info["max_grid"] * info["block"]
    side = 8
    while side * per_row_items(side) * cv <= cap:
        side += 8
    return side


@gpu
@requires_gpu
def test_forward_past_grid_cap():
    """C = 24 (3 vectors): the launcher also rounds the grid so the stride
    stays a multiple of Cv."""
    ext = _ext()
    info = ext.dwconv3x3_info()
    L = info["strip"]
    side = _past_cap(info, lambda s: (s + L - 1) // L, 3)
    assert side * side * 24 * 2 < 40e6
    _assert_exact(ext, 1, 24, side, side, 1, BF16, what=("fwd",))


@gpu
@requires_gpu
def test_dgrad_past_grid_cap():
    ext = _ext()
    info = ext.dwconv3x3_info()
    pair = info["pair"]
    side = _past_cap(info, lambda s: (s + pair - 1) // pair, 3)
    assert side * side * 24 * 2 < 40e6
    _assert_exact(ext, 1, 24, side, side, 2, BF16, what=("dgrad",))


@gpu
@requires_gpu
def test_dgrad_stride1_past_grid_cap():
    ext = _ext()
    info = ext.dwconv3x3_info()
    L = info["strip"]
    side = _past_cap(info, lambda s: (s + L - 1) // L, 3)
    assert side * side * 24 * 2 < 40e6
    _assert_exact(ext, 1, 24, side, side, 1, BF16, what=("dgrad",))


@gpu
@requires_gpu
def test_wrw_past_block_cap():
    """More pixels than wrw_max_blocks slabs of the minimum size: the slab
    grows past the minimum and the last one is ragged."""
    ext = _ext()
    info = ext.dwconv3x3_info()
    C, Cv = 32, 4
    side = 8
    while True:
        plan = ext.dwconv3x3_wrw_plan(side * side, Cv)
        if plan["slab"] > plan["P"] * info["wrw_min_pix"] \
                and (side * side) % plan["slab"]:
            break
        side += 8
    assert plan["nblk"] * plan["grid_y"] <= info["wrw_max_blocks"]
    assert side * side * C * 2 < 40e6
    _assert_exact(ext, 1, C, side, side, 1, BF16, what=("wrw",))


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_weight_view_in_flat_bucket(dtype):
    """A DDP engine keeps parameters as views into one flat buffer: the
    weight may start at any 4-byte offset."""
    ext = _ext()
    C = 3 * _vec(dtype)
    x, dy, w = exact_inputs(2, C, 5, 6, 2, dtype, _DEV)
    flat = torch.zeros(w.numel() + 3, device=_DEV)
    wv = flat[3:].view(C, 1, 3, 3)
    wv.copy_(w)
    assert wv.data_ptr() % 16 != 0 and wv.is_contiguous()
    assert _bits_equal(ext.dwconv3x3_fwd(x, wv, 2), ext.dwconv3x3_fwd(x, w, 2))
    assert _bits_equal(ext.dwconv3x3_dgrad(dy, wv, 2, 5, 6),
                       ext.dwconv3x3_dgrad(dy, w, 2, 5, 6))
    assert _bits_equal(ext.dwconv3x3_dgrad(dy, wv, 1, 3, 3),
                       ext.dwconv3x3_dgrad(dy, w, 1, 3, 3))


@gpu
@requires_gpu
def test_wrw_plan_tiers():
    """The small cases reach the split they are listed for."""
    ext = _ext()
    one = ext.dwconv3x3_wrw_plan(1 * 5 * 7, 1)
    assert one["nblk"] == 1 and one["slab"] >= 35          # less than a slab
    two = ext.dwconv3x3_wrw_plan(3 * 5 * 7, 18)            # C = 144 bf16
    assert two["nblk"] == 2 and two["P"] == 14 and 256 % 18
    assert 35 < two["slab"] < 70 and 105 % two["slab"]     # inside image 1
    deep = ext.dwconv3x3_wrw_plan(1 * 4 * 4, 120)          # C = 960 bf16
    assert deep["grid_y"] == 2 and deep["cvb"] == 60
    many = ext.dwconv3x3_wrw_plan(2 * 9 * 9, 120)
    fin = ext.dwconv3x3_info()["fin_lanes"]
    assert many["nblk"] > fin and many["nblk"] % fin
    assert (2 * 9 * 9) % many["slab"]


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_wrw_deterministic(stride):
    ext = _ext()
    x, dy, _ = real_inputs(3, 144, 12, 12, stride, BF16, _DEV, seed=5)
    a = ext.dwconv3x3_wrw(dy, x, stride)
    b = ext.dwconv3x3_wrw(dy, x, stride)
    assert _bits_equal(a, b)


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------

def _valid(dtype=BF16, stride=1):
    x, dy, w = exact_inputs(2, 2 * _vec(dtype), 5, 6, stride, dtype, _DEV)
    return x, dy, w


@gpu
@requires_gpu
def test_bindings_accept_valid_calls():
    ext = _ext()
    for dtype in (BF16, FP32):
        for stride in (1, 2):
            x, dy, w = _valid(dtype, stride)
            _run(ext, x, dy, w, stride)


@gpu
@requires_gpu
def test_bindings_reject_device_mismatch():
    ext = _ext()
    x, dy, w = _valid()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.dwconv3x3_fwd(x.cpu(), w, 1)
    with pytest.raises(RuntimeError, match="weight must be on"):
        ext.dwconv3x3_fwd(x, w.cpu(), 1)
    with pytest.raises(RuntimeError, match="weight must be on"):
        ext.dwconv3x3_dgrad(dy, w.cpu(), 1, 5, 6)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.dwconv3x3_dgrad(dy.cpu(), w, 1, 5, 6)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.dwconv3x3_wrw(dy, x.cpu(), 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.dwconv3x3_wrw(dy.cpu(), x, 1)


@gpu
@requires_gpu
def test_bindings_reject_dtype():
    ext = _ext()
    x, dy, w = _valid()
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        ext.dwconv3x3_fwd(x.half(), w, 1)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        ext.dwconv3x3_dgrad(dy.half(), w, 1, 5, 6)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        ext.dwconv3x3_wrw(dy.double(), x.double(), 1)
    with pytest.raises(RuntimeError, match="one dtype"):
        ext.dwconv3x3_wrw(dy.float(), x, 1)


@gpu
@requires_gpu
def test_bindings_reject_layout():
    ext = _ext()
    x, dy, w = _valid()
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.dwconv3x3_fwd(x.contiguous(), w, 1)
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.dwconv3x3_dgrad(dy.contiguous(), w, 1, 5, 6)
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.dwconv3x3_wrw(dy.contiguous(), x, 1)
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.dwconv3x3_wrw(dy, x.contiguous(), 1)
    with pytest.raises(RuntimeError, match="4-D"):
        ext.dwconv3x3_fwd(x[0], w, 1)
    # the expanded gradient of y.sum().backward() is not a real tensor
    with pytest.raises(RuntimeError, match="channels_last"):
        ext.dwconv3x3_dgrad(torch.ones((), device=_DEV, dtype=BF16)
                            .expand_as(dy), w, 1, 5, 6)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_bindings_reject_channel_count(dtype):
    ext = _ext()
    C = _vec(dtype) + _vec(dtype) // 2
    x, dy, w = exact_inputs(1, C, 4, 4, 1, dtype, _DEV)
    with pytest.raises(RuntimeError, match="multiple of"):
        ext.dwconv3x3_fwd(x, w, 1)
    with pytest.raises(RuntimeError, match="multiple of"):
        ext.dwconv3x3_dgrad(dy, w, 1, 4, 4)
    with pytest.raises(RuntimeError, match="multiple of"):
        ext.dwconv3x3_wrw(dy, x, 1)


@gpu
@requires_gpu
def test_bindings_reject_weight():
    ext = _ext()
    x, dy, w = _valid()
    C = x.shape[1]
    bad = {
        "bf16": w.to(BF16),
        "channels": w[: C // 2].contiguous(),
        "full": w.expand(C, C, 3, 3).contiguous(),
        "5x5": torch.zeros(C, 1, 5, 5, device=_DEV),
        "3-D": w.view(C, 3, 3),
        "strided": torch.zeros(C, 1, 3, 6, device=_DEV)[..., ::2],
    }
    for name, wb in bad.items():
        with pytest.raises(RuntimeError, match=r"\[C,1,3,3\]"):
            ext.dwconv3x3_fwd(x, wb, 1)
        with pytest.raises(RuntimeError, match=r"\[C,1,3,3\]"):
            ext.dwconv3x3_dgrad(dy, wb, 1, 5, 6)


@gpu
@requires_gpu
def test_bindings_reject_stride_and_geometry():
    ext = _ext()
    x, dy, w = _valid()
    for s in (0, 3, -1):
        with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
            ext.dwconv3x3_fwd(x, w, s)
        with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
            ext.dwconv3x3_dgrad(dy, w, s, 5, 6)
        with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
            ext.dwconv3x3_wrw(dy, x, s)
    # dy is 5x6: H/W that do not give it
    with pytest.raises(RuntimeError, match="the gradient is"):
        ext.dwconv3x3_dgrad(dy, w, 1, 6, 6)
    with pytest.raises(RuntimeError, match="the gradient is"):
        ext.dwconv3x3_dgrad(dy, w, 2, 5, 6)
    with pytest.raises(RuntimeError, match="the gradient is"):
        ext.dwconv3x3_dgrad(dy, w, 2, 9, 13)      # 5x7
    ext.dwconv3x3_dgrad(dy, w, 2, 9, 11)          # 5x6: both 9x11 and 10x12
    ext.dwconv3x3_dgrad(dy, w, 2, 10, 12)
    with pytest.raises(RuntimeError, match="gives a gradient of"):
        ext.dwconv3x3_wrw(dy, x, 2)
    with pytest.raises(RuntimeError, match="gives a gradient of"):
        ext.dwconv3x3_wrw(dy[:1], x, 1)
    with pytest.raises(RuntimeError, match="gives a gradient of"):
        ext.dwconv3x3_wrw(dy[:, :8].contiguous(memory_format=CL), x, 1)
    torch.cuda.synchronize()


@gpu
@requires_gpu
def test_empty_returns_empty():
    ext = _ext()
    w = torch.ones(16, 1, 3, 3, device=_DEV)
    x = torch.empty(0, 16, 5, 6, device=_DEV, dtype=BF16)
    y = ext.dwconv3x3_fwd(x, w, 2)
    assert y.shape == (0, 16, 3, 3) and y.dtype == BF16
    dx = ext.dwconv3x3_dgrad(y, w, 2, 5, 6)
    assert dx.shape == (0, 16, 5, 6)
    dw = ext.dwconv3x3_wrw(y, x, 2)
    assert dw.shape == (16, 1, 3, 3) and dw.dtype == FP32
    assert not dw.any()
    x0 = torch.empty(2, 16, 0, 6, device=_DEV, dtype=FP32)
    y0 = ext.dwconv3x3_fwd(x0, w, 1)
    assert y0.shape == (2, 16, 0, 6) and y0.numel() == 0


# ---------------------------------------------------------------------------
# module wiring
# ---------------------------------------------------------------------------

def _module_case(dtype, stride, C=None):
    from tensorflowonspark_amd.ops.modules import DepthwiseConv3x3
    C = C or 3 * _vec(dtype)
    x, dy, w = exact_inputs(3, C, 7, 5, stride, dtype, _DEV)
    m = DepthwiseConv3x3(C, stride).to(_DEV)
    with torch.no_grad():
        m.weight.copy_(w)
    return m, x.requires_grad_(), w


def _assert_module_exact(m, x, w, dtype, stride):
    """y.sum().backward(): the gradient arrives expanded (stride 0)."""
    y = m(x)
    y.sum().backward()
    ones = torch.ones_like(y)
    ry, rdx, rdw = dw_ref(x.detach(), seen_weight(w, dtype), ones, stride)
    assert _bits_equal(_canon(y.detach()), _canon(ry.to(dtype)))
    assert _bits_equal(_canon(x.grad), _canon(rdx.to(dtype)))
    assert m.weight.grad.dtype == FP32
    assert _bits_equal(_canon(m.weight.grad), _canon(rdw.to(FP32)))
    return y


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_module_hip_route(monkeypatch, dtype, stride):
    from tensorflowonspark_amd.ops.modules import _DepthwiseFn
    monkeypatch.setenv("TFOS_DW", "hip")
    m, x, w = _module_case(dtype, stride)
    y = _assert_module_exact(m, x, w, dtype, stride)
    assert type(y.grad_fn).__name__ == _DepthwiseFn.__name__ + "Backward"


@gpu
@requires_gpu
def test_module_library_routes(monkeypatch):
    # the plain conv takes bf16 activations with its fp32 weight only under
    # autocast, which is how the models run it
    monkeypatch.setenv("TFOS_DW", "miopen")
    m, x, w = _module_case(BF16, 1)
    with torch.autocast("cuda", dtype=BF16):
        y = m(x)
    assert "Depthwise" not in type(y.grad_fn).__name__
    # bf16 C = 12 is no multiple of 8: library, whatever the mode says
    monkeypatch.setenv("TFOS_DW", "hip")
    m, x, w = _module_case(BF16, 1, C=12)
    with torch.autocast("cuda", dtype=BF16):
        y = m(x)
    assert y.dtype == BF16
    assert "Depthwise" not in type(y.grad_fn).__name__
    ry, _, _ = dw_ref(x.detach(), seen_weight(w, BF16), torch.ones_like(y), 1)
    assert _bits_equal(_canon(y.detach()), _canon(ry.to(BF16)))


@gpu
@requires_gpu
@pytest.mark.parametrize("route", [(True, False, False), (False, True, False),
                                   (False, False, True), (False, True, True),
                                   (True, False, True)],
                         ids=lambda r: "".join("hl"[not f] for f in r))
@pytest.mark.parametrize("stride", [1, 2])
def test_module_mixed_routes(monkeypatch, route, stride):
    """A forward through the library with an in-tree backward, and every
    other mix, gives the same exact results."""
    import tensorflowonspark_amd.ops.modules as M
    monkeypatch.setenv("TFOS_DW", "auto")
    monkeypatch.setattr(
        M, "_dw_auto",
        lambda d, *a: route[("fwd", "dgrad", "wrw").index(d)])
    m, x, w = _module_case(BF16, stride)
    ext = _ext()
    calls = []
    for n in ("dwconv3x3_fwd", "dwconv3x3_dgrad", "dwconv3x3_wrw"):
        orig = getattr(ext, n)
        monkeypatch.setattr(
            ext, n, lambda *a, _n=n, _o=orig: (calls.append(_n), _o(*a))[1])
    _assert_module_exact(m, x, w, BF16, stride)
    want = [n for n, f in zip(("dwconv3x3_fwd", "dwconv3x3_dgrad",
                               "dwconv3x3_wrw"), route) if f]
    assert calls == want


@gpu
@requires_gpu
def test_module_needs_input_grad(monkeypatch):
    monkeypatch.setenv("TFOS_DW", "hip")
    m, x, w = _module_case(BF16, 1)
    ext = _ext()
    calls = []
    for n in ("dwconv3x3_dgrad", "dwconv3x3_wrw"):
        orig = getattr(ext, n)
        monkeypatch.setattr(
            ext, n, lambda *a, _n=n, _o=orig: (calls.append(_n), _o(*a))[1])
    m(x.detach()).sum().backward()           # no grad for x
    assert calls == ["dwconv3x3_wrw"]
    del calls[:]
    m.weight.requires_grad_(False)
    m(x).sum().backward()
    assert calls == ["dwconv3x3_dgrad"]


@gpu
@requires_gpu
def test_inverted_residual_reaches_kernels(monkeypatch):
    from test_gpu_calltrace import _record
    from tensorflowonspark_amd.models.segmentation import InvertedResidual
    monkeypatch.setenv("TFOS_DW", "hip")
    torch.manual_seed(0)
    blk = InvertedResidual(32, 32, 1).to(_DEV).train()
    x = torch.randn(2, 32, 16, 16, device=_DEV).contiguous(
        memory_format=CL).requires_grad_()

    def run():
        with torch.autocast("cuda", dtype=BF16):
            y = blk(x)
        y.float().sum().backward()
        return y

    with monkeypatch.context() as mp:
        trace, y = _record(mp, run)
    names = [c[0] for c in trace]
    for n in ("dwconv3x3_fwd", "dwconv3x3_dgrad", "dwconv3x3_wrw"):
        assert names.count(n) == 1, names
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    for n, p in blk.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    from tensorflowonspark_amd.ops.modules import DepthwiseConv3x3
    assert type(blk.conv[1][0]) is DepthwiseConv3x3
