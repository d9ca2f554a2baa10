"""Atrous (filter-dilated) convolution on the in-tree MFMA kernels vs fp64.

``conv_mfma(..., fd=)`` forward and dgrad, ``conv_wrw2(..., fd=)`` and the
``DilatedConv3x3`` module, with the method of test_gpu_mfma.py: exact probes
on small integers compared bit for bit, real-valued probes against the derived
bound (see atrous_cases.py).  The fp64 references are ``F.conv2d`` with
``dilation=fd`` and its fp64 autograd gradients on the CPU.
"""

import pytest
import torch
import torch.nn.functional as F

import atrous_cases as ac
from atrous_cases import BF16, FP32

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _run_fwd(c, x, w4, out_f32, explicit=False):
    oh, ow = (c["OH"], c["OW"]) if explicit else (-1, -1)
    return _ext().conv_mfma(_cl(x.cuda()), ac.w4_to_wk(w4).cuda(), c["Cout"],
                            c["fh"], c["fw"], c["S"], c["P"], 1, oh, ow,
                            fd=c["fd"], out_f32=out_f32)


def _run_dgrad(c, dy, w4, out_f32):
    # dy has c.Cin channels, dx c.Cout; pad = 2*fd - P = fd, output H x W
    return _ext().conv_mfma(_cl(dy.cuda()), ac.dgrad_weight(w4).cuda(),
                            c["Cout"], 3, 3, 1, 2 * c["fd"] - c["P"], 1,
                            c["H"], c["W"], fd=c["fd"], out_f32=out_f32)


def _run_wrw(c, x, dy):
    return _ext().conv_wrw2(_cl(dy.cuda()), _cl(x.cuda()), 3, 3, 1, c["P"],
                            fd=c["fd"])


@gpu
@requires_gpu
@pytest.mark.parametrize("out", ["bf16", "f32"])
@pytest.mark.parametrize("case", ac.FWD_EXACT, ids=lambda c: c["name"])
def test_atrous_forward_exact(case, out):
    c = case
    x, w4 = ac.fwd_inputs(c["name"])
    y64, _ = ac.fwd_refs(c["name"])
    assert y64.shape == (c["N"], c["Cout"], c["OH"], c["OW"])
    got = _run_fwd(c, x, w4, out == "f32")
    assert got.is_contiguous(memory_format=torch.channels_last)
    ac.assert_bits("conv_mfma fd={} {}".format(c["fd"], out), got,
            y64.float() if out == "f32" else ac.to_bf16(y64))
    if c["name"].startswith("dead"):
        # every outer tap goes to the guard: the 1x1 conv of the centre tap
        centre = F.conv2d(x.double(), w4.double()[:, :, 1:2, 1:2])
        ac.assert_bits("dead taps", got, centre.float() if out == "f32"
                       else ac.to_bf16(centre))


@gpu
@requires_gpu
def test_atrous_forward_explicit_output_size():
    """Explicit OH/OW equal to the natural size give the same result."""
    c = ac.FWD_BY_NAME["pad1"]
    x, w4 = ac.fwd_inputs(c["name"])
    y64, _ = ac.fwd_refs(c["name"])
    ac.assert_bits("explicit OH/OW", _run_fwd(c, x, w4, False, explicit=True),
                   ac.to_bf16(y64))


@gpu
@requires_gpu
@pytest.mark.parametrize("out", ["bf16", "f32"])
@pytest.mark.parametrize("name", ac.DGRAD_NAMES)
def test_atrous_dgrad_exact(name, out):
    c = ac.FWD_BY_NAME[name]
    dy, w4 = ac.dgrad_inputs(name)
    dx64, _ = ac.dgrad_refs(name)
    got = _run_dgrad(c, dy, w4, out == "f32")
    ac.assert_bits("dgrad fd={} {}".format(c["fd"], out), got,
                   dx64.float() if out == "f32" else ac.to_bf16(dx64))


@gpu
@requires_gpu
@pytest.mark.parametrize("out", ["bf16", "f32"])
def test_atrous_forward_real(out):
    c = ac.FWD_BY_NAME["t256-d2"]
    x, w4 = ac.fwd_inputs(c["name"], True)
    y64, absprod = ac.fwd_refs(c["name"], True)
    got = _run_fwd(c, x, w4, out == "f32")
    ac.assert_bound("fwd real " + out, got, y64, absprod, 9 * c["Cin"],
                    FP32 if out == "f32" else BF16)


@gpu
@requires_gpu
@pytest.mark.parametrize("out", ["bf16", "f32"])
def test_atrous_dgrad_real(out):
    c = ac.FWD_BY_NAME["t256-d2"]
    dy, w4 = ac.dgrad_inputs(c["name"], True)
    dx64, absprod = ac.dgrad_refs(c["name"], True)
    got = _run_dgrad(c, dy, w4, out == "f32")
    ac.assert_bound("dgrad real " + out, got, dx64, absprod, 9 * c["Cin"],
                    FP32 if out == "f32" else BF16)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ac.WRW_EXACT, ids=lambda c: c["name"])
def test_atrous_wrw_exact(case):
    c = case
    x, dy = ac.wrw_inputs(c["name"])
    dw64, _ = ac.wrw_refs(c["name"])
    M = c["N"] * c["OH"] * c["OW"]
    if c["name"] == ac.WRW_SPLIT_CASE:
        assert ac.wrw2_split(c["Cout"], c["Cin"], M) > 1
    got = _run_wrw(c, x, dy)
    assert got.dtype == FP32
    ac.assert_bits("conv_wrw2 fd={}".format(c["fd"]), got, dw64.float())
    if c["name"] == ac.WRW_DEAD_CASE:
        dead = got.view(c["Cout"], 9, c["Cin"])[:, [0, 1, 2, 3, 5, 6, 7, 8]]
        assert (dead == 0).all() and (got != 0).any()


@gpu
@requires_gpu
def test_atrous_wrw_real():
    c = ac.WRW_REAL
    x, dy = ac.wrw_inputs(c["name"], True)
    dw64, absprod = ac.wrw_refs(c["name"], True)
    got = _run_wrw(c, x, dy)
    ac.assert_bound("wrw real", got, dw64, absprod,
                    c["N"] * c["OH"] * c["OW"], FP32)


@gpu
@requires_gpu
def test_atrous_argument_checks():
    ext = _ext()
    x = _cl(torch.ones(1, 32, 9, 9, device="cuda", dtype=BF16))
    w9 = torch.ones(64, 9 * 32, device="cuda", dtype=BF16)
    w1 = torch.ones(64, 32, device="cuda", dtype=BF16)
    ok = ext.conv_mfma(x, w9, 64, 3, 3, 1, 2, 1, -1, -1, fd=2)
    assert ok.shape == (1, 64, 9, 9)
    big = (1 << 20) // 2 + 1                   # fd*(3-1) just past the cap
    for fd in (0, -1):
        with pytest.raises(RuntimeError):
            ext.conv_mfma(x, w9, 64, 3, 3, 1, 2, 1, -1, -1, fd=fd)
    with pytest.raises(RuntimeError):          # fd > 1 needs D == 1
        ext.conv_mfma(x, w9, 64, 3, 3, 1, 2, 2, -1, -1, fd=2)
    with pytest.raises(RuntimeError):          # fd*(fh-1) bounded
        ext.conv_mfma(x, w9, 64, 3, 3, 1, big, 1, 9, 9, fd=big)
    w13 = torch.ones(64, 3 * 32, device="cuda", dtype=BF16)
    with pytest.raises(RuntimeError):          # fd*(fw-1) bounded
        ext.conv_mfma(x, w13, 64, 1, 3, 1, 0, 1, 9, 9, fd=big)
    with pytest.raises(RuntimeError):          # fd itself bounded (1x1 filter)
        ext.conv_mfma(x, w1, 64, 1, 1, 1, 0, 1, -1, -1, fd=(1 << 20) + 1)
    with pytest.raises(RuntimeError):          # filter larger than the input
        ext.conv_mfma(x, w9, 64, 3, 3, 1, 0, 1, -1, -1, fd=5)
    # D == 2 with fd == 1 is still served
    assert ext.conv_mfma(x, w1, 64, 1, 1, 1, 0, 2, -1, -1).shape \
        == (1, 64, 17, 17)

    dy = _cl(torch.ones(1, 64, 9, 9, device="cuda", dtype=BF16))
    assert ext.conv_wrw2(dy, x, 3, 3, 1, 2, fd=2).shape == (64, 9 * 32)
    for fd in (0, -3):
        with pytest.raises(RuntimeError):
            ext.conv_wrw2(dy, x, 3, 3, 1, 2, fd=fd)
    with pytest.raises(RuntimeError):          # 1x1 has no dilation
        ext.conv_wrw2(dy, x, 1, 1, 1, 0, fd=2)
    with pytest.raises(RuntimeError):          # reach bounded
        ext.conv_wrw2(dy, x, 3, 3, 1, big, fd=big)
    torch.cuda.synchronize()


@gpu
@requires_gpu
def test_fd1_regression_guard_exact():
    """The fd = 1 path of the edited kernels, through the same entry points,
    stays bit-identical to fp64 (test_gpu_mfma.py pins it in full)."""
    c = ac.FD1_CASE
    x, w4 = ac.fwd_inputs(c["name"])
    y64, _ = ac.fwd_refs(c["name"])
    ext = _ext()
    wk = ac.w4_to_wk(w4).cuda()
    pos = ext.conv_mfma(_cl(x.cuda()), wk, c["Cout"], 3, 3, 1, 1, 1, -1, -1)
    kw = ext.conv_mfma(_cl(x.cuda()), wk, c["Cout"], 3, 3, 1, 1, 1, -1, -1,
                       fd=1)
    ac.assert_bits("conv_mfma positional", pos, ac.to_bf16(y64))
    ac.assert_bits("conv_mfma fd=1", kw, ac.to_bf16(y64))
    w = ac.WRW_FD1
    xw, dyw = ac.wrw_inputs(w["name"])
    dw64, _ = ac.wrw_refs(w["name"])
    pos = ext.conv_wrw2(_cl(dyw.cuda()), _cl(xw.cuda()), 3, 3, 1, 1)
    kw = ext.conv_wrw2(_cl(dyw.cuda()), _cl(xw.cuda()), 3, 3, 1, 1, fd=1)
    ac.assert_bits("conv_wrw2 positional", pos, dw64.float())
    ac.assert_bits("conv_wrw2 fd=1", kw, dw64.float())


# ---------------------------------------------------------------------------
# module wiring
# ---------------------------------------------------------------------------

def _module_refs(m, x, dy, fd):
    """fp64 (y, dx, dw) and their abs-sums from the bf16 values the kernels
    see (the module rounds its fp32 weight to bf16)."""
    w = m.weight.detach().cpu().to(BF16)

    def run(xv, wv, dyv):
        xv = xv.double().requires_grad_(True)
        wv = wv.double().requires_grad_(True)
        y = F.conv2d(xv, wv, padding=fd, dilation=fd)
        y.backward(dyv.double())
        return y.detach(), xv.grad, wv.grad
    return run(x, w, dy), run(x.abs(), w.abs(), dy.abs())


@gpu
@requires_gpu
@pytest.mark.parametrize("wrw", ["mfma2", "miopen"])
def test_module_wiring_mfma(monkeypatch, wrw):
    from tensorflowonspark_amd.ops.modules import (DilatedConv3x3,
                                                   _AtrousConv3x3Fn)
    monkeypatch.setenv("TFOS_ATROUS", "mfma")
    monkeypatch.setenv("TFOS_WRW", wrw)
    g = ac.gen("atrous-module-d2")
    torch.manual_seed(11)
    m = DilatedConv3x3(64, 64, dilation=2).cuda()
    x = ac.real_nchw(g, 2, 64, 10, 9)
    dy = ac.real_nchw(g, 2, 64, 10, 9)
    xg = _cl(x.cuda()).requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == _AtrousConv3x3Fn.__name__ + "Backward"
    y.backward(_cl(dy.cuda()))
    (y64, dx64, dw64), (ya, dxa, dwa) = _module_refs(m, x, dy, 2)
    assert y.dtype == BF16 and xg.grad.dtype == BF16
    assert m.weight.grad.dtype == FP32
    ac.assert_bound("module y", y, y64, ya, 9 * 64, BF16)
    ac.assert_bound("module dx", xg.grad, dx64, dxa, 9 * 64, BF16)
    # the in-tree wrw returns its fp32 accumulator; the library's bf16
    ac.assert_bound("module dw " + wrw, m.weight.grad, dw64, dwa, 2 * 10 * 9,
                    FP32 if wrw == "mfma2" else BF16)


@gpu
@requires_gpu
@pytest.mark.parametrize("wrw", ["mfma2", "miopen"])
def test_module_collapse_mfma(monkeypatch, wrw):
    from tensorflowonspark_amd.ops.modules import (Conv1x1, DilatedConv3x3,
                                                   _AtrousCollapsedFn)
    monkeypatch.setenv("TFOS_ATROUS", "mfma")
    monkeypatch.setenv("TFOS_WRW", wrw)
    g = ac.gen("atrous-module-d12")
    torch.manual_seed(12)
    m = DilatedConv3x3(64, 64, dilation=12).cuda()
    x = ac.real_nchw(g, 2, 64, 8, 8)
    dy = ac.real_nchw(g, 2, 64, 8, 8)
    xg = _cl(x.cuda()).requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == _AtrousCollapsedFn.__name__ + "Backward"
    y.backward(_cl(dy.cuda()))
    # bit-identical to the Conv1x1 path on the centre tap
    c1 = Conv1x1(64, 64).cuda()
    with torch.no_grad():
        c1.weight.copy_(m.weight[:, :, 1:2, 1:2])
    x1 = _cl(x.cuda()).requires_grad_(True)
    y1 = c1(x1)
    y1.backward(_cl(dy.cuda()))
    ac.assert_bits("collapsed y", y, y1.detach().cpu())
    ac.assert_bits("collapsed dx", xg.grad, x1.grad.cpu())
    dw = m.weight.grad
    assert dw.shape == (64, 64, 3, 3)
    ac.assert_bits("collapsed dw centre", dw[:, :, 1, 1],
                   c1.weight.grad[:, :, 0, 0].cpu())
    dead = dw.reshape(64, 64, 9)[:, :, [0, 1, 2, 3, 5, 6, 7, 8]]
    assert (dead == 0).all() and (dw[:, :, 1, 1] != 0).any()
    # and it is the atrous conv: fp64 at the derived bound
    (y64, dx64, dw64), (ya, dxa, dwa) = _module_refs(m, x, dy, 12)
    assert (dw64.reshape(64, 64, 9)[:, :, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()
    ac.assert_bound("collapsed y vs fp64", y, y64, ya, 64, BF16)
    ac.assert_bound("collapsed dx vs fp64", xg.grad, dx64, dxa, 64, BF16)


@gpu
@requires_gpu
def test_module_miopen_route(monkeypatch):
    from tensorflowonspark_amd.ops.modules import DilatedConv3x3
    monkeypatch.setenv("TFOS_ATROUS", "miopen")
    m = DilatedConv3x3(64, 64, dilation=2).cuda().to(BF16)
    x = _cl(ac.real_nchw(ac.gen("atrous-miopen"), 1, 64, 10, 9).cuda())
    y = m(x.requires_grad_(True))
    name = type(y.grad_fn).__name__
    assert "Atrous" not in name and "Convolution" in name, name
    assert y.shape == (1, 64, 10, 9)


@gpu
@requires_gpu
@pytest.mark.parametrize("fwd_in_tree,dgrad_in_tree",
                         [(False, True), (True, False)],
                         ids=["lib-fwd", "lib-dgrad"])
def test_mixed_routes(monkeypatch, fwd_in_tree, dgrad_in_tree):
    """TFOS_ATROUS=auto may leave one direction on the library: the function
    then mixes library and in-tree calls.  The in-tree direction meets the
    derived bound; the library's direction returns what the library returns
    when called directly (its rounding is its own: the forward was measured
    a full bf16 ulp off the fp64 result, outside the in-tree bound)."""
    from tensorflowonspark_amd.ops.modules import (DilatedConv3x3,
                                                   _AtrousConv3x3Fn)
    monkeypatch.setenv("TFOS_WRW", "auto")
    g = ac.gen("atrous-module-mixed")
    torch.manual_seed(13)
    m = DilatedConv3x3(64, 64, dilation=3).cuda()
    x = ac.real_nchw(g, 2, 64, 10, 9)
    dy = ac.real_nchw(g, 2, 64, 10, 9)
    xg = _cl(x.cuda()).requires_grad_(True)
    dyg = _cl(dy.cuda())
    y = _AtrousConv3x3Fn.apply(xg, m.weight, 3, fwd_in_tree, dgrad_in_tree)
    y.backward(dyg)
    (y64, dx64, dw64), (ya, dxa, dwa) = _module_refs(m, x, dy, 3)
    wb = m.weight.detach().to(BF16)
    if fwd_in_tree:
        ac.assert_bound("mixed y", y, y64, ya, 9 * 64, BF16)
    else:
        ac.assert_bits("mixed y (library)", y,
                       F.conv2d(xg.detach(), wb, None, 1, 3, 3).cpu())
    if dgrad_in_tree:
        ac.assert_bound("mixed dx", xg.grad, dx64, dxa, 9 * 64, BF16)
    else:
        lib_dx = torch.ops.aten.convolution_backward(
            dyg, xg.detach(), _cl(wb), None, [1, 1], [3, 3], [3, 3], False,
            [0, 0], 1, [True, False, False])[0]
        ac.assert_bits("mixed dx (library)", xg.grad, lib_dx.cpu())
    ac.assert_bound("mixed dw", m.weight.grad, dw64, dwa, 2 * 10 * 9, FP32)
