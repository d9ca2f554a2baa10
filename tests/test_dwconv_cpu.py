"""DepthwiseConv3x3 without a GPU: the CPU path, the U-Net wiring, scripting,
the TFOS_DW routing and the premises of the GPU suite (tests/test_gpu_dwconv).
"""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dwconv_cases import (BF16, FP32, SMALL, channels, dw_ref, exact_inputs,
                          out_size, real_inputs, seen_weight)
from tensorflowonspark_amd.ops import modules as M
from tensorflowonspark_amd.ops.modules import DepthwiseConv3x3


def _plain(C, stride=1):
    return nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [FP32, torch.float64])
def test_cpu_path_is_the_plain_conv(stride, dtype):
    torch.manual_seed(0)
    new = DepthwiseConv3x3(12, stride).to(dtype)
    old = _plain(12, stride).to(dtype)
    with torch.no_grad():
        old.weight.copy_(new.weight)
    x = torch.randn(2, 12, 7, 6, dtype=dtype)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = new(xa), old(xb)
    assert type(ya.grad_fn).__name__ == type(yb.grad_fn).__name__
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(ya, yb)
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(new.weight.grad, old.weight.grad)


def test_module_is_the_conv_it_stands_for():
    torch.manual_seed(11)
    new = DepthwiseConv3x3(24, 2)
    torch.manual_seed(11)
    old = _plain(24, 2)
    assert isinstance(new, nn.Conv2d)
    assert [n for n, _ in new.named_parameters()] == ["weight"]
    assert new.weight.shape == (24, 1, 3, 3) and new.bias is None
    assert (new.stride, new.padding, new.dilation, new.groups) == \
        (old.stride, old.padding, old.dilation, old.groups)
    assert torch.equal(new.weight, old.weight)
    with pytest.raises(ValueError):
        DepthwiseConv3x3(8, 3)


def _unet_depthwise(model):
    return [(n, m) for n, m in model.named_modules()
            if isinstance(m, DepthwiseConv3x3)]


def test_unet_wiring_and_state_dict(monkeypatch):
    from tensorflowonspark_amd.models import segmentation as seg
    torch.manual_seed(7)
    model = seg.unet_mobilenet()
    dws = _unet_depthwise(model)
    assert len(dws) == 17
    # at exactly the grouped 3x3 convs, nowhere else
    for n, m in model.named_modules():
        if isinstance(m, nn.Conv2d):
            grouped = m.groups > 1
            assert (type(m) is DepthwiseConv3x3) == grouped, n
            if grouped:
                assert m.groups == m.in_channels == m.out_channels
                assert m.kernel_size == (3, 3) and m.padding == (1, 1)
                assert m.stride in ((1, 1), (2, 2)) and m.bias is None
    assert sorted({m.in_channels for _, m in dws}) == \
        [32, 96, 144, 192, 384, 576, 960]
    assert sum(m.stride == (2, 2) for _, m in dws) == 4
    sd_new = model.state_dict()

    def plain(channels, stride=1):
        return _plain(channels, stride)
    monkeypatch.setattr(seg, "DepthwiseConv3x3", plain)
    torch.manual_seed(7)
    old = seg.unet_mobilenet()
    assert not _unet_depthwise(old)
    sd_old = old.state_dict()
    assert list(sd_new.keys()) == list(sd_old.keys())
    for k in sd_new:
        assert sd_new[k].shape == sd_old[k].shape, k
        assert torch.equal(sd_new[k], sd_old[k]), k


def test_other_convbnrelu_shapes_stay_plain():
    from tensorflowonspark_amd.models.segmentation import ConvBNReLU
    assert type(ConvBNReLU(32, 32, groups=32, stride=2)[0]) is DepthwiseConv3x3
    assert type(ConvBNReLU(32, 32, groups=32)[0]) is DepthwiseConv3x3
    assert type(ConvBNReLU(32, 32)[0]) is nn.Conv2d              # dense
    assert type(ConvBNReLU(32, 64, groups=32)[0]) is nn.Conv2d   # multiplier 2
    assert type(ConvBNReLU(32, 32, groups=8)[0]) is nn.Conv2d    # grouped
    assert type(ConvBNReLU(32, 32, k=1, groups=32)[0]) is nn.Conv2d
    assert type(ConvBNReLU(32, 32, k=5, groups=32)[0]) is nn.Conv2d
    assert type(ConvBNReLU(32, 32, groups=32, stride=3)[0]) is nn.Conv2d
    assert type(ConvBNReLU(32, 32, groups=32, dilation=2)[0]) is nn.Conv2d


def test_scripts_and_matches_eager():
    from tensorflowonspark_amd.models.segmentation import ConvBNReLU
    torch.manual_seed(3)
    m = ConvBNReLU(32, 32, groups=32, stride=2).eval()
    assert type(m[0]) is DepthwiseConv3x3
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 32, 10, 9)
    with torch.no_grad():
        eager = m(x)
    clone = m[0].__prepare_scriptable__()
    assert type(clone) is nn.Conv2d
    assert clone.weight is m[0].weight
    assert clone.groups == 32 and clone.stride == (2, 2)
    assert clone.padding == (1, 1) and clone.bias is None
    scripted = torch.jit.script(m)
    with torch.no_grad():
        got = scripted(x)
    assert got.shape == eager.shape == (2, 32, 5, 5)
    assert torch.allclose(got, eager, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------

def test_route_modes(monkeypatch):
    shape = (64, 96, 64, 64, 2)
    monkeypatch.setenv("TFOS_DW", "miopen")
    assert M._dw_route(*shape) is None
    monkeypatch.setenv("TFOS_DW", "hip")
    assert M._dw_route(*shape) == (True, True, True)
    assert M._dw_route(1, 8, 1, 1, 1) == (True, True, True)
    monkeypatch.setenv("TFOS_DW", "cudnn")
    with pytest.raises(ValueError, match="TFOS_DW"):
        M._dw_route(*shape)
    # auto: per direction from _dw_auto; all-library is the plain conv
    monkeypatch.setenv("TFOS_DW", "auto")
    monkeypatch.setattr(M, "_dw_auto", lambda d, *a: d == "dgrad")
    assert M._dw_route(*shape) == (False, True, False)
    monkeypatch.setattr(M, "_dw_auto", lambda d, *a: False)
    assert M._dw_route(*shape) is None
    monkeypatch.delenv("TFOS_DW")
    assert M._dw_route(*shape) is None       # auto is the default


def _unet_shapes(batch):
    """(N, C, H, W, stride) of the 17 depthwise layers at 128 x 128."""
    from tensorflowonspark_amd.models import unet_mobilenet
    model = unet_mobilenet().eval()
    seen = []
    hooks = [m.register_forward_pre_hook(
        lambda mod, a: seen.append((batch, mod.in_channels, a[0].shape[2],
                                    a[0].shape[3], mod.stride[0])))
        for _, m in _unet_depthwise(model)]
    with torch.no_grad():
        model(torch.zeros(1, 3, 128, 128))
    for h in hooks:
        h.remove()
    return seen


# docs/performance.md "Depthwise convolutions": the decision of the b64 run
# for each distinct U-Net layer, (fwd, dgrad, wrw).
UNET_B64_AUTO = {
    (64, 32, 64, 64, 1): (True, True, True),
    (64, 96, 64, 64, 2): (True, True, True),
    (64, 144, 32, 32, 1): (True, True, True),
    (64, 144, 32, 32, 2): (True, True, True),
    (64, 192, 16, 16, 1): (True, True, True),
    (64, 192, 16, 16, 2): (True, True, True),
    (64, 384, 8, 8, 1): (True, True, True),
    (64, 576, 8, 8, 1): (True, True, True),
    (64, 576, 8, 8, 2): (True, True, True),
    (64, 960, 4, 4, 1): (True, True, True),
}


def test_auto_is_the_measured_table(monkeypatch):
    monkeypatch.setenv("TFOS_DW", "auto")
    shapes = _unet_shapes(64)
    assert len(shapes) == 17
    assert set(shapes) == set(UNET_B64_AUTO)
    for s in shapes:
        want = UNET_B64_AUTO[s]
        got = tuple(M._dw_auto(d, *s) for d in ("fwd", "dgrad", "wrw"))
        assert got == want, s
        assert M._dw_route(*s) == (want if any(want) else None)


def test_auto_table_is_the_recorded_run():
    """_dw_table() repeats profiles/unet_dw_bench.json row for row: in-tree
    exactly where that run measured the in-tree kernel no slower."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "unet_dw_bench.json")
    with open(path) as f:
        rows = json.load(f)
    table = {r[:5]: r[5:] for r in M._dw_table()}
    seen = set()
    for r in rows:
        key = (r["N"], r["C"], r["H"], r["W"], r["stride"])
        seen.add(key)
        won = r["in_tree_ms"] <= r["library_ms"]
        assert (r["auto"] == "in-tree") == won, r
        assert table[key][("fwd", "dgrad", "wrw").index(r["dir"])] == won, r
    assert seen == set(table) and len(rows) == 3 * len(table)


def test_auto_unmeasured_shape_takes_nearest_rule():
    """A shape off the table takes the decision of the measured shape of the
    same stride nearest in element count, as _dw_auto's docstring says."""
    for s in (1, 2):
        rows = [r for r in M._dw_table() if r[4] == s]
        small = min(rows, key=lambda r: r[0] * r[1] * r[2] * r[3])
        big = max(rows, key=lambda r: r[0] * r[1] * r[2] * r[3])
        for i, d in enumerate(("fwd", "dgrad", "wrw")):
            assert M._dw_auto(d, 1, 8, 2, 2, s) == small[5 + i]
            assert M._dw_auto(d, 4096, 96, 64, 64, s) == big[5 + i]
            # one more channel vector than a measured row: that row's rule
            n, c, h, w = big[:4]
            assert M._dw_auto(d, n, c + 8, h, w, s) == big[5 + i]


# ---------------------------------------------------------------------------
# premises of the GPU suite
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
def test_reference_agrees_with_the_library(stride):
    x, dy, w = real_inputs(2, 12, 7, 6, stride, FP32, "cpu", seed=3)
    ry, rdx, rdw = dw_ref(x, w, dy, stride)
    xl, wl = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv2d(xl, wl, None, stride, 1, 1, 12)
    y.backward(dy)
    for got, ref in ((y.detach(), ry), (xl.grad, rdx), (wl.grad, rdw)):
        assert got.shape == ref.shape
        assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-5)
    # and with the formulas of the kernels' header, tap by tap
    N, C, H, W = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = F.pad(x.double(), (1, 1, 1, 1))
    y2 = torch.zeros(N, C, Ho, Wo, dtype=torch.float64)
    dw2 = torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride,
                     kx:kx + (Wo - 1) * stride + 1:stride]
            y2 += win * w.double()[:, 0, ky, kx][None, :, None, None]
            dw2[:, 0, ky, kx] = (win * dy.double()).sum((0, 2, 3))
    assert torch.allclose(y2, ry, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dw2, rdw, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
def test_exact_probe_premise(dtype, stride):
    """Integer inputs in [-3, 3], distinct filters, every partial sum below
    2^24 and every forward/dgrad output a bf16 value."""
    for N, c, H, W in SMALL:
        C = channels(c, dtype)
        x, dy, w = exact_inputs(N, C, H, W, stride, dtype, "cpu")
        for t in (x, dy, w):
            assert torch.equal(t.double(), t.double().round())
            assert t.abs().max() <= 3
        assert x.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(seen_weight(w, dtype), w)
        flat = w.view(C, 9)
        assert len({tuple(r.tolist()) for r in flat}) == C
        # the largest any partial sum can get is the sum of magnitudes
        ay, adx, adw = dw_ref(x.abs(), w.abs(), dy.abs(), stride)
        M_ = N * out_size(H, stride) * out_size(W, stride)
        assert ay.max() <= 81 and adx.max() <= 81 and adw.max() <= 9 * M_
        assert max(ay.max(), adx.max(), adw.max()) < 2 ** 24
        ry, rdx, rdw = dw_ref(x, w, dy, stride)
        for r in (ry, rdx):
            assert r.abs().max() <= 256
            assert torch.equal(r.to(BF16).double(), r)
        assert torch.equal(rdw.to(FP32).double(), rdw)
