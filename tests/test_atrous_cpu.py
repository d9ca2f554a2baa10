"""Atrous (filter-dilated) 3x3 convolution: everything that needs no GPU.

``live_taps`` against a brute-force enumeration, ``DilatedConv3x3`` as a
drop-in for the ``nn.Conv2d`` it replaces (same parameters, same initial
weights under one seed, same CPU results), the DeepLabV3 wiring, scripting,
and the premise of the exact probes of test_gpu_atrous.py.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

import atrous_cases as ac
from tensorflowonspark_amd.ops.modules import DilatedConv3x3, live_taps


def _brute_live(H, W, k, stride, pad, fd):
    def axis(L):
        out_len = (L + 2 * pad - fd * (k - 1) - 1) // stride + 1
        return tuple(t for t in range(k)
                     if any(0 <= o * stride - pad + t * fd < L
                            for o in range(out_len)))
    return axis(H), axis(W)


def test_live_taps_named_cases():
    assert live_taps(32, 32, 3, 1, 36, 36) == ((1,), (1,))
    assert live_taps(32, 32, 3, 1, 24, 24) == ((0, 1, 2), (0, 1, 2))
    assert live_taps(8, 40, 3, 1, 12, 12) == ((1,), (0, 1, 2))


def test_live_taps_matches_brute_force():
    cases = [(32, 32, 3, 1, 36, 36), (32, 32, 3, 1, 24, 24),
             (8, 40, 3, 1, 12, 12)]
    for H in (1, 4, 5, 8, 13):
        for W in (3, 8):
            for k in (1, 2, 3):
                for stride in (1, 2, 3):
                    for fd in (1, 2, 3, 5, 8, 13):
                        for pad in sorted({0, 1, fd, fd * (k - 1)}):
                            if min(H, W) + 2 * pad - fd * (k - 1) - 1 < 0:
                                continue
                            cases.append((H, W, k, stride, pad, fd))
    assert len(cases) > 500
    for c in cases:
        assert live_taps(*c) == _brute_live(*c), c
    # the module's collapse rule: centre tap only iff fd >= H and fd >= W
    for H in range(1, 10):
        for W in range(1, 10):
            for fd in range(2, 12):
                centre = live_taps(H, W, 3, 1, fd, fd) == ((1,), (1,))
                assert centre == (fd >= H and fd >= W), (H, W, fd)


def test_dilated_conv_is_a_drop_in_conv2d():
    for cin, cout, d in [(64, 64, 2), (32, 96, 12), (3, 5, 4)]:
        torch.manual_seed(1234)
        ref = nn.Conv2d(cin, cout, 3, padding=d, dilation=d, bias=False)
        after_ref = torch.rand(1)
        torch.manual_seed(1234)
        new = DilatedConv3x3(cin, cout, dilation=d)
        after_new = torch.rand(1)
        assert isinstance(new, nn.Conv2d)
        assert torch.equal(new.weight.detach().view(torch.int32),
                           ref.weight.detach().view(torch.int32))
        assert torch.equal(after_ref, after_new)      # same RNG draws
        sd_ref, sd_new = ref.state_dict(), new.state_dict()
        assert list(sd_ref.keys()) == list(sd_new.keys())
        for k in sd_ref:
            assert sd_ref[k].shape == sd_new[k].shape
        assert new.bias is None
        assert new.dilation == (d, d) and new.padding == (d, d)
        assert new.stride == (1, 1) and new.kernel_size == (3, 3)


def test_dilated_conv_rejects_dilation_below_2():
    for d in (0, 1):
        try:
            DilatedConv3x3(32, 64, dilation=d)
        except ValueError:
            continue
        raise AssertionError("dilation {} accepted".format(d))


def test_dilated_conv_cpu_forward_backward():
    g = ac.gen("atrous-cpu-module")
    for d, hw in [(2, (10, 9)), (12, (8, 8)), (3, (7, 16))]:
        m = DilatedConv3x3(8, 6, dilation=d).double()
        x = torch.randn(2, 8, *hw, generator=g).double().requires_grad_(True)
        y = m(x)
        dy = torch.randn(*y.shape, generator=g).double()
        y.backward(dy)
        x2 = x.detach().clone().requires_grad_(True)
        w2 = m.weight.detach().clone().requires_grad_(True)
        y2 = F.conv2d(x2, w2, padding=d, dilation=d)
        y2.backward(dy)
        assert y.shape == (2, 6) + hw
        assert torch.equal(y, y2)
        assert torch.equal(x.grad, x2.grad)
        assert torch.equal(m.weight.grad, w2.grad)


def test_deeplab_wiring_and_state_dict_keys(monkeypatch):
    from tensorflowonspark_amd.models import segmentation as seg
    model = seg.deeplabv3_resnet50()
    for i, rate in zip((1, 2, 3), (12, 24, 36)):
        conv = model.aspp.branches[i][0]
        assert type(conv) is DilatedConv3x3
        assert conv.dilation == (rate, rate) and conv.padding == (rate, rate)
        assert conv.in_channels == 2048 and conv.out_channels == 256
    assert type(model.aspp.branches[0][0]) is nn.Conv2d          # the 1x1
    stage4 = model.backbone.stages[3]
    c2 = stage4[0].conv2
    assert type(c2) is DilatedConv3x3
    assert c2.dilation == (2, 2) and c2.padding == (2, 2)
    assert c2.in_channels == 512 and c2.out_channels == 512
    for blk in stage4:
        assert blk._block_fusable is False
    for blk in list(stage4)[1:]:
        assert not isinstance(blk.conv2, DilatedConv3x3)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]

    # the same model with the class patched back to the plain nn.Conv2d
    def plain(cin, cout, dilation=2):
        return nn.Conv2d(cin, cout, 3, stride=1, padding=dilation,
                         dilation=dilation, bias=False)
    monkeypatch.setattr(seg, "DilatedConv3x3", plain)
    old = seg.deeplabv3_resnet50()
    assert not any(isinstance(m, DilatedConv3x3) for m in old.modules())
    assert keys == [(k, tuple(v.shape)) for k, v in old.state_dict().items()]


def test_deeplab_initial_weights_unchanged(monkeypatch):
    """Under one seed the ASPP branch holds the weights the plain nn.Conv2d
    model holds (subclassing keeps the RNG draw order)."""
    from tensorflowonspark_amd.models import segmentation as seg
    torch.manual_seed(7)
    new = seg.ASPP(64, 32, rates=(2, 3))

    def plain(cin, cout, dilation=2):
        return nn.Conv2d(cin, cout, 3, stride=1, padding=dilation,
                         dilation=dilation, bias=False)
    monkeypatch.setattr(seg, "DilatedConv3x3", plain)
    torch.manual_seed(7)
    old = seg.ASPP(64, 32, rates=(2, 3))
    sd_new, sd_old = new.state_dict(), old.state_dict()
    assert list(sd_new.keys()) == list(sd_old.keys())
    for k in sd_new:
        assert torch.equal(sd_new[k], sd_old[k]), k


def test_convbnrelu_scripts_and_matches_eager():
    from tensorflowonspark_amd.models.segmentation import ConvBNReLU
    torch.manual_seed(3)
    m = ConvBNReLU(64, 64, dilation=2).eval()
    assert type(m[0]) is DilatedConv3x3
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 64, 10, 9)
    with torch.no_grad():
        eager = m(x)
    # the hook hands the scripter a plain conv sharing the weight
    clone = m[0].__prepare_scriptable__()
    assert type(clone) is nn.Conv2d
    assert clone.weight is m[0].weight
    assert clone.dilation == (2, 2) and clone.padding == (2, 2)
    scripted = torch.jit.script(m)
    with torch.no_grad():
        got = scripted(x)
    assert got.shape == eager.shape == (2, 64, 10, 9)
    assert torch.allclose(got, eager, rtol=1e-5, atol=1e-6)


def test_atrous_routing(monkeypatch):
    from tensorflowonspark_amd.ops import modules
    route = modules._atrous_route
    monkeypatch.setenv("TFOS_ATROUS", "miopen")
    assert route(32, 32, 32, 2048, 256, 36) is None
    monkeypatch.setenv("TFOS_ATROUS", "mfma")
    assert route(32, 32, 32, 2048, 256, 36) == (True, True, True)
    assert route(32, 32, 32, 2048, 256, 24) == (False, True, True)
    assert route(1, 8, 40, 2048, 256, 12) == (False, True, True)
    # auto at the DeepLabV3 benchmark shapes follows the measured table
    monkeypatch.delenv("TFOS_ATROUS")
    assert route(32, 32, 32, 512, 512, 2) == (False, True, True)
    assert route(32, 32, 32, 2048, 256, 12) == (False, False, True)
    assert route(32, 32, 32, 2048, 256, 24) == (False, False, True)
    assert route(32, 32, 32, 2048, 256, 36) == (True, True, True)
    # a launch that cannot fill the chip stays on the library
    assert route(2, 10, 9, 64, 64, 2) is None
    monkeypatch.setenv("TFOS_ATROUS", "bogus")
    try:
        route(32, 32, 32, 2048, 256, 36)
    except ValueError:
        return
    raise AssertionError("TFOS_ATROUS=bogus accepted")


def test_exact_probe_premise_cpu():
    """For every exact case: sum |a||b| < 2^24, so each partial sum in any
    order is exact in fp32, and the fp32 CPU result does equal the fp64
    reference bit for bit."""
    names = set()
    for name, fn in ac.exact_contractions():
        names.add(name)
        s64 = fn(ac.FP64, False)
        abs_sum = fn(ac.FP64, True)
        assert abs_sum.max().item() < ac.EXACT_LIMIT, name
        assert (s64.abs() <= abs_sum).all(), name
        s32 = fn(ac.FP32, False)
        assert s32.dtype == ac.FP32 and s64.dtype == ac.FP64, name
        assert torch.equal(s32.contiguous().view(torch.int32),
                           s64.float().contiguous().view(torch.int32)), name
    assert len(names) == len(ac.FWD_EXACT) + 1 + len(ac.DGRAD_NAMES) \
        + len(ac.WRW_EXACT) + 1


def test_case_geometry_cpu():
    """Each case lands where its name says (dispatch rules recomputed from
    the launchers) and pins what the table claims."""
    by = ac.FWD_BY_NAME
    for c in ac.FWD_EXACT:
        assert c["Cin"] % 32 == 0
    M = lambda c: c["N"] * c["OH"] * c["OW"]
    assert ac.conv_tier(M(by["t128-d2"]), 72) == ("t128", 2)
    assert M(by["t128-d2"]) == 264
    assert ac.conv_tier(M(by["t256-d2"]), 200) == ("t256", 2)
    assert by["t128-d3-rect"]["Cin"] * 9 // 32 == 18
    assert (by["pad0"]["OH"], by["pad1"]["OH"], by["s2"]["OH"]) == (5, 7, 5)
    assert (by["f2x3"]["OH"], by["f2x3"]["OW"]) == (10, 9)
    # aspp: the outer tap rows are valid on only 4 of the 16 output rows
    c = by["aspp"]
    assert sum(1 for oh in range(16) if 0 <= oh - 12 + 0 * 12 < 16) == 4
    assert live_taps(c["H"], c["W"], 3, 1, 12, 12) == ((0, 1, 2), (0, 1, 2))
    for name in ("dead-5", "dead-7"):
        c = by[name]
        assert live_taps(c["H"], c["W"], 3, 1, c["P"], c["fd"]) \
            == ((1,), (1,))
        assert (c["OH"], c["OW"]) == (5, 5)
    for name in ac.DGRAD_NAMES:
        c = by[name]
        assert c["S"] == 1 and c["P"] == c["fd"] and c["Cin"] % 32 == 0
    for c in ac.WRW_EXACT:
        m = c["N"] * c["OH"] * c["OW"]
        want = 2 if c["name"] == ac.WRW_SPLIT_CASE else 1
        assert ac.wrw2_split(c["Cout"], c["Cin"], m) == want, c["name"]
        assert (c["OH"], c["OW"]) == (c["H"], c["W"])
    c = ac.WRW_BY_NAME[ac.WRW_DEAD_CASE]
    assert live_taps(c["H"], c["W"], 3, 1, c["P"], c["fd"]) == ((1,), (1,))
    ref, _ = ac.wrw_refs(ac.WRW_DEAD_CASE)
    dead = ref.view(c["Cout"], 9, c["Cin"])[:, [0, 1, 2, 3, 5, 6, 7, 8], :]
    assert (dead == 0).all() and (ref != 0).any()
    # dead-tap forward cases equal the 1x1 conv of the centre tap
    for name in ("dead-5", "dead-7"):
        x, w4 = ac.fwd_inputs(name)
        y, _ = ac.fwd_refs(name)
        assert torch.equal(y, F.conv2d(x.double(), w4.double()[:, :, 1:2, 1:2]))
