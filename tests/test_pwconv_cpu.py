"""PointwiseConv without a GPU: the module is the conv it stands for, the
U-Net wiring, TFOS_PW parsing and the premise of the exact GPU probes."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tensorflowonspark_amd.models.segmentation as seg
import tensorflowonspark_amd.ops.modules as M
from pwconv_cases import SHAPES, exact_inputs, exact_premise, pw_ref
from tensorflowonspark_amd.ops.modules import PointwiseConv


def _plain(cin, cout):
    return nn.Conv2d(cin, cout, 1, bias=False)


def test_module_is_the_conv_it_stands_for():
    torch.manual_seed(3)
    m = PointwiseConv(24, 144)
    torch.manual_seed(3)
    ref = _plain(24, 144)
    assert isinstance(m, nn.Conv2d) and m.bias is None
    assert [n for n, _ in m.named_parameters()] == ["weight"]
    assert torch.equal(m.weight, ref.weight)
    x = torch.randn(2, 24, 5, 3)
    assert torch.equal(m(x), F.conv2d(x, ref.weight))


def test_unet_wiring_and_state_dict(monkeypatch):
    torch.manual_seed(0)
    unet = seg.unet_mobilenet()
    assert sum(isinstance(m, PointwiseConv) for m in unet.modules()) == 33
    deeplab = seg.deeplabv3_resnet50()
    assert not any(isinstance(m, PointwiseConv) for m in deeplab.modules())
    aspp = deeplab.aspp
    for conv in (aspp.branches[0][0], aspp.pool[1], aspp.project[0]):
        assert type(conv) is nn.Conv2d and conv.kernel_size == (1, 1)
    monkeypatch.setattr(seg, "PointwiseConv", _plain)
    torch.manual_seed(0)
    plain = seg.unet_mobilenet().state_dict()
    sd = unet.state_dict()
    assert list(sd) == list(plain)
    assert all(torch.equal(sd[k], plain[k]) for k in sd)


def test_route_modes_and_nearest_rule(monkeypatch):
    assert all(row[7] in ("wrw2", "lib") for row in M._pw_table())
    monkeypatch.setenv("TFOS_PW", "miopen")
    assert M._pw_route(64, 16, 96, 64, 64) is None
    monkeypatch.setenv("TFOS_PW", "hip")
    assert M._pw_route(64, 192, 64, 8, 8) == (True, True, "wrw2")
    monkeypatch.setenv("TFOS_PW", "fast")
    with pytest.raises(ValueError, match="TFOS_PW"):
        M._pw_route(64, 16, 96, 64, 64)
    monkeypatch.setenv("TFOS_PW", "auto")
    monkeypatch.setattr(M, "_pw_table", lambda: (
        (64, 16, 96, 64, 64, True, False, "wrw2"),
        (64, 960, 320, 4, 4, False, False, "lib")))
    assert M._pw_route(64, 16, 96, 64, 64) == (True, False, "wrw2")
    assert M._pw_route(64, 960, 320, 4, 4) is None
    # unmeasured: the row with the nearest M * (cin + cout)
    assert M._pw_route(32, 16, 96, 64, 64) == (True, False, "wrw2")
    assert M._pw_route(8, 960, 160, 4, 4) is None


def test_scripted_unet_matches_eager():
    torch.manual_seed(0)
    model = seg.unet_mobilenet().eval()
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        want = model(x)
        got = torch.jit.script(model)(x)
    assert (got - want).abs().max() <= 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_premise(shape):
    shape = tuple({"T": 64, "T+1": 65}.get(v, v) for v in shape)
    assert max(exact_premise(*shape).values()) < 2 ** 24
    x, dy, w = exact_inputs(*shape)
    for t in (x, dy, w * 8):
        assert torch.equal(t.float(), t.float().round())
    y, _, _ = pw_ref(x, w, dy)
    assert torch.equal(y.float().double(), y)      # exact in fp32
