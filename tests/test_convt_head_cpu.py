"""ConvTranspose2dHead without a GPU: drop-in parity with nn.ConvTranspose2d,
the U-Net wiring, scripting, TFOS_CONVT_HEAD and the exact-probe premise."""

import pytest
import torch
import torch.nn as nn

from convt_head_cases import ct_ref, exact_inputs, exact_premise
from tensorflowonspark_amd.ops import modules as M
from tensorflowonspark_amd.ops.modules import ConvTranspose2dHead


def _pair(cin=80, cout=3, seed=3):
    torch.manual_seed(seed)
    ours = ConvTranspose2dHead(cin, cout)
    after_ours = torch.rand(1)
    torch.manual_seed(seed)
    lib = nn.ConvTranspose2d(cin, cout, 4, stride=2, padding=1)
    return ours, lib, after_ours, torch.rand(1)


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_drop_in_parity_and_cpu_forward():
    ours, lib, r0, r1 = _pair()
    assert _same_state(ours, lib) and torch.equal(r0, r1)
    assert list(ours.state_dict()) == ["weight", "bias"]
    x = torch.randn(2, 80, 5, 3)
    assert torch.equal(ours(x), lib(x))
    assert torch.equal(ours(x, output_size=[10, 6]), lib(x, output_size=[10, 6]))


def test_unet_head_wiring(monkeypatch):
    from tensorflowonspark_amd.models import segmentation as seg
    torch.manual_seed(0)
    net = seg.UNetMobileNet(3)
    assert type(net.head) is ConvTranspose2dHead
    assert (net.head.in_channels, net.head.out_channels) == (80, 3)
    keys = [k for k in net.state_dict() if k.startswith("head.")]
    assert keys == ["head.weight", "head.bias"]
    # the same model with the library module in the head's place
    monkeypatch.setattr(seg, "ConvTranspose2dHead",
                        lambda cin, cout: nn.ConvTranspose2d(
                            cin, cout, 4, stride=2, padding=1))
    torch.manual_seed(0)
    assert _same_state(net, seg.UNetMobileNet(3))


def test_scripting_shares_parameters():
    ours, lib, _, _ = _pair(16, 2)
    scripted = torch.jit.script(ours)
    x = torch.randn(1, 16, 3, 4)
    assert torch.equal(scripted(x), lib(x))
    names = dict(scripted.named_parameters())
    assert names["weight"].data_ptr() == ours.weight.data_ptr()
    assert names["bias"].data_ptr() == ours.bias.data_ptr()


def test_route_modes(monkeypatch):
    shape = (64, 80, 3, 64, 64)
    monkeypatch.setenv("TFOS_CONVT_HEAD", "hip")
    assert M._cth_route(*shape) == (True, True, True)
    monkeypatch.setenv("TFOS_CONVT_HEAD", "miopen")
    assert M._cth_route(*shape) is None
    monkeypatch.delenv("TFOS_CONVT_HEAD")
    table = M._cth_table()
    for row in table:
        want = row[5:] if any(row[5:]) else None
        assert M._cth_route(*row[:5]) == want
    # an unmeasured shape takes the rule of the nearest measured one
    near = min(table, key=lambda r: r[0])
    assert M._cth_route(near[0] + 1, *near[1:5]) == \
        (near[5:] if any(near[5:]) else None)
    monkeypatch.setenv("TFOS_CONVT_HEAD", "fast")
    with pytest.raises(ValueError, match="TFOS_CONVT_HEAD"):
        M._cth_route(*shape)


def test_exact_probe_premise():
    """The largest probes stay exact in fp32, and the integers really are
    what the fp64 reference sums."""
    for shape in ((3, 256, 8, 5, 3), (1, 8, 1, 643, 643), (1, 8, 1, 520, 520)):
        assert max(exact_premise(*shape).values()) < 2 ** 24
    shape = (2, 16, 3, 3, 5)
    x, dy, w, b = exact_inputs(*shape)
    assert len({tuple(f.flatten().tolist()) for f in w.flatten(0, 1)}) == 48
    refs = ct_ref(x, w, b, dy)
    bound = exact_premise(*shape)
    for r, k in zip(refs, ("fwd", "dgrad", "wrw", "db")):
        assert torch.equal(r, r.round()) and r.abs().max() <= bound[k]
