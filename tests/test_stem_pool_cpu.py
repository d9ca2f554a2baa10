"""The stem helper off the GPU: TFOS_STEM_POOL is validated at every call, a
CPU forward is the three stem modules' whatever the switch says, and the
models still script."""

import copy

import pytest
import torch

from tensorflowonspark_amd.models.resnet import resnet50
from tensorflowonspark_amd.models.segmentation import deeplabv3_resnet50
from tensorflowonspark_amd.ops.modules import stem_forward


def _models():
    torch.manual_seed(0)
    return {"resnet50": (resnet50(num_classes=10), (2, 3, 64, 64)),
            "deeplabv3": (deeplabv3_resnet50(num_classes=3), (2, 3, 64, 64))}


@pytest.fixture(scope="module")
def baselines():
    """Per model: the model, its input and the output of the plain
    composition stem -> rest, computed once without the helper."""
    out = {}
    for name, (model, shape) in _models().items():
        x = torch.randn(*shape)
        state = copy.deepcopy(model.state_dict())
        body = model if name == "resnet50" else model.backbone
        model.train()
        with torch.no_grad():
            h = body.stages(body.stem(x))
            if name == "resnet50":
                ref = model.fc(torch.flatten(model.avgpool(h), 1))
            else:
                ref = model.upsample(model.classifier(model.aspp(h)),
                                     x.shape[-2:])
        out[name] = (model, x, state, ref)
    return out


@pytest.mark.parametrize("mode", ["on", "off", None])
@pytest.mark.parametrize("name", ["resnet50", "deeplabv3"])
def test_cpu_forward_unchanged(name, mode, baselines, monkeypatch):
    model, x, state, ref = baselines[name]
    if mode is None:
        monkeypatch.delenv("TFOS_STEM_POOL", raising=False)
    else:
        monkeypatch.setenv("TFOS_STEM_POOL", mode)
    model.load_state_dict(state)     # running statistics as the baseline had
    model.train()
    with torch.no_grad():
        got = model(x)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("bad", ["", "1", "ON", "auto"])
def test_bad_switch_raises(bad, baselines, monkeypatch):
    model, x, state, _ = baselines["resnet50"]
    monkeypatch.setenv("TFOS_STEM_POOL", bad)
    with pytest.raises(ValueError, match="TFOS_STEM_POOL"):
        stem_forward(model.stem, x)
    with pytest.raises(ValueError, match="TFOS_STEM_POOL"):
        model(x)


def test_stem_is_the_same_sequential():
    from tensorflowonspark_amd.ops.modules import (FusedBNReLU,
                                                   FusedMaxPool2d, StemConv7x7)
    model = resnet50(num_classes=10)
    assert [type(m) for m in model.stem] == [StemConv7x7, FusedBNReLU,
                                             FusedMaxPool2d]
    keys = [k for k in model.state_dict() if k.startswith("stem.")]
    assert keys == ["stem.0.weight", "stem.1.weight", "stem.1.bias",
                    "stem.1.running_mean", "stem.1.running_var",
                    "stem.1.num_batches_tracked"]


def test_resnet50_scripts(monkeypatch):
    monkeypatch.setenv("TFOS_STEM_POOL", "on")
    torch.manual_seed(1)
    model = resnet50(num_classes=10).eval()
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        want = model(x)
    sm = torch.jit.script(copy.deepcopy(model))
    with torch.no_grad():
        got = sm(x)
    assert torch.allclose(got, want, atol=1e-4, rtol=1e-4)
