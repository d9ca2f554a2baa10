"""What the bilinear upsampling GPU tests rest on, without a GPU."""

import pytest
import torch
import torch.nn.functional as F

import tensorflowonspark_amd.ops.modules as M
from upsample_cases import (BF16, CASES, FP32, axis_matrix, case_id, inputs,
                            ub_ref)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_is_the_library_in_fp64(case):
    x, dy = (t.double().contiguous() for t in inputs(case, FP32, exact=False))
    for align in case[6]:
        xr = x.clone().requires_grad_()
        y = F.interpolate(xr, size=case[4:6], mode="bilinear", align_corners=align)
        dx, = torch.autograd.grad(y, xr, dy)
        ry, rdx = ub_ref(x, dy, align)
        assert (y - ry).abs().max() < 1e-12 and (dx - rdx).abs().max() < 1e-11


@pytest.mark.parametrize("case", [c for c in CASES if c[7]], ids=case_id)
def test_exact_premise(case):
    """Every term is a multiple of 2^-10, absolute sums below 2^24 of them."""
    x, dy = inputs(case, BF16, exact=True)
    assert x.abs().max() <= 3 and torch.equal(x, x.round())
    Wy, Wx = axis_matrix(case[2], case[4], False), axis_matrix(case[3], case[5], False)
    w = torch.einsum("oh,pw->ohpw", Wy, Wx) * 1024
    assert torch.equal(w, w.round())
    ay, adx = ub_ref(x.abs(), dy.abs(), False)
    assert max(ay.max(), adx.max()) * 1024 < 2 ** 24


def test_mode_parsing(monkeypatch):
    shape = (32, 21, 32, 32, 512, 512)
    monkeypatch.setenv("TFOS_UPSAMPLE", "hip")
    assert M._ub_route(*shape) == (True, True)
    monkeypatch.setenv("TFOS_UPSAMPLE", "aten")
    assert M._ub_route(*shape) is None
    monkeypatch.setenv("TFOS_UPSAMPLE", "HIP")
    with pytest.raises(ValueError, match="TFOS_UPSAMPLE"):
        M._ub_route(*shape)
    monkeypatch.delenv("TFOS_UPSAMPLE")
    rows = {r[:6]: r[6:] for r in M._ub_table()}
    want = rows[shape] if any(rows[shape]) else None
    assert M._ub_route(*shape) == want
    # an unmeasured shape takes the nearest measured rule
    near = rows[(32, 256, 1, 1, 32, 32)]
    assert M._ub_route(2, 256, 1, 1, 8, 8) == (near if any(near) else None)


def test_cpu_path_is_the_library():
    x = torch.randn(2, 3, 4, 5, requires_grad=True)
    for align in (False, True):
        y = M.BilinearUpsample(align)(x, (9, 7))
        assert torch.equal(y, F.interpolate(x, size=(9, 7), mode="bilinear",
                                            align_corners=align))
    y.sum().backward()
    assert x.grad.shape == x.shape


def test_deeplab_keys_and_script():
    import copy
    from tensorflowonspark_amd.models.segmentation import DeepLabV3
    model = DeepLabV3(num_classes=5).eval()
    assert isinstance(model.upsample, M.BilinearUpsample)
    assert isinstance(model.aspp.upsample, M.BilinearUpsample)
    assert not [k for k in model.state_dict() if "upsample" in k]
    x = torch.randn(1, 3, 64, 64)
    sm = torch.jit.script(copy.deepcopy(model))
    with torch.no_grad():
        assert torch.allclose(sm(x), model(x), atol=1e-5)
