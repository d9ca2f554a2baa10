"""Bilinear upsampling kernels (csrc/upsample_bilinear.hip) against fp64:
exact probes bit for bit, real probes inside the bound of upsample_cases.
Tiers and their cases: docs/components.md, "Bilinear upsampling coverage"."""

import pytest
import torch

from test_gpu_bn import _DEV, _bits_equal, _ext, _off_grid, gpu, requires_gpu
from upsample_cases import (BF16, CASES, CL, FP32, bounds, case_id, inputs,
                            ub_ref)



def _canon(t):   # -0 -> +0
    return t.cpu() + torch.zeros((), dtype=t.dtype)


def _run(what, x, dy, align):
    if what == "fwd":
        out = _ext().upsample_bilinear_fwd(x.to(_DEV), *dy.shape[2:], align)
    else:
        out = _ext().upsample_bilinear_bwd(dy.to(_DEV), *x.shape[2:], align)
    assert out.shape == (dy if what == "fwd" else x).shape
    assert out.is_contiguous(memory_format=CL)
    return out


def _assert_exact(case, what, dtype, align):
    x, dy = inputs(case, dtype, exact=True)
    ref = ub_ref(x, dy, align)[what == "bwd"]
    assert float(ref.abs().max()) * 1024 < 2 ** 24
    got = _run(what, x, dy, align)
    assert _bits_equal(_canon(got), _canon(ref.to(dtype)))


def _assert_real(got, what, x, dy, align, dtype):
    ref = ub_ref(x, dy, align)[what == "bwd"]
    tol = bounds(x, dy, align, dtype)[what == "bwd"]
    err = (got.detach().cpu().double() - ref).abs()
    print(what, "max err", err.max().item(), "max tol", tol.max().item())
    assert not (err > tol).any(), "{} outside the bound".format(int((err > tol).sum()))


@gpu
@requires_gpu
def test_cases_reach_the_channel_chunks():
    ext_plan = _ext().upsample_bilinear_plan
    plan = ext_plan(2048, 2, 2, 4, 4, False, 2)
    assert plan["bwd_cc"] + 1 == CASES[-3][1] and plan["fwd_cc"] + 1 == CASES[-2][1]
    assert ext_plan(*CASES[-1][1:6], False, 4)["bwd_cols"] < CASES[-1][5]


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("what", ["fwd", "bwd"])
@pytest.mark.parametrize("case", [c for c in CASES if c[7]], ids=case_id)
def test_exact(case, what, dtype):
    for align in case[6]:
        if align and case[2:4] != (1, 1) and case[2:4] != case[4:6]:
            continue   # align_corners weights are dyadic only in these
        _assert_exact(case, what, dtype, align)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("what", ["fwd", "bwd"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_real(case, what, dtype):
    x, dy = inputs(case, dtype, exact=False)
    for align in case[6]:
        _assert_real(_run(what, x, dy, align), what, x, dy, align, dtype)


@gpu
@requires_gpu
@pytest.mark.parametrize("what", ["fwd", "bwd"])
def test_past_grid_cap(what):
    """A second, partial pass of the stride loop; ragged last tiles."""
    ext = _ext()
    info = ext.upsample_bilinear_info()
    th, tw = info[what + "_tile_h"], info[what + "_tile_w"]
    k = 2 if what == "fwd" else 1
    Hin, Win = (46 * th - k) // k, (45 * tw - k) // k
    case = (1, 1, Hin, Win, 2 * Hin, 2 * Win)
    tiles = ext.upsample_bilinear_plan(1, *case[2:], False, 2)[what + "_tiles"]
    assert info["max_grid"] < tiles < 2 * info["max_grid"]
    _assert_exact(case, what, BF16, False)


@gpu
@requires_gpu
def test_backward_deterministic():
    _, dy = inputs((3, 21, 3, 2, 48, 32), BF16, exact=False, seed=5)
    dy = dy.to(_DEV)
    a, b = (_ext().upsample_bilinear_bwd(dy, 3, 2, False) for _ in range(2))
    assert _bits_equal(a, b)


@gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    ext = _ext()
    fwd, bwd = ext.upsample_bilinear_fwd, ext.upsample_bilinear_bwd
    x = torch.zeros(2, 8, 4, 5, device=_DEV, dtype=BF16).contiguous(memory_format=CL)
    bad_calls = [
        ("upsample_bilinear_fwd: x must be a GPU", lambda: fwd(x.cpu(), 8, 10, False)),
        ("4-D", lambda: fwd(x[0], 8, 10, False)),
        ("bf16 or fp32", lambda: fwd(x.half(), 8, 10, False)),
        ("channels_last", lambda: fwd(x.contiguous(), 8, 10, False)),
        ("channels_last", lambda: bwd(x[:1, :1, :1, :1].expand_as(x), 2, 2, False)),
        ("16-byte aligned", lambda: fwd(_off_grid(x), 8, 10, False)),
        ("upscale only", lambda: fwd(x, 3, 10, False)),
        ("upscale only", lambda: bwd(x, 5, 5, False)),
        (r"sizes must be in \[1,", lambda: fwd(x, 8, 2 ** 31, False)),
        ("more than the kernels index", lambda: fwd(x, 2 ** 20, 2 ** 20, False)),
        ("at most 2048", lambda: fwd(torch.zeros(1, 2049, 1, 1, device=_DEV), 2, 2, False)),
    ]
    for match, call in bad_calls:
        with pytest.raises(RuntimeError, match=match):
            call()


@gpu
@requires_gpu
def test_empty_returns_empty():
    ext = _ext()
    for shape in ((0, 8, 4, 5), (2, 0, 4, 5)):
        x = torch.empty(*shape, device=_DEV, dtype=BF16)
        y = ext.upsample_bilinear_fwd(x, 8, 10, False)
        assert y.shape == shape[:2] + (8, 10) and y.dtype == BF16
        assert ext.upsample_bilinear_bwd(y, 4, 5, False).shape == shape


def _count_calls(monkeypatch):
    ext, calls = _ext(), []
    for n in ("upsample_bilinear_fwd", "upsample_bilinear_bwd"):
        orig = getattr(ext, n)
        monkeypatch.setattr(
            ext, n, lambda *a, _n=n, _o=orig: (calls.append(_n), _o(*a))[1])
    return calls


@gpu
@requires_gpu
def test_module_routes(monkeypatch):
    import tensorflowonspark_amd.ops.modules as M
    case = (2, 21, 5, 7, 13, 9)
    cx, cdy = inputs(case, BF16, exact=False)
    up = M.BilinearUpsample()
    calls = _count_calls(monkeypatch)
    in_tree = M._BilinearUpsampleFn.__name__ + "Backward"

    monkeypatch.setenv("TFOS_UPSAMPLE", "hip")
    x = cx.to(_DEV).requires_grad_()
    y = up(x, (13, 9))
    assert type(y.grad_fn).__name__ == in_tree
    y.sum().backward()      # the gradient arrives expanded (stride 0)
    assert calls == ["upsample_bilinear_fwd", "upsample_bilinear_bwd"]
    _assert_real(y, "fwd", cx, cdy, False, BF16)
    _assert_real(x.grad, "bwd", cx, torch.ones_like(cdy), False, BF16)
    del calls[:]
    for other in (up(x, (4, 9)),                          # a downscale
                  up(x.detach().contiguous().requires_grad_(), (13, 9)),
                  up(cx.requires_grad_(), (13, 9))):       # NCHW, CPU
        assert type(other.grad_fn).__name__ != in_tree
    monkeypatch.setenv("TFOS_UPSAMPLE", "aten")
    lib = up(x, (13, 9))
    assert type(lib.grad_fn).__name__ != in_tree and not calls
    monkeypatch.setenv("TFOS_UPSAMPLE", "fast")
    with pytest.raises(ValueError, match="TFOS_UPSAMPLE"):
        up(x, (13, 9))


@gpu
@requires_gpu
def test_deeplab_reaches_kernels(monkeypatch):
    from tensorflowonspark_amd.models.segmentation import DeepLabV3
    monkeypatch.setenv("TFOS_UPSAMPLE", "hip")
    model = DeepLabV3().to(_DEV).to(memory_format=CL)
    x = torch.randn(2, 3, 64, 64, device=_DEV).contiguous(memory_format=CL)
    calls = _count_calls(monkeypatch)
    with torch.autocast("cuda", dtype=BF16):
        out = model(x)
    assert out.shape == (2, 21, 64, 64) and out.dtype == BF16
    out.float().mean().backward()
    assert sorted(calls) == ["upsample_bilinear_bwd"] * 2 + ["upsample_bilinear_fwd"] * 2
