"""Pointwise-conv kernels (csrc/pwconv.hip) against fp64.

Exact probes (pwconv_cases) must match bit for bit: y and dx against the bf16
rounding of the fp64 result. Real-valued probes are held to the project's
MFMA bound

    K * 2^-23 * (|A| |B|^T) + half_ulp(bf16)

with K = Cin (fwd), Cout (dgrad) and, for the dw that PointwiseConv takes
from conv_wrw2, M = N*H*W <= 512 without the half-ulp term. Tiers and the
case that reaches each are listed in docs/components.md ("Pointwise conv
coverage").
"""

import pytest
import torch

from pwconv_cases import (BF16, CL, FP32, SHAPES, exact_inputs, exact_premise,
                          pw_ref, real_inputs)
from tensorflowonspark_amd.ops.modules import PointwiseConv
from test_gpu_bn import (_DEV, _bits_equal, _ext, _half_ulp, _off_grid, gpu,
                         requires_gpu)

DIRECTIONS = ("fwd", "dgrad")
_ENTRIES = ("pwconv_fwd", "pwconv_dgrad", "conv_wrw2")


def _shape(s):
    T = _ext().pwconv_info()["tile_m"]
    return tuple({"T": T, "T+1": T + 1}.get(v, v) for v in s)


def _canon(t):
    """-0 -> +0: the sign of an exact zero depends on the summation's start
    value, which is not the kernels' business."""
    return t.cpu() + torch.zeros((), dtype=t.dtype)


def _run(what, x, dy, w):
    ext = _ext()
    return ext.pwconv_fwd(x, w) if what == "fwd" else ext.pwconv_dgrad(dy, w)


def _assert_exact(shape, what, place=lambda t: t.to(_DEV)):
    assert exact_premise(*shape)[what] < 2 ** 24
    x, dy, w = exact_inputs(*shape)
    ref = pw_ref(x, w, dy)[DIRECTIONS.index(what)]
    got = _run(what, place(x), place(dy), w.to(_DEV))
    assert got.is_contiguous(memory_format=CL)
    assert _bits_equal(_canon(got), _canon(ref.to(BF16)))


def _assert_real(got, x, w, dy):
    """got: {direction: result} for CPU inputs x, w, dy with M <= 512."""
    M = x.numel() // x.shape[1]
    assert M <= 512
    K = {"fwd": x.shape[1], "dgrad": dy.shape[1], "wrw": M}
    names = DIRECTIONS + ("wrw",)
    refs = dict(zip(names, pw_ref(x, w, dy)))
    mags = dict(zip(names, pw_ref(x.abs(), w.abs(), dy.abs())))
    for name, g in got.items():
        ref = refs[name]
        tol = K[name] * 2.0 ** -23 * mags[name]
        if name != "wrw":
            tol = tol + _half_ulp(ref, BF16)
        err = (g.detach().cpu().double().reshape(ref.shape) - ref).abs()
        print("{} max err {:.3e} max tol {:.3e}".format(
            name, err.max().item(), tol.max().item()))
        bad = err > tol
        assert not bad.any(), "{}: {} of {} outside the bound".format(
            name, int(bad.sum()), bad.numel())


def _cases():
    return [pytest.param(s, d, id="{}-{}".format("x".join(map(str, s)), d))
            for s in SHAPES for d in DIRECTIONS]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,what", _cases())
def test_exact(shape, what):
    _assert_exact(_shape(shape), what)


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,what", _cases())
def test_real(shape, what):
    x, dy, w = real_inputs(*_shape(shape))
    got = _run(what, x.to(_DEV), dy.to(_DEV), w.to(_DEV))
    _assert_real({what: got}, x, w, dy)


@gpu
@requires_gpu
@pytest.mark.parametrize("what", DIRECTIONS)
def test_past_grid_cap(what):
    """More M tiles than max_grid by a ragged remainder: the stride loop runs
    a second, partial pass."""
    ext = _ext()
    info = ext.pwconv_info()
    T = info["tile_m"]
    M = (info["max_grid"] + 5) * T + 3
    plan = ext.pwconv_plan(M, 8, 8)
    assert info["max_grid"] < plan["m_tiles"] < 2 * info["max_grid"]
    assert M % T and plan["grid"] == info["max_grid"]
    _assert_exact((1, 8, 8, 1, M), what)


@gpu
@requires_gpu
@pytest.mark.parametrize("what", DIRECTIONS)
def test_neighbours_are_not_read(what):
    """The operands sit between NaNs: a ragged-K or ragged-M fragment that is
    masked on one operand only would bring one into the result."""
    def between_nans(t):
        big = torch.full((3,) + tuple(t.shape[1:]), float("nan"), dtype=BF16,
                         device=_DEV).contiguous(memory_format=CL)
        big[1:2].copy_(t)
        assert big[1:2].is_contiguous(memory_format=CL)
        return big[1:2]
    _assert_exact(_shape((1, 24, 16, 1, "T+1")), what, place=between_nans)


@gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    ext = _ext()
    x, dy, w = [t.to(_DEV) for t in exact_inputs(2, 16, 24, 5, 6)]
    fwd, dgrad = ext.pwconv_fwd, ext.pwconv_dgrad
    act = lambda *sh: torch.zeros(*sh, device=_DEV, dtype=BF16).contiguous(  # noqa: E731
        memory_format=CL)
    bad_calls = [
        ("pwconv_fwd: x must be a GPU tensor", lambda: fwd(x.cpu(), w)),
        ("pwconv_dgrad: dy must be a GPU tensor", lambda: dgrad(dy.cpu(), w)),
        ("pwconv_fwd: weight must be on", lambda: fwd(x, w.cpu())),
        ("must be bf16", lambda: fwd(x.float(), w)),
        ("must be bf16", lambda: dgrad(dy.float(), w)),
        ("channels_last", lambda: fwd(x.contiguous(), w)),
        ("channels_last", lambda: dgrad(dy[:1, :1, :1, :1].expand_as(dy), w)),
        ("16-byte aligned", lambda: fwd(_off_grid(x), w)),
        ("4-D", lambda: fwd(x[0], w)),
        (r"\[Cout,Cin,1,1\]", lambda: fwd(x, w.half())),
        (r"\[Cout,Cin,1,1\]", lambda: fwd(x, w[:, :, 0, 0])),
        (r"\[Cout,Cin,1,1\]", lambda: fwd(x, w[:, :8].contiguous())),
        (r"\[Cout,Cin,1,1\]", lambda: dgrad(dy, w[:8].contiguous())),
        ("multiple of 8", lambda: fwd(act(1, 12, 2, 2), w)),
        ("multiple of 8", lambda: fwd(act(1, 968, 2, 2),
                                      torch.zeros(8, 968, 1, 1, device=_DEV))),
        ("multiple of 8", lambda: fwd(x, torch.zeros(12, 16, 1, 1, device=_DEV))),
    ]
    for match, call in bad_calls:
        with pytest.raises(RuntimeError, match=match):
            call()
    e = torch.empty(0, 16, 5, 6, device=_DEV, dtype=BF16)
    y = fwd(e, w)
    assert y.shape == (0, 24, 5, 6) and y.dtype == BF16
    assert dgrad(y, w).shape == (0, 16, 5, 6)
    fwd(x, w.to(BF16))                  # a bf16 parameter is taken as it is
    torch.cuda.synchronize()


def _count_calls(monkeypatch):
    ext, calls = _ext(), []
    for n in _ENTRIES:
        orig = getattr(ext, n)
        monkeypatch.setattr(
            ext, n, lambda *a, _n=n, _o=orig, **k: (calls.append(_n), _o(*a, **k))[1])
    return calls


@gpu
@requires_gpu
@pytest.mark.parametrize("pair", [(24, 144), (192, 64)],
                         ids=lambda p: "x".join(map(str, p)))
def test_module_routes(monkeypatch, pair):
    wrw = "conv_wrw2"
    shape = (2, pair[0], pair[1], 3, 3)
    cx, _, cw = real_inputs(*shape)
    m = PointwiseConv(*pair).to(_DEV)
    with torch.no_grad():
        m.weight.copy_(cw)
    calls = _count_calls(monkeypatch)

    def step(x):
        m.weight.grad = None
        x = x.to(_DEV).requires_grad_()
        with torch.autocast("cuda", dtype=BF16):
            y = m(x)
        y.float().sum().backward()      # the gradient arrives expanded
        return x, y

    monkeypatch.setenv("TFOS_PW", "hip")
    x, y = step(cx.float())             # fp32 in, autocast decides
    assert calls == ["pwconv_fwd", "pwconv_dgrad", wrw]
    assert y.dtype == BF16 and m.weight.grad.dtype == FP32
    _assert_real({"fwd": y, "dgrad": x.grad, "wrw": m.weight.grad}, cx, cw,
                 torch.ones(shape[0], pair[1], 3, 3))
    del calls[:]
    step(cx.float().contiguous())       # NCHW in: made channels_last
    assert calls == ["pwconv_fwd", "pwconv_dgrad", wrw]
    del calls[:]
    monkeypatch.setenv("TFOS_PW", "fast")
    with pytest.raises(ValueError, match="TFOS_PW"):
        step(cx.float())
    monkeypatch.setenv("TFOS_PW", "miopen")
    step(cx.float())
    monkeypatch.setenv("TFOS_PW", "hip")
    m.cpu()(cx.float())                 # a CPU input takes the library path
    assert calls == []


@gpu
@requires_gpu
def test_unet_reaches_kernels(monkeypatch):
    from tensorflowonspark_amd.models import unet_mobilenet
    monkeypatch.setenv("TFOS_PW", "hip")
    torch.manual_seed(0)
    model = unet_mobilenet().to(_DEV).train()
    layers = sum(isinstance(m, PointwiseConv) for m in model.modules())
    calls = _count_calls(monkeypatch)
    x = torch.randn(2, 3, 64, 64, device=_DEV).contiguous(memory_format=CL)
    with torch.autocast("cuda", dtype=BF16):
        out = model(x)
    out.float().square().mean().backward()
    assert layers == 33 and calls.count("pwconv_fwd") == layers
    assert calls.count("pwconv_dgrad") == layers
    assert calls.count("conv_wrw2") == layers
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
