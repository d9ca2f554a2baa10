"""Transposed-conv weight gradient (csrc/convt_wrw.hip) against fp64.

Exact probes (convt_wrw_cases) must match bit for bit after -0 -> +0. Real
probes are held to M * 2^-23 * sum |x||dy| with M = N*H*W: the transposed-conv
head's dW bound, with no half-ulp term since dW stays fp32. What each shape
reaches is its id, asserted through the plan; docs/components.md
("Transposed-conv weight gradient coverage") has the table.
"""

import pytest
import torch

from convt_wrw_cases import BF16, CASES, CL, case, exact_premise, inputs, wrw_ref
from test_gpu_bn import _DEV, _bits_equal, _ext, _off_grid, gpu, requires_gpu


def _canon(t):
    """-0 -> +0: the sign of an exact zero depends on the summation's start
    value, which is not the kernel's business."""
    return t.cpu() + torch.zeros((), dtype=t.dtype)


def _assert_real(got, ref, aref, M):
    err = (got.detach().cpu().double() - ref).abs()
    tol = M * 2.0 ** -23 * aref
    print("max err {:.3e} max tol {:.3e}".format(err.max().item(),
                                                 tol.max().item()))
    bad = err > tol
    assert not bad.any(), "{} of {} outside the bound".format(
        int(bad.sum()), bad.numel())


@gpu
@requires_gpu
@pytest.mark.parametrize("name", CASES)
def test_exact(name):
    shape, reaches = CASES[name]
    N, cin, cout, H, W = shape
    assert reaches(_ext().convt_wrw_plan(N, H, W, cin, cout), N * H)
    assert exact_premise(*shape) < 2 ** 24
    x, dy, ref, _ = case(shape, True)
    dw = _ext().convt_wrw(dy.to(_DEV), x.to(_DEV))
    assert dw.shape == (cin, cout, 4, 4) and dw.is_contiguous()
    assert _bits_equal(_canon(dw), _canon(ref.float()))


@gpu
@requires_gpu
@pytest.mark.parametrize("name", CASES)
def test_real(name):
    shape = CASES[name][0]
    x, dy, ref, aref = case(shape, False)
    dw = _ext().convt_wrw(dy.to(_DEV), x.to(_DEV))
    _assert_real(dw, ref, aref, shape[0] * shape[3] * shape[4])


@gpu
@requires_gpu
def test_deterministic():
    x, dy = [t.to(_DEV) for t in inputs((2, 16, 24, 23, 9), False, seed=5)]
    assert _ext().convt_wrw_plan(2, 23, 9, 16, 24)["slabs"] > 1
    assert _bits_equal(_ext().convt_wrw(dy, x), _ext().convt_wrw(dy, x))


@gpu
@requires_gpu
def test_neighbours_are_not_read():
    """x and dy are channel slices of wider tensors, one image of three:
    NaNs sit in the channels past Cin / Cout of every pixel and in the images
    before and after."""
    shape = (1, 152, 72, 3, 5)
    x, dy, ref, _ = case(shape, True)

    def between_nans(t):
        big = torch.full((3, t.shape[1] + 8) + tuple(t.shape[2:]),
                         float("nan"), dtype=BF16,
                         device=_DEV).contiguous(memory_format=CL)
        view = big[1:2, :t.shape[1]]
        view.copy_(t)
        assert not view.is_contiguous(memory_format=CL)
        return view
    dw = _ext().convt_wrw(between_nans(dy), between_nans(x))
    assert _bits_equal(_canon(dw), _canon(ref.float()))


@gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    wrw = _ext().convt_wrw
    x, dy = [t.to(_DEV) for t in inputs((2, 16, 24, 5, 6), True)]
    act = lambda *sh: torch.zeros(*sh, device=_DEV, dtype=BF16).contiguous(  # noqa: E731
        memory_format=CL)
    bad_calls = [
        ("x must be a GPU tensor", lambda: wrw(dy, x.cpu())),
        ("dy must be a GPU tensor", lambda: wrw(dy.cpu(), x)),
        ("must be bf16", lambda: wrw(dy.float(), x)),
        ("must be bf16", lambda: wrw(dy, x.half())),
        ("4-D", lambda: wrw(dy[0], x)),
        ("channels_last", lambda: wrw(dy.contiguous(), x)),
        ("channels_last", lambda: wrw(dy, x.contiguous())),
        ("channels_last", lambda: wrw(dy, x[:1, :1, :1, :1].expand_as(x))),
        ("channels_last", lambda: wrw(dy, act(2, 16, 6, 5).transpose(2, 3))),
        ("pixel stride", lambda: wrw(dy, act(2, 20, 5, 6)[:, :16])),
        ("16-byte aligned", lambda: wrw(dy, _off_grid(x))),
        ("multiple of 8", lambda: wrw(dy, act(2, 12, 5, 6))),
        ("multiple of 8", lambda: wrw(act(2, 20, 10, 12), x)),
        ("gives a gradient of", lambda: wrw(dy[:1], x)),
        ("gives a gradient of", lambda: wrw(act(2, 24, 10, 13), x)),
        ("gives a gradient of", lambda: wrw(act(2, 24, 11, 12), x)),
        ("wider than", lambda: wrw(act(1, 8, 2, 758), act(1, 8, 1, 379))),
    ]
    for match, call in bad_calls:
        with pytest.raises(RuntimeError, match=match):
            call()
    dw = wrw(act(0, 24, 10, 12), act(0, 16, 5, 6))       # empty: zeros
    assert dw.shape == (16, 24, 4, 4) and dw.dtype == torch.float32
    assert not dw.any()
    torch.cuda.synchronize()


def _record(mp, fn):
    """Names of the extension entries fn() reaches, in order."""
    ext, trace = _ext(), []

    def wrap(name, orig):
        return lambda *a, **kw: (trace.append(name), orig(*a, **kw))[1]
    with mp.context() as m:
        for n in dir(ext):
            if not n.startswith("_") and callable(getattr(ext, n)):
                m.setattr(ext, n, wrap(n, getattr(ext, n)))
        fn()
        torch.cuda.synchronize()
    return trace


@gpu
@requires_gpu
@pytest.mark.parametrize("shape", [(2, 64, 96, 64, 64), (2, 152, 64, 5, 6)],
                         ids=["64to96_mfma_layer", "152to64_library_layer"])
def test_module_routes(monkeypatch, shape):
    """ConvTranspose2dMFMA under TFOS_CONVT_WRW, at a layer its MFMA path
    takes (the call-trace yardstick's shape) and at one it leaves to the
    library."""
    import tensorflowonspark_amd.ops.modules as M
    N, cin, cout, H, W = shape
    x, dy, ref, aref = case(shape, False)
    m = M.ConvTranspose2dMFMA(cin, cout, 4, 2, 1).to(_DEV)
    assert m._eligible == (cin % 32 == 0)

    def step():
        m.weight.grad = None
        xg = x.to(_DEV).requires_grad_()
        m(xg).backward(dy.to(_DEV))
        return xg.grad

    for mode, in_tree in (("hip", True), ("miopen", False), (None, False)):
        if mode is None:
            monkeypatch.delenv("TFOS_CONVT_WRW", raising=False)
        else:
            monkeypatch.setenv("TFOS_CONVT_WRW", mode)
        trace = _record(monkeypatch, step)
        assert ("convt_wrw" in trace) == in_tree, (mode, trace)
        assert m.weight.grad.dtype == torch.float32
        if in_tree:
            _assert_real(m.weight.grad, ref, aref, N * H * W)
        else:
            assert "convt_wrw_plan" not in trace
    monkeypatch.setenv("TFOS_CONVT_WRW", "fast")
    with pytest.raises(ValueError, match="TFOS_CONVT_WRW"):
        step()
