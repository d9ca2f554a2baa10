"""Transposed-conv head kernels (csrc/convt_head.hip) against fp64.

Exact probes (convt_head_cases) must match bit for bit: y and dx against the
bf16 rounding of the fp64 result, dw and db in fp32. Real-valued probes are
held to the project's MFMA bound

    K * 2^-23 * (|A| |B|^T) + half_ulp(out dtype)

with K = 4*Cin (fwd, plus 2^-24 |ref| for the fp32 bias add), 16*Cout (dgrad)
and M = N*H*W <= 512 for dw and db, which have no half-ulp term. Tiers and the
case that reaches each are listed in docs/components.md ("Transposed-conv
head coverage").
"""

import pytest
import torch

from convt_head_cases import (BF16, CL, FP32, ct_ref, exact_inputs,
                              exact_premise, real_inputs)
from test_gpu_bn import (_DEV, _bits_equal, _ext, _half_ulp, _off_grid, gpu,
                         requires_gpu)

# (N, Cin, Cout, H, W); "T" is the forward tile's interior side (14).
#   1x1            a 2x2 output, only the centre four taps live
#   3x5, 5x3       Cout = 3: output rows of 60 and 36 bytes, 2-byte aligned;
#                  N = 3: tiles and wrw K steps cross image boundaries
#   T, T+1         one forward tile exactly, and four (two dgrad tile rows)
#   9x17           two dgrad tile columns
#   Cin 8/80/256   one K step mostly padding / half-empty last / largest
#   Cout 1/8       one N tile / eight; 256x8 restages the weight per class
#                  (fwd) and per N tile (dgrad)
SHAPES = [
    (1, 80, 3, 1, 1), (1, 8, 1, 1, 1), (1, 80, 3, 3, 5), (3, 80, 3, 5, 3),
    (1, 8, 3, 3, 5), (3, 256, 3, 5, 3), (1, 80, 3, "T", "T"),
    (1, 80, 3, "T+1", "T+1"), (1, 8, 1, "T+1", "T+1"), (1, 8, 3, 9, 17),
    (2, 80, 8, 5, 3), (1, 256, 8, 3, 5), (3, 256, 1, 5, 3),
]
DIRECTIONS = ("fwd", "dgrad", "wrw")


def _shape(s):
    T = _ext().convt_head_info()["fwd_tile"]
    return tuple({"T": T, "T+1": T + 1}.get(v, v) for v in s)


def _canon(t):
    """-0 -> +0: the sign of an exact zero depends on the summation's start
    value, which is not the kernels' business."""
    return t.cpu() + torch.zeros((), dtype=t.dtype)


def _dev(*ts):
    return [t.to(_DEV) for t in ts]


def _assert_exact(shape, what, w_of=None):
    ext = _ext()
    N, cin, cout, H, W = shape
    assert max(exact_premise(*shape).values()) < 2 ** 24
    x, dy, w, b = exact_inputs(*shape)
    ry, rdx, rdw, rdb = ct_ref(x, w, b, dy)
    x, dy, w, b = _dev(x, dy, w, b)
    if w_of is not None:
        w = w_of(w)
    if what == "fwd":
        y = ext.convt_head_fwd(x, w, b)
        assert y.is_contiguous(memory_format=CL)
        assert _bits_equal(_canon(y), _canon(ry.to(BF16)))
    elif what == "dgrad":
        dx = ext.convt_head_dgrad(dy, w, H, W)
        assert dx.is_contiguous(memory_format=CL)
        assert _bits_equal(_canon(dx), _canon(rdx.to(BF16)))
    else:
        dw, db = ext.convt_head_wrw(dy, x)
        assert _bits_equal(_canon(dw), _canon(rdw.to(FP32))), "dw"
        assert _bits_equal(_canon(db), _canon(rdb.to(FP32))), "db"


def _assert_real(got, shape, x, w, b, dy):
    """got: dict of fwd/dgrad/dw/db results for real_inputs(*shape)."""
    N, cin, cout, H, W = shape
    M = N * H * W
    assert M <= 512
    ry, rdx, rdw, rdb = ct_ref(x, w, b, dy)
    ay, adx, adw, adb = ct_ref(x.abs(), w.abs(), b * 0, dy.abs())
    u = 2.0 ** -23
    bounds = {
        "fwd": (ry, 4 * cin * u * ay + _half_ulp(ry, BF16) + 2.0 ** -24 * ry.abs()),
        "dgrad": (rdx, 16 * cout * u * adx + _half_ulp(rdx, BF16)),
        "dw": (rdw, M * u * adw), "db": (rdb, M * u * adb)}
    for name, g in got.items():
        ref, tol = bounds[name]
        err = (g.detach().cpu().double() - ref).abs()
        print("{} max err {:.3e} max tol {:.3e}".format(
            name, err.max().item(), tol.max().item()))
        bad = err > tol
        assert not bad.any(), "{}: {} of {} outside the bound".format(
            name, int(bad.sum()), bad.numel())


_ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else s)


@gpu
@requires_gpu
@pytest.mark.parametrize("what", DIRECTIONS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact(shape, what):
    _assert_exact(_shape(shape), what)


@gpu
@requires_gpu
@pytest.mark.parametrize("what", DIRECTIONS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_real(shape, what):
    ext = _ext()
    shape = _shape(shape)
    cpu = real_inputs(*shape)
    x, dy, w, b = _dev(*cpu)
    if what == "fwd":
        got = {"fwd": ext.convt_head_fwd(x, w, b)}
    elif what == "dgrad":
        got = {"dgrad": ext.convt_head_dgrad(dy, w, shape[3], shape[4])}
    else:
        got = dict(zip(("dw", "db"), ext.convt_head_wrw(dy, x)))
    _assert_real(got, shape, cpu[0], cpu[2], cpu[3], cpu[1])


@gpu
@requires_gpu
@pytest.mark.parametrize("what", ["fwd", "dgrad"])
def test_past_grid_cap(what):
    """More tiles than max_grid by a ragged remainder: the stride loop runs a
    second, partial pass."""
    info = _ext().convt_head_info()
    th, tw = {"fwd": (info["fwd_tile"],) * 2,
              "dgrad": (info["dgrad_tile_h"], info["dgrad_tile_w"])}[what]
    side = 1
    while side * side <= info["max_grid"]:
        side += 1
    H, W = th * side - 1, tw * side - 1
    assert 0 < side * side % info["max_grid"] < info["max_grid"]
    assert H * W * (8 + 4) * 2 < 100e6
    _assert_exact((1, 8, 1, H, W), what)


@gpu
@requires_gpu
@pytest.mark.parametrize("tier", ["one", "ragged", "past_cap"])
def test_wrw_slabs(tier):
    ext = _ext()
    info = ext.convt_head_info()
    shape = {"one": (1, 8, 3, 9, 17), "ragged": (3, 80, 3, 23, 23),
             "past_cap": (1, 8, 1, 520, 520)}[tier]
    M = shape[0] * shape[3] * shape[4]
    plan = ext.convt_head_wrw_plan(M, shape[1], shape[2])
    if tier == "one":
        assert plan["nblk"] == 1 and M < info["wrw_min_pix"]
    elif tier == "ragged":
        assert 1 < plan["nblk"] < info["wrw_max_blocks"]
        assert M % plan["slab"] and plan["slab"] % (shape[3] * shape[4])
    else:
        assert plan["nblk"] == info["wrw_max_blocks"]
        assert plan["slab"] > info["wrw_min_pix"] and M % plan["slab"]
    assert (plan["nblk"] - 1) * plan["slab"] < M      # every slab non-empty
    _assert_exact(shape, "wrw")


@gpu
@requires_gpu
def test_wrw_deterministic():
    ext = _ext()
    x, dy, _, _ = _dev(*real_inputs(3, 80, 3, 23, 23, seed=5))
    a, b = ext.convt_head_wrw(dy, x), ext.convt_head_wrw(dy, x)
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])


@gpu
@requires_gpu
@pytest.mark.parametrize("what", ["fwd", "dgrad"])
def test_weight_view_in_flat_bucket(what):
    """A DDP engine keeps parameters as views into one flat buffer: the
    weight may start at any 4-byte offset."""
    def view(w):
        flat = torch.zeros(w.numel() + 1, device=_DEV)
        wv = flat[1:].view_as(w)
        wv.copy_(w)
        assert wv.data_ptr() % 16 != 0 and wv.is_contiguous()
        return wv
    _assert_exact((2, 80, 3, 5, 3), what, w_of=view)


@gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    ext = _ext()
    x, dy, w, b = _dev(*exact_inputs(2, 16, 3, 5, 6))
    z = lambda *sh: torch.zeros(*sh, device=_DEV)  # noqa: E731
    fwd, dgrad, wrw = ext.convt_head_fwd, ext.convt_head_dgrad, ext.convt_head_wrw
    bad_calls = [
        ("GPU tensor", lambda: fwd(x.cpu(), w, b)),
        ("GPU tensor", lambda: wrw(dy, x.cpu())),
        ("weight must be on", lambda: fwd(x, w.cpu(), b)),
        ("must be bf16", lambda: fwd(x.float(), w, b)),
        ("must be bf16", lambda: dgrad(dy.float(), w, 5, 6)),
        ("channels_last", lambda: fwd(x.contiguous(), w, b)),
        ("channels_last", lambda: wrw(dy.contiguous(), x)),
        ("channels_last", lambda: dgrad(dy[:1, :1, :1, :1].expand_as(dy), w, 5, 6)),
        ("16-byte aligned", lambda: fwd(_off_grid(x), w, b)),
        ("4-D", lambda: fwd(x[0], w, b)),
        (r"\[Cin,Cout,4,4\]", lambda: fwd(x, w.to(BF16), b)),
        (r"\[Cin,Cout,4,4\]", lambda: fwd(x, w[:8].contiguous(), b)),
        (r"\[Cin,Cout,4,4\]", lambda: dgrad(dy, z(16, 3, 3, 3), 5, 6)),
        (r"\[Cin,Cout,4,4\]", lambda: dgrad(dy, w[:, :2].contiguous(), 5, 6)),
        ("bias must be", lambda: fwd(x, w, b.to(BF16))),
        ("bias must be", lambda: fwd(x, w, b[:2])),
        ("multiple of 8", lambda: fwd(z(1, 12, 2, 2).to(BF16).contiguous(
            memory_format=CL), z(12, 3, 4, 4), b)),
        ("multiple of 8", lambda: fwd(z(1, 264, 2, 2).to(BF16).contiguous(
            memory_format=CL), z(264, 3, 4, 4), b)),
        (r"in \[1, 8\]", lambda: fwd(x, z(16, 9, 4, 4), None)),
        ("the gradient is", lambda: dgrad(dy, w, 6, 5)),
        ("gives a gradient of", lambda: wrw(dy[:1], x)),
        ("gives a gradient of", lambda: wrw(
            dy[:, :, :8].contiguous(memory_format=CL), x)),
    ]
    for match, call in bad_calls:
        with pytest.raises(RuntimeError, match=match):
            call()
    ext.convt_head_fwd(x, w, None)       # the bias is optional
    torch.cuda.synchronize()


@gpu
@requires_gpu
def test_empty_returns_empty():
    ext = _ext()
    w = torch.ones(16, 3, 4, 4, device=_DEV)
    x = torch.empty(0, 16, 5, 6, device=_DEV, dtype=BF16)
    y = ext.convt_head_fwd(x, w, None)
    assert y.shape == (0, 3, 10, 12) and y.dtype == BF16
    assert ext.convt_head_dgrad(y, w, 5, 6).shape == (0, 16, 5, 6)
    dw, db = ext.convt_head_wrw(y, x)
    assert dw.shape == (16, 3, 4, 4) and dw.dtype == FP32 and not dw.any()
    assert db.shape == (3,) and not db.any()


_ENTRIES = ("convt_head_fwd", "convt_head_dgrad", "convt_head_wrw")


def _module_case(shape=(3, 80, 3, 5, 3)):
    from tensorflowonspark_amd.ops.modules import ConvTranspose2dHead
    cpu = real_inputs(*shape)
    x, dy, w, b = _dev(*cpu)
    m = ConvTranspose2dHead(shape[1], shape[2]).to(_DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    return m, x.requires_grad_(), dy, cpu


def _count_calls(monkeypatch):
    ext, calls = _ext(), []
    for n in _ENTRIES:
        orig = getattr(ext, n)
        monkeypatch.setattr(
            ext, n, lambda *a, _n=n, _o=orig: (calls.append(_n), _o(*a))[1])
    return calls


@gpu
@requires_gpu
@pytest.mark.parametrize("route", [(True, True, True), (True, False, False),
                                   (False, True, False), (True, False, True),
                                   (False, False, True)],
                         ids=lambda r: "".join("hl"[not f] for f in r))
def test_module_routes(monkeypatch, route):
    """All in-tree ('hip') and every mix with the library give results inside
    the real-valued bound; the library's own bf16 bias is the one difference
    the forward bound has to leave room for, so mixed forwards are checked
    in-tree only."""
    import tensorflowonspark_amd.ops.modules as M
    if all(route):
        monkeypatch.setenv("TFOS_CONVT_HEAD", "hip")
    else:
        monkeypatch.setenv("TFOS_CONVT_HEAD", "auto")
        monkeypatch.setattr(M, "_cth_auto",
                            lambda d, *a: route[DIRECTIONS.index(d)])
    m, x, dy, (cx, cdy, cw, cb) = _module_case()
    calls = _count_calls(monkeypatch)
    y = m(x)
    assert type(y.grad_fn).__name__ == M._ConvTHeadFn.__name__ + "Backward"
    y.backward(dy)
    assert calls == [n for n, f in zip(_ENTRIES, route) if f]
    assert m.weight.grad.dtype == FP32 and m.bias.grad.dtype == FP32
    got = {"dgrad": x.grad, "dw": m.weight.grad, "db": m.bias.grad}
    if route[0]:
        got["fwd"] = y
    for d, name in ((1, "dgrad"), (2, "dw"), (2, "db")):
        if not route[d]:
            del got[name]
    _assert_real(got, (3, 80, 3, 5, 3), cx, cw, cb, cdy)


@gpu
@requires_gpu
def test_module_library_routes(monkeypatch):
    monkeypatch.setenv("TFOS_CONVT_HEAD", "miopen")
    m, x, _, _ = _module_case()
    with torch.autocast("cuda", dtype=BF16):
        y = m(x)
    assert "ConvTHead" not in type(y.grad_fn).__name__
    monkeypatch.setenv("TFOS_CONVT_HEAD", "hip")
    y = m(x.detach().float())                 # fp32 activations
    assert y.dtype == FP32 and "ConvTHead" not in type(y.grad_fn).__name__
    m9, x9, _, _ = _module_case((1, 16, 9, 3, 3))   # Cout = 9
    with torch.autocast("cuda", dtype=BF16):
        y = m9(x9)
    assert y.dtype == BF16 and "ConvTHead" not in type(y.grad_fn).__name__


@gpu
@requires_gpu
def test_module_sum_backward_and_needs_input_grad(monkeypatch):
    """y.sum().backward(): the gradient arrives expanded (stride 0)."""
    monkeypatch.setenv("TFOS_CONVT_HEAD", "hip")
    m, x, _, (cx, cdy, cw, cb) = _module_case()
    calls = _count_calls(monkeypatch)
    with torch.autocast("cuda", dtype=BF16):
        y = m(x.detach().float().requires_grad_(False))   # cast, no grad for x
    y.sum().backward()
    assert calls == ["convt_head_fwd", "convt_head_wrw"]
    _assert_real({"dw": m.weight.grad, "db": m.bias.grad}, (3, 80, 3, 5, 3),
                 cx, cw, cb, torch.ones_like(cdy))
    del calls[:]
    m.weight.requires_grad_(False)
    m.bias.requires_grad_(False)
    m(x).sum().backward()
    assert calls == ["convt_head_fwd", "convt_head_dgrad"]
    _assert_real({"dgrad": x.grad}, (3, 80, 3, 5, 3), cx, cw, cb,
                 torch.ones_like(cdy))
