"""Dense softmax cross-entropy kernels (csrc/softmax_xent_dense.hip) vs the
defining formulas in fp64.

    loss_i  = lse_i - (1-eps) * x[i, t_i] - (eps/C) * sum_c x[i, c]
    dlogits = (softmax(x)_ic - (1-eps) * [c == t_i] - eps/C) * g_i

evaluated in fp64 on the device, on exactly the values the kernel sees (inputs
already rounded to the test dtype). A row is ignored when its target equals
ignore_index or lies outside [0, C): it must give exactly 0 loss and a
bit-zero gradient. ``mean`` divides by the number of rows that are not
ignored, or by 1 when there is none.

Tolerances follow the rule of tests/test_gpu_bn.py and come from the
reference alone. For each compared quantity q (per-row loss, lse, reduced
loss, dlogits):

    bound(q) = 16 * max|ref32(q) - ref64(q)|  +  half_ulp(out dtype) * |ref64(q)|

with ref32 the same helper run in fp32, and half_ulp 2^-24 * |ref64| for fp32
outputs and the exact 2^(e-9) of |ref64|'s binade for bf16 outputs.

Every kernel family is reached through the extension entry points (which also
return lse and accept max_grid, so that a small shape makes the grid-stride
loops iterate) and again through the public function and autograd.
"""

import pytest
import torch

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

BF16 = torch.bfloat16
FP32 = torch.float32
_DEV = "cuda"
ROWS2D, NCHW, NHWC = "2d", "nchw", "nhwc"
REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}
G_SCALAR = 0.75          # upstream gradient of the reduced forms


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _half_ulp(ref64, dtype):
    if dtype == BF16:
        _, e = torch.frexp(ref64)
        half = torch.ldexp(torch.ones_like(ref64), e - 9)
        return torch.where(ref64 == 0, torch.zeros_like(ref64), half)
    return 2.0 ** -24 * ref64.abs()


def _check(what, got, ref64, ref32, out_dtype):
    """|got - ref64| <= bound elementwise; prints the figures first."""
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), "{}: non-finite values".format(what)
    got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
    ref_err = (ref32.double() - ref64).abs().max()
    tol = 16.0 * ref_err + _half_ulp(ref64, out_dtype)
    err = (got.double() - ref64).abs()
    worst = (err - tol).argmax()
    print("  {:<14s} err max {:.3e}  ref32-vs-fp64 max {:.3e}  "
          "worst err/bound {:.3e}/{:.3e}".format(
              what, err.max().item(), ref_err.item(), err[worst].item(),
              tol[worst].item()))
    assert (err <= tol).all(), "{}: err {:.3e} > bound {:.3e}".format(
        what, err[worst].item(), tol[worst].item())


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _rows(t, layout):
    """The logits-shaped tensor t as (P, C) rows in target order."""
    if layout == ROWS2D:
        return t
    return t.movedim(1, -1).reshape(-1, t.shape[1])


def _make(shape, dtype, layout, ignore_index, seed=0):
    """Logits in ``layout`` rounded to ``dtype``, and the target.

    Every class has its own offset in [-4, 4], one row has entries near +-60,
    the targets cycle through all classes, about a quarter of the rows are
    ignored (the first, the last and a run of 9 among them) and one target is
    C + 2."""
    C = shape[1]
    P = 1
    for d in (shape[:1] + shape[2:]):
        P *= d
    gen = torch.Generator().manual_seed(seed + 1000 * C + P)
    offs = -4.0 + 8.0 * torch.randperm(C, generator=gen).float() / max(C - 1, 1)
    x = torch.randn(P, C, generator=gen) * 3 + offs
    big = P // 2
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    sign[0] = 1.0
    x[big] = sign * 60.0 + torch.randn(C, generator=gen)
    t = (torch.arange(P) + int(torch.randint(0, C, (1,), generator=gen))) % C
    t = t[torch.randperm(P, generator=gen)] if P > C else t
    ign = torch.rand(P, generator=gen) < 0.2
    ign[0] = True
    ign[-1] = True
    if P >= 16:
        ign[3:12] = True
    if P > 1:
        ign[big] = False
    t[ign] = ignore_index
    if P >= 3:
        t[1 if big != 1 else 2] = C + 2      # out of range, not ignore_index
    x = x.to(_DEV).to(dtype)
    t = t.to(_DEV)
    if layout == ROWS2D:
        return x, t
    N, sp = shape[0], tuple(shape[2:])
    x = x.view(N, *sp, C).movedim(-1, 1)
    x = x.contiguous() if layout == NCHW else \
        x.contiguous(memory_format=torch.channels_last)
    return x, t.view(N, *sp)


def _ref(dt, rows, t, ignore_index, eps, g_rows):
    """The formulas in dtype ``dt`` for all three reductions. The per-row
    upstream gradient of ``none`` is g_rows; sum and mean get G_SCALAR."""
    X = rows.to(dt)
    C = X.shape[1]
    t = t.reshape(-1)
    valid = (t != ignore_index) & (t >= 0) & (t < C)
    tc = torch.where(valid, t, torch.zeros_like(t))
    m = X.max(dim=1).values
    lse = m + torch.log(torch.exp(X - m[:, None]).sum(dim=1))
    xt = X.gather(1, tc[:, None])[:, 0]
    loss = lse - (1 - eps) * xt - (eps / C) * X.sum(dim=1)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    n = valid.sum().clamp(min=1).to(dt)
    onehot = torch.zeros_like(X).scatter_(1, tc[:, None], 1.0)
    core = torch.exp(X - lse[:, None]) - (1 - eps) * onehot - eps / C
    core = torch.where(valid[:, None], core, torch.zeros_like(core))
    gs = torch.tensor(G_SCALAR, dtype=dt, device=X.device)
    return {
        "valid": valid, "lse": lse,
        "none": loss, "sum": loss.sum(), "mean": loss.sum() / n,
        "d_none": core * g_rows.to(dt)[:, None],
        "d_sum": core * gs, "d_mean": core * (gs / n),
    }


def _bit_zero(t):
    return (t.contiguous().view(torch.int16 if t.dtype == BF16
                                else torch.int32) == 0).all()


def _run_case(shape, dtype, layout, eps, max_grid=0, reductions=REDUCTIONS):
    """One shape through the extension entry points, every reduction."""
    ext = _ext()
    ignore_index = 255 if dtype == BF16 else -100
    x, t = _make(shape, dtype, layout, ignore_index)
    rows = _rows(x, layout)
    P = rows.shape[0]
    g_rows = torch.randn(P, device=_DEV,
                         generator=torch.Generator(_DEV).manual_seed(5))
    r64 = _ref(torch.float64, rows, t, ignore_index, eps, g_rows)
    r32 = _ref(torch.float32, rows, t, ignore_index, eps, g_rows)
    ign = ~r64["valid"]
    assert ign[0] and ign[-1]
    for red in reductions:
        code = REDUCTIONS[red]
        loss, lse, nvalid = ext.xent_dense_fwd(x, t, ignore_index, eps, code,
                                               max_grid)
        assert loss.dtype == FP32 and lse.dtype == FP32
        _check("lse/" + red, lse, r64["lse"], r32["lse"], FP32)
        if red == "none":
            assert loss.shape == t.shape
            assert (loss.reshape(-1)[ign] == 0).all()
            gout = g_rows.view(t.shape)
        else:
            assert loss.dim() == 0
            assert int(nvalid.item()) == int(r64["valid"].sum().item())
            gout = torch.tensor(G_SCALAR, device=_DEV)
        _check("loss/" + red, loss.reshape(-1), r64[red].reshape(-1),
               r32[red].reshape(-1), FP32)
        dl = ext.xent_dense_bwd(x, lse, t, gout,
                                None if red == "none" else nvalid,
                                ignore_index, eps, code, max_grid)
        assert dl.dtype == dtype and dl.shape == x.shape
        assert dl.stride() == x.stride()
        dl_rows = _rows(dl, layout)
        assert _bit_zero(dl_rows[ign]), "ignored rows must have bit-zero grads"
        _check("dlogits/" + red, dl_rows, r64["d_" + red], r32["d_" + red],
               dtype)
    return x, t, r64, r32, g_rows, ignore_index


def _run_public(shape, dtype, layout, eps):
    """The same shape through softmax_cross_entropy and autograd: none with a
    per-row upstream, sum, and mean with a non-unit scalar upstream."""
    from tensorflowonspark_amd.ops.modules import softmax_cross_entropy
    ignore_index = 255 if dtype == BF16 else -100
    x, t = _make(shape, dtype, layout, ignore_index)
    rows = _rows(x, layout)
    g_rows = torch.randn(rows.shape[0], device=_DEV,
                         generator=torch.Generator(_DEV).manual_seed(5))
    r64 = _ref(torch.float64, rows, t, ignore_index, eps, g_rows)
    r32 = _ref(torch.float32, rows, t, ignore_index, eps, g_rows)
    for red in REDUCTIONS:
        leaf = x.detach().clone(memory_format=torch.preserve_format) \
            .requires_grad_()
        loss = softmax_cross_entropy(leaf, t, reduction=red,
                                     ignore_index=ignore_index,
                                     label_smoothing=eps)
        _check("loss/" + red, loss.reshape(-1), r64[red].reshape(-1),
               r32[red].reshape(-1), FP32)
        saved = loss.grad_fn.saved_tensors[0]
        assert saved.data_ptr() == leaf.data_ptr(), "logits were copied"
        if red == "none":
            (loss * g_rows.view(t.shape)).sum().backward()
        else:
            (loss * G_SCALAR).backward()
        _check("dlogits/" + red, _rows(leaf.grad, layout), r64["d_" + red],
               r32["d_" + red], dtype)
        assert _bit_zero(_rows(leaf.grad, layout)[~r64["valid"]])


DTYPES = pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
EPS = pytest.mark.parametrize("eps", [0.0, 0.1], ids=["eps0", "eps0.1"])


# ---------------------------------------------------------------------------
# tile family: class-contiguous rows, C < 64
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@DTYPES
@EPS
@pytest.mark.parametrize("C", [2, 3, 21, 63])
@pytest.mark.parametrize("P", [1, 37, 4099])
def test_tile_2d(P, C, dtype, eps):
    # 4099 is prime: more than one tile, a ragged last tile and an element
    # count that is no multiple of 8, for every tile height
    _run_case((P, C), dtype, ROWS2D, eps)


@gpu
@requires_gpu
@DTYPES
@EPS
@pytest.mark.parametrize("shape", [(2, 21, 5, 7), (3, 3, 16, 16)])
def test_tile_channels_last(shape, dtype, eps):
    _run_case(shape, dtype, NHWC, eps)
    _run_public(shape, dtype, NHWC, eps)


@gpu
@requires_gpu
@DTYPES
@EPS
def test_tile_grid_stride(dtype, eps):
    _run_case((4099, 3), dtype, ROWS2D, eps, max_grid=2)


# ---------------------------------------------------------------------------
# strided family: standard-contiguous (N, C, H, W)
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@DTYPES
@EPS
@pytest.mark.parametrize("shape", [(2, 21, 8, 8),      # 16 B vector path
                                   (3, 5, 7, 9),       # scalar path
                                   (2, 70, 4, 4)])     # C >= 64, still strided
def test_strided_nchw(shape, dtype, eps):
    _run_case(shape, dtype, NCHW, eps)
    _run_public(shape, dtype, NCHW, eps)


@gpu
@requires_gpu
@DTYPES
@EPS
def test_strided_grid_stride(dtype, eps):
    _run_case((2, 21, 8, 8), dtype, NCHW, eps, max_grid=1)


# ---------------------------------------------------------------------------
# rows family: one block per row, C >= 64
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@DTYPES
@EPS
@pytest.mark.parametrize("shape,max_grid", [((33, 64), 0), ((64, 1000), 0),
                                            ((5, 100), 0), ((64, 1000), 2)])
def test_rows(shape, max_grid, dtype, eps):
    _run_case(shape, dtype, ROWS2D, eps, max_grid=max_grid)
    if max_grid == 0:
        _run_public(shape, dtype, ROWS2D, eps)


# ---------------------------------------------------------------------------
# routing and the further properties
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@DTYPES
@EPS
def test_noncontiguous_4d(dtype, eps):
    """A [..., ::2] slice is neither contiguous nor channels_last: the public
    function makes it contiguous and the gradient reaches the base tensor."""
    from tensorflowonspark_amd.ops.modules import softmax_cross_entropy
    ignore_index = 255
    wide, _ = _make((2, 21, 8, 16), dtype, NCHW, ignore_index, seed=7)
    _, t = _make((2, 21, 8, 8), dtype, NCHW, ignore_index)
    leaf = wide.detach().clone().requires_grad_()
    x = leaf[..., ::2]
    assert not x.is_contiguous()
    rows = _rows(x.detach(), NCHW)
    g_rows = torch.zeros(rows.shape[0], device=_DEV)
    r64 = _ref(torch.float64, rows, t, ignore_index, eps, g_rows)
    r32 = _ref(torch.float32, rows, t, ignore_index, eps, g_rows)
    loss = softmax_cross_entropy(x, t, ignore_index=ignore_index,
                                 label_smoothing=eps)
    _check("loss/mean", loss.reshape(-1), r64["mean"].reshape(-1),
           r32["mean"].reshape(-1), FP32)
    (loss * G_SCALAR).backward()
    _check("dlogits/mean", _rows(leaf.grad[..., ::2], NCHW), r64["d_mean"],
           r32["d_mean"], dtype)
    assert (leaf.grad[..., 1::2] == 0).all()


FAMILY_SHAPES = [((37, 21), ROWS2D), ((2, 21, 8, 8), NCHW), ((33, 64), ROWS2D)]
FAMILY_IDS = ["tile", "strided", "rows"]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,layout", FAMILY_SHAPES, ids=FAMILY_IDS)
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_all_ignored(shape, layout, reduction):
    from tensorflowonspark_amd.ops.modules import softmax_cross_entropy
    x, t = _make(shape, BF16, layout, 255)
    t = torch.full_like(t, 255)
    leaf = x.detach().clone().requires_grad_()
    loss = softmax_cross_entropy(leaf, t, reduction=reduction,
                                 ignore_index=255, label_smoothing=0.1)
    assert (loss == 0).all() and torch.isfinite(loss).all()
    loss.sum().backward()
    assert _bit_zero(leaf.grad)


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,layout", FAMILY_SHAPES, ids=FAMILY_IDS)
def test_deterministic(shape, layout):
    """No floating-point atomics: the same call twice gives the same bits."""
    ext = _ext()
    x, t = _make(shape, BF16, layout, 255)
    g = torch.tensor(G_SCALAR, device=_DEV)
    outs = []
    for _ in range(2):
        loss, lse, nv = ext.xent_dense_fwd(x, t, 255, 0.1, 2, 0)
        dl = ext.xent_dense_bwd(x, lse, t, g, nv, 255, 0.1, 2, 0)
        outs.append((loss, lse, dl))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@gpu
@requires_gpu
@pytest.mark.parametrize("shape", [(0, 21), (0, 100), (2, 21, 0, 4)])
def test_empty_input(shape):
    """No rows: nothing is launched, mean and sum are 0, shapes hold."""
    from tensorflowonspark_amd.ops.modules import softmax_cross_entropy
    x = torch.zeros(shape, device=_DEV, requires_grad=True)
    t = torch.zeros(shape[:1] + shape[2:], dtype=torch.long, device=_DEV)
    assert softmax_cross_entropy(x, t, reduction="none").shape == t.shape
    loss = softmax_cross_entropy(x, t)
    assert loss.item() == 0.0
    loss.backward()
    assert x.grad.shape == x.shape


@gpu
@requires_gpu
def test_binding_checks():
    ext = _ext()
    x, t = _make((37, 21), FP32, ROWS2D, -100)
    with pytest.raises(RuntimeError):
        ext.xent_dense_fwd(x, t.int(), -100, 0.0, 0, 0)       # target dtype
    with pytest.raises(RuntimeError):
        ext.xent_dense_fwd(x, t[:-1], -100, 0.0, 0, 0)        # target shape
    with pytest.raises(RuntimeError):
        ext.xent_dense_fwd(x.t(), t[:21], -100, 0.0, 0, 0)    # strided rows
    with pytest.raises(RuntimeError):
        ext.xent_dense_fwd(x.double(), t, -100, 0.0, 0, 0)    # logits dtype
    with pytest.raises(RuntimeError):
        ext.xent_dense_fwd(x.cpu(), t.cpu(), -100, 0.0, 0, 0)
    # the earlier entry points keep their signatures
    x, t = _make((33, 64), FP32, ROWS2D, -100)
    t = t.clamp(0, 63)
    loss, lse = ext.softmax_xent_fwd(x, t)
    new_loss, new_lse, _ = ext.xent_dense_fwd(x, t, -100, 0.0, 0, 0)
    assert torch.equal(loss, new_loss) and torch.equal(lse, new_lse)
    g = torch.ones(33, device=_DEV)
    assert torch.equal(ext.softmax_xent_bwd(x, lse, t, g),
                       ext.xent_dense_bwd(x, lse, t, g, None, -100, 0.0, 0, 0))
