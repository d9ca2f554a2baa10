"""Fused BatchNorm kernels (csrc/bn_relu.hip) vs a plain fp64 reference.

Every dispatch tier of the BN family is driven directly through the extension
(``bn_fwd_train`` / ``bn_fwd_eval`` / ``bn_bwd``) and compared with textbook
batch-norm arithmetic done in fp64 on the same device, on inputs where every
channel has its own mean, spread, weight, bias and running statistics, so that
a kernel which mixes up channel slots cannot pass.

Tolerances come from the reference alone, never from the kernel's observed
error.  For each compared quantity q:

    bound(q) = 16 * max|ref32(q) - ref64(q)|  +  half_ulp(out dtype) * |ref64(q)|

    ref64 / ref32   the same helper (_bn_ref) run in fp64 / fp32 on exactly the
                    values the kernel sees (inputs rounded to the test dtype)
    half_ulp        half an ulp of the output dtype at |ref64|: 2^-24 * |ref64|
                    for fp32 tensors and the fp32 per-channel statistics; for
                    bf16 the exact 2^(e-8) with 2^e <= |ref64| < 2^(e+1), which
                    lies between 2^-9 and 2^-8 times |ref64| (a flat
                    2^-9 * |ref64| is less than the error of rounding the fp64
                    reference itself to bf16 over most of each binade)
    16x           torch reduces pairwise; the kernels chain up to
                    nvec/(grid*256) sequential fp32 adds per thread and then
                    merge through LDS atomics in arbitrary order

ReLU gating: the gradient jumps where the pre-activation crosses 0, so the
backward reference gates with the kernel's own ``y > 0``.  The gate itself is
pinned separately and exactly (bitmask == y > 0, gout bit-identical to
where(y > 0, dy, 0)), and wherever it disagrees with the fp64 gate the fp64
pre-activation must lie within the forward bound of 0, for at most 0.1% of
the elements.
"""

import pytest
import torch

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

EPS = 1e-5
BF16 = torch.bfloat16
FP32 = torch.float32
NHWC = "nhwc"
NCHW = "nchw"
FAST = "fast"
GENERIC = "generic"
_DEV = "cuda"      # where inputs and references live


def _ext():
    from tensorflowonspark_amd.ops import get_ext
    e = get_ext(required=True)
    assert e is not None
    return e


def _vec(dtype):
    return 8 if dtype == BF16 else 4


def _half_ulp(ref64, dtype):
    """Half an ulp of ``dtype`` at |ref64|."""
    if dtype == BF16:
        # |ref| = m * 2^e with m in [0.5, 1): a bf16 ulp there is 2^(e-8)
        _, e = torch.frexp(ref64)
        half = torch.ldexp(torch.ones_like(ref64), e - 9)
        return torch.where(ref64 == 0, torch.zeros_like(ref64), half)
    return 2.0 ** -24 * ref64.abs()


def _bc(v):
    return v[None, :, None, None]


def _layout(t, layout):
    if layout == NHWC:
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def _memory_order(t, layout):
    """Elements of a 4-D tensor in the order they sit in memory."""
    if layout == NHWC:
        t = t.permute(0, 2, 3, 1)
    return t.reshape(-1)


# ---------------------------------------------------------------------------
# inputs: every channel has its own distribution
# ---------------------------------------------------------------------------

def _per_channel(C, lo, hi, gen):
    """C distinct values spread evenly over [lo, hi], in shuffled order."""
    frac = torch.randperm(C, generator=gen).double() / max(C - 1, 1)
    return (lo + (hi - lo) * frac).float().to(_DEV)


def _make_inputs(dtype, shape, layout, seed, const_channel=None):
    N, C, H, W = shape
    cpu_gen = torch.Generator().manual_seed(seed)
    gen = torch.Generator(device=_DEV).manual_seed(seed)

    def randn():
        return torch.randn(N, C, H, W, device=_DEV, generator=gen)

    mu = _per_channel(C, -4.0, 4.0, cpu_gen)        # |mean|/std <= 8
    sigma = _per_channel(C, 0.5, 2.0, cpu_gen)
    x = randn().mul_(_bc(sigma)).add_(_bc(mu))
    if const_channel is not None:
        x[:, const_channel] = 1.75                  # var == 0 there
    w = _per_channel(C, 0.5, 2.0, cpu_gen)
    w[torch.arange(C, device=_DEV) % 5 == 3] *= -1.0   # a few negative
    d = {
        "x": _layout(x.to(dtype), layout),
        "res": _layout(randn().mul_(_bc(_per_channel(C, 0.5, 2.0, cpu_gen)))
                       .to(dtype), layout),
        "dy": _layout(randn().mul_(_bc(_per_channel(C, 0.5, 2.0, cpu_gen)))
                      .to(dtype), layout),
        "w": w,
        "b": _per_channel(C, -1.0, 1.0, cpu_gen),
        "rm0": _per_channel(C, -2.0, 2.0, cpu_gen),
        "rv0": _per_channel(C, 0.5, 3.0, cpu_gen),
    }
    return d


# ---------------------------------------------------------------------------
# reference: textbook batch norm in plain tensor arithmetic
# ---------------------------------------------------------------------------

def _bn_ref(dt, x, w, b, res=None, dy=None, relu=False, gate=None,
            rm0=None, rv0=None, momentum=0.1, eps=EPS):
    """Training-mode BN (+res)(+relu) forward and backward in dtype ``dt``.

    ``gate`` is the boolean ReLU gate for the backward; None means the
    reference's own ``pre > 0``.
    """
    X = x.to(dt)
    N, C, H, W = X.shape
    M = N * H * W
    dims = (0, 2, 3)
    mean = X.mean(dim=dims)
    xc = X - _bc(mean)
    var = (xc * xc).mean(dim=dims)
    var_unbiased = var * M / (M - 1) if M > 1 else var
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = xc * _bc(rstd)
    W_, B_ = w.to(dt), b.to(dt)
    pre = xhat * _bc(W_) + _bc(B_)
    if res is not None:
        pre = pre + res.to(dt)
    out = {"mean": mean, "var": var, "var_unbiased": var_unbiased,
           "rstd": rstd, "pre": pre,
           "y": pre.clamp_min(0) if relu else pre}
    if rm0 is not None:
        out["running_mean"] = (1 - momentum) * rm0.to(dt) + momentum * mean
        out["running_var"] = ((1 - momentum) * rv0.to(dt)
                              + momentum * var_unbiased)
    if dy is not None:
        g = dy.to(dt)
        if relu:
            g = g * (pre > 0 if gate is None else gate).to(dt)
        dbeta = g.sum(dim=dims)
        dgamma = (g * xhat).sum(dim=dims)
        out["dbeta"], out["dgamma"], out["dres"] = dbeta, dgamma, g
        out["dx"] = _bc(W_ * rstd) * (g - _bc(dbeta) / M
                                      - xhat * _bc(dgamma) / M)
    return out


def _eval_ref(dt, x, w, b, rm, rv, res=None, relu=False, eps=EPS):
    rstd = 1.0 / torch.sqrt(rv.to(dt) + eps)
    y = (x.to(dt) - _bc(rm.to(dt))) * _bc(rstd * w.to(dt)) + _bc(b.to(dt))
    if res is not None:
        y = y + res.to(dt)
    return y.clamp_min(0) if relu else y


def _bound(ref64, ref32, out_dtype):
    ref_err = (ref32.double() - ref64).abs().max()
    return 16.0 * ref_err + _half_ulp(ref64, out_dtype)


def _check(what, got, ref64, ref32, out_dtype, keep=None):
    """|got - ref64| <= bound elementwise; prints the figures first."""
    assert got.shape == ref64.shape, "{}: shape {} vs {}".format(
        what, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), "{}: non-finite values".format(what)
    if keep is not None:
        got, ref64, ref32 = got[keep], ref64[keep], ref32[keep]
    tol = _bound(ref64, ref32, out_dtype)
    err = (got.double() - ref64).abs()
    ref_err = (ref32.double() - ref64).abs().max().item()
    worst = (err - tol).argmax()
    print("  {:<13s} err max {:.3e}  ref32-vs-fp64 max {:.3e}  "
          "worst err/bound {:.3e}/{:.3e}".format(
              what, err.max().item(), ref_err,
              err.reshape(-1)[worst].item(), tol.reshape(-1)[worst].item()))
    bad = err > tol
    assert not bad.any(), (
        "{}: {} of {} outside the bound; worst err {:.4e} vs bound {:.4e} "
        "(ref32-vs-fp64 max {:.3e})".format(
            what, int(bad.sum()), bad.numel(),
            err.reshape(-1)[worst].item(), tol.reshape(-1)[worst].item(),
            ref_err))


def _bits_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int16 if a.dtype == BF16 else torch.int32
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---------------------------------------------------------------------------
# one kernel-matrix case: forward, saved stats, running stats, gate, backward
# ---------------------------------------------------------------------------

def _run_train_case(dtype, shape, layout, relu, add, path, momentum=0.1,
                    const_channel=None, seed=0):
    ext = _ext()
    N, C, H, W = shape
    M = N * H * W
    d = _make_inputs(dtype, shape, layout, seed, const_channel)
    x, w, b = d["x"], d["w"], d["b"]
    res = d["res"] if add else None
    dy = d["dy"]
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    print("\ncase {} {} {} relu={} add={} {} momentum={}".format(
        str(dtype).replace("torch.", ""), shape, layout, relu, add, path,
        momentum))

    y, mean, rstd, mask = ext.bn_fwd_train(x, res, w, b, rm, rv, momentum,
                                           EPS, relu)
    out = ext.bn_bwd(x, dy, y, mask, w, mean, rstd, relu, add)
    torch.cuda.synchronize()

    assert y.dtype == dtype and y.stride() == x.stride()
    assert mean.dtype == FP32 and rstd.dtype == FP32
    # inputs are left alone
    fresh = _make_inputs(dtype, shape, layout, seed, const_channel)
    assert _bits_equal(x, fresh["x"]) and _bits_equal(dy, fresh["dy"])
    assert torch.equal(w, fresh["w"]) and torch.equal(b, fresh["b"])
    del fresh

    gate = (y > 0) if relu else None
    kw = dict(x=x, w=w, b=b, res=res, dy=dy, relu=relu, gate=gate,
              rm0=d["rm0"], rv0=d["rv0"], momentum=momentum)
    r64 = _bn_ref(torch.float64, **kw)
    r32 = _bn_ref(torch.float32, **kw)

    # forward
    _check("y", y, r64["y"], r32["y"], dtype)
    _check("save_mean", mean, r64["mean"], r32["mean"], FP32)
    keep = None
    if const_channel is not None:
        keep = torch.arange(C, device="cuda") != const_channel
    _check("save_rstd", rstd, r64["rstd"], r32["rstd"], FP32, keep)
    _check("running_mean", rm, r64["running_mean"], r32["running_mean"], FP32)
    _check("running_var", rv, r64["running_var"], r32["running_var"], FP32)
    if M > 1:
        # the reference's running_var really is the unbiased one
        expect = ((1 - momentum) * d["rv0"].double()
                  + momentum * (r64["var"] * M / (M - 1)))
        assert torch.equal(r64["running_var"], expect)

    if const_channel is not None:
        cc = const_channel
        expect = torch.full((N, H, W), float(b[cc]), device="cuda",
                            dtype=torch.float64)
        if add:
            expect = expect + res[:, cc].double()
        if relu:
            expect = expect.clamp_min(0)
        tol = _bound(r64["y"], r32["y"], dtype)[:, cc]
        got = y[:, cc].double()
        assert torch.isfinite(got).all()
        assert ((got - expect).abs() <= tol).all(), "constant channel y"

    # gate: exact where it can be, bounded where it cannot
    vec = _vec(dtype)
    if relu and path == FAST:
        assert mask.dtype == torch.uint8 and mask.numel() == x.numel() // vec
        bits = (mask.to(torch.int32)[:, None]
                >> torch.arange(vec, device="cuda", dtype=torch.int32)) & 1
        assert torch.equal(bits.reshape(-1).bool(),
                           _memory_order(y, layout) > 0), "bitmask != (y > 0)"
    else:
        assert mask.numel() == 0, "unexpected dispatch: mask of {}".format(
            mask.numel())
    if relu:
        disagree = gate != (r64["pre"] > 0)
        frac = disagree.double().mean().item()
        print("  gate disagreements with fp64: {} ({:.4%})".format(
            int(disagree.sum()), frac))
        ytol = _bound(r64["y"], r32["y"], dtype)
        assert (r64["pre"].abs()[disagree] <= ytol[disagree]).all(), \
            "gate differs from fp64 away from 0"
        assert frac <= 1e-3

    # backward
    assert len(out) == (4 if add else 3)
    dx, dgamma, dbeta = out[0], out[1], out[2]
    assert dx.dtype == dtype and dx.stride() == x.stride()
    _check("dx", dx, r64["dx"], r32["dx"], dtype)
    _check("dgamma", dgamma, r64["dgamma"], r32["dgamma"], FP32)
    _check("dbeta", dbeta, r64["dbeta"], r32["dbeta"], FP32)
    if add:
        gout = out[3]
        assert gout.dtype == dtype and gout.stride() == x.stride()
        expect = torch.where(gate, dy, torch.zeros_like(dy)) if relu else dy
        assert _bits_equal(gout, expect), "gout not bit-identical"
        _check("dres", gout, r64["dres"], r32["dres"], dtype)


FF, TF, TT, FT = (False, False), (True, False), (True, True), (False, True)


def _cases():
    """(dtype, shape, layout, (relu, add), path, momentum) per dispatch tier."""
    out = []

    def add(dtype, shape, layout, variants, path, momentum=0.1):
        for v in variants:
            out.append(pytest.param(
                dtype, shape, layout, v[0], v[1], path, momentum,
                id="{}-{}-{}-{}{}-{}".format(
                    "bf16" if dtype == BF16 else "fp32",
                    "x".join(map(str, shape)), layout,
                    "relu" if v[0] else "lin", "+res" if v[1] else "", path)))

    # single pass, minimum C
    add(BF16, (2, 8, 5, 5), NHWC, (FF, TF, TT, FT), FAST)
    add(FP32, (2, 4, 5, 5), NHWC, (FF, TF, TT, FT), FAST)
    # ragged multi-iteration stats loop on the minimum 64-block grid
    add(BF16, (8, 64, 28, 28), NHWC, (TF, TT), FAST)
    add(FP32, (8, 64, 14, 14), NHWC, (FF, TT), FAST)
    # 64 < reduction grid < 1024; apply/dx capped at TFOSR_MAX_GRID and stride
    add(BF16, (32, 256, 28, 28), NHWC, (TT,), FAST, momentum=0.3)
    # largest C
    add(BF16, (3, 2048, 7, 7), NHWC, (TF, TT), FAST)
    add(BF16, (2, 2048, 2, 2), NHWC, (TF, TT), FAST)
    # fp32 C=2048: one block row (256*4) covers only half of the channels
    add(FP32, (2, 2048, 2, 2), NHWC, (FF, TT), FAST)
    add(FP32, (3, 2048, 7, 7), NHWC, (FF, TT), FAST)
    # fp32 C=1024: one block row is exactly C
    add(FP32, (2, 1024, 3, 3), NHWC, (TF,), FAST)
    # generic NHWC: C does not divide a block row, or C % V != 0
    for C in (24, 96, 12):
        add(BF16, (4, C, 7, 7), NHWC, (FF, TF, TT), GENERIC)
    for C in (6, 24):
        add(FP32, (4, C, 7, 7), NHWC, (FF, TF, TT), GENERIC)
    # generic NHWC with more vectors than TFOSR_MAX_GRID * 256: were this C let
    # onto the fast path, its channel slots would go wrong from the second
    # grid-stride iteration on (the grid stride is no multiple of 24) while
    # smaller tensors would still come out right
    add(FP32, (32, 24, 56, 56), NHWC, (FF, TT), GENERIC)
    # generic NCHW
    add(BF16, (4, 32, 7, 7), NCHW, (TF, TT), GENERIC)
    add(FP32, (4, 32, 7, 7), NCHW, (TF, TT), GENERIC)
    # M = 8 and M = 2: the unbiased factor M/(M-1) is 1.14 and 2
    add(FP32, (2, 16, 2, 2), NHWC, (FF,), FAST)
    add(FP32, (2, 16, 2, 2), NCHW, (FF,), GENERIC)
    add(FP32, (1, 16, 2, 1), NHWC, (FF,), FAST)
    add(FP32, (1, 16, 2, 1), NCHW, (FF,), GENERIC)
    return out


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,shape,layout,relu,add,path,momentum", _cases())
def test_bn_train_matrix(dtype, shape, layout, relu, add, path, momentum):
    _run_train_case(dtype, shape, layout, relu, add, path, momentum)


@gpu
@requires_gpu
def test_bn_train_reduction_grid_clamped():
    """69 M elements: the reduction grid clamps at 1024 blocks and every
    thread chains 33 loads, the last one ragged."""
    _run_train_case(BF16, (66, 64, 128, 128), NHWC, True, True, FAST)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype,shape,layout,relu,add,path", [
    pytest.param(BF16, (2, 8, 5, 5), NHWC, True, True, FAST, id="bf16-fast"),
    pytest.param(FP32, (2, 4, 5, 5), NHWC, True, True, FAST, id="fp32-fast"),
    pytest.param(FP32, (4, 6, 7, 7), NHWC, True, False, GENERIC,
                 id="fp32-generic"),
    pytest.param(BF16, (4, 32, 7, 7), NCHW, False, True, GENERIC,
                 id="bf16-nchw"),
])
def test_bn_train_constant_channel(dtype, shape, layout, relu, add, path):
    """One channel is constant (var = 0): y there is bias (+res)(+relu), dx is
    finite, and only that channel's rstd is left out of the comparison."""
    _run_train_case(dtype, shape, layout, relu, add, path, const_channel=1,
                    seed=3)


# ---------------------------------------------------------------------------
# eval
# ---------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("relu,add", [FF, TF, TT, FT],
                         ids=["lin", "relu", "relu+res", "lin+res"])
@pytest.mark.parametrize("shape,layout", [
    ((4, 64, 7, 7), NHWC), ((4, 24, 7, 7), NHWC), ((2, 2048, 2, 2), NHWC),
    ((3, 2048, 7, 7), NHWC), ((4, 64, 7, 7), NCHW)],
    ids=["c64", "c24", "c2048-small", "c2048", "c64-nchw"])
def test_bn_eval(dtype, relu, add, shape, layout):
    ext = _ext()
    d = _make_inputs(dtype, shape, layout, seed=11)
    res = d["res"] if add else None
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    y = ext.bn_fwd_eval(d["x"], res, d["w"], d["b"], rm, rv, EPS, relu)
    torch.cuda.synchronize()
    assert y.dtype == dtype and y.stride() == d["x"].stride()
    assert torch.equal(rm, d["rm0"]) and torch.equal(rv, d["rv0"])
    r64 = _eval_ref(torch.float64, d["x"], d["w"], d["b"], rm, rv, res, relu)
    r32 = _eval_ref(torch.float32, d["x"], d["w"], d["b"], rm, rv, res, relu)
    print()
    _check("eval y", y, r64, r32, dtype)


# ---------------------------------------------------------------------------
# modules, through autograd
# ---------------------------------------------------------------------------

def _load(mod, d):
    with torch.no_grad():
        mod.weight.copy_(d["w"])
        mod.bias.copy_(d["b"])
        mod.running_mean.copy_(d["rm0"])
        mod.running_var.copy_(d["rv0"])


def _run_module_case(cls, dtype, shape, layout, momentum=0.1):
    C = shape[1]
    d = _make_inputs(dtype, shape, layout, seed=5)
    mod = cls(C, eps=EPS, momentum=momentum).cuda()
    _load(mod, d)
    x = d["x"].clone().requires_grad_(True)
    res = d["res"].clone().requires_grad_(True) if cls.ADD else None
    assert int(mod.num_batches_tracked) == 0
    y = mod(x, res) if cls.ADD else mod(x)
    y.backward(d["dy"])
    torch.cuda.synchronize()
    assert int(mod.num_batches_tracked) == 1

    yk = y.detach()
    kw = dict(x=d["x"], w=d["w"], b=d["b"], res=d["res"] if cls.ADD else None,
              dy=d["dy"], relu=cls.RELU, gate=(yk > 0) if cls.RELU else None,
              rm0=d["rm0"], rv0=d["rv0"], momentum=momentum)
    r64 = _bn_ref(torch.float64, **kw)
    r32 = _bn_ref(torch.float32, **kw)
    print()
    _check("y", yk, r64["y"], r32["y"], dtype)
    _check("x.grad", x.grad, r64["dx"], r32["dx"], dtype)
    _check("weight.grad", mod.weight.grad, r64["dgamma"], r32["dgamma"], FP32)
    _check("bias.grad", mod.bias.grad, r64["dbeta"], r32["dbeta"], FP32)
    _check("running_mean", mod.running_mean, r64["running_mean"],
           r32["running_mean"], FP32)
    _check("running_var", mod.running_var, r64["running_var"],
           r32["running_var"], FP32)
    if cls.ADD:
        _check("res.grad", res.grad, r64["dres"], r32["dres"], dtype)
        expect = torch.where(yk > 0, d["dy"], torch.zeros_like(d["dy"]))
        assert _bits_equal(res.grad, expect)

    # eval uses the buffers the training step just updated
    mod.eval()
    with torch.no_grad():
        ye = mod(d["x"], d["res"]) if cls.ADD else mod(d["x"])
    assert int(mod.num_batches_tracked) == 1
    ekw = dict(x=d["x"], w=d["w"], b=d["b"], res=d["res"] if cls.ADD else None,
               relu=cls.RELU)
    e64 = _eval_ref(torch.float64, rm=r64["running_mean"],
                    rv=r64["running_var"], **ekw)
    e32 = _eval_ref(torch.float32, rm=r32["running_mean"],
                    rv=r32["running_var"], **ekw)
    _check("eval y", ye, e64, e32, dtype)
    # ... and not the initial ones
    stale = _eval_ref(torch.float64, rm=d["rm0"], rv=d["rv0"], **ekw)
    assert ((ye.double() - stale).abs() > _bound(e64, e32, dtype)).any()


@gpu
@requires_gpu
def test_module_bn_add_relu_bf16_channels_last():
    from tensorflowonspark_amd.ops.modules import FusedBNAddReLU
    _run_module_case(FusedBNAddReLU, BF16, (8, 256, 14, 14), NHWC)


@gpu
@requires_gpu
def test_module_bn_relu_bf16_generic():
    from tensorflowonspark_amd.ops.modules import FusedBNReLU
    _run_module_case(FusedBNReLU, BF16, (4, 24, 7, 7), NHWC, momentum=0.3)


@gpu
@requires_gpu
def test_module_bn_plain_fp32_nchw():
    from tensorflowonspark_amd.ops.modules import FusedBN
    _run_module_case(FusedBN, FP32, (4, 32, 7, 7), NCHW)


# ---------------------------------------------------------------------------
# argument checks in the bindings
# ---------------------------------------------------------------------------

def _valid_args(dtype=BF16, shape=(2, 16, 3, 3), layout=NHWC):
    d = _make_inputs(dtype, shape, layout, seed=2)
    d["rm"], d["rv"] = d["rm0"].clone(), d["rv0"].clone()
    return d


def _other_layout(t):
    if t.is_contiguous(memory_format=torch.channels_last):
        return t.contiguous()
    return t.contiguous(memory_format=torch.channels_last)


_BAD_RES = {
    "size": lambda r: r[:1].clone(),
    "dtype": lambda r: r.float(),
    "layout": _other_layout,
    "device": lambda r: r.cpu(),
}

_BAD_PARAM = {
    "dtype": lambda p: p.double(),
    "half": lambda p: p.to(BF16),
    "strided": lambda p: torch.cat([p, p])[::2],
    "short": lambda p: p[:-1].clone(),
    "long": lambda p: torch.cat([p, p]),
    "device": lambda p: p.cpu(),
}


@gpu
@requires_gpu
@pytest.mark.parametrize("how", sorted(_BAD_RES))
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_bindings_reject_bad_residual(how, layout):
    ext = _ext()
    d = _valid_args(layout=layout)
    bad = _BAD_RES[how](d["res"])
    with pytest.raises(RuntimeError):
        ext.bn_fwd_train(d["x"], bad, d["w"], d["b"], d["rm"], d["rv"], 0.1,
                         EPS, True)
    with pytest.raises(RuntimeError):
        ext.bn_fwd_eval(d["x"], bad, d["w"], d["b"], d["rm"], d["rv"], EPS,
                        True)
    torch.cuda.synchronize()
    assert torch.equal(d["rm"], d["rm0"]) and torch.equal(d["rv"], d["rv0"])


@gpu
@requires_gpu
@pytest.mark.parametrize("how", sorted(_BAD_PARAM))
@pytest.mark.parametrize("which", ["w", "b", "rm", "rv"])
def test_bindings_reject_bad_forward_params(which, how):
    ext = _ext()
    d = _valid_args()
    d[which] = _BAD_PARAM[how](d[which])
    with pytest.raises(RuntimeError):
        ext.bn_fwd_train(d["x"], None, d["w"], d["b"], d["rm"], d["rv"], 0.1,
                         EPS, True)
    with pytest.raises(RuntimeError):
        ext.bn_fwd_eval(d["x"], d["res"], d["w"], d["b"], d["rm"], d["rv"],
                        EPS, False)


@gpu
@requires_gpu
@pytest.mark.parametrize("how", sorted(_BAD_PARAM))
@pytest.mark.parametrize("which", ["w", "save_mean", "save_rstd"])
def test_bindings_reject_bad_backward_params(which, how):
    ext = _ext()
    d = _valid_args()
    y, mean, rstd, mask = ext.bn_fwd_train(
        d["x"], None, d["w"], d["b"], d["rm"], d["rv"], 0.1, EPS, True)
    a = {"w": d["w"], "save_mean": mean, "save_rstd": rstd}
    a[which] = _BAD_PARAM[how](a[which])
    with pytest.raises(RuntimeError):
        ext.bn_bwd(d["x"], d["dy"], y, mask, a["w"], a["save_mean"],
                   a["save_rstd"], True, False)


@gpu
@requires_gpu
@pytest.mark.parametrize("which,how", [
    ("dy", "dtype"), ("dy", "size"), ("dy", "device"),
    ("y", "dtype"), ("y", "size"), ("y", "layout"), ("y", "device"),
    ("x", "device"), ("mask", "short"), ("mask", "device")])
def test_bindings_reject_bad_backward_tensors(which, how):
    ext = _ext()
    d = _valid_args()
    y, mean, rstd, mask = ext.bn_fwd_train(
        d["x"], None, d["w"], d["b"], d["rm"], d["rv"], 0.1, EPS, True)
    a = {"x": d["x"], "dy": d["dy"], "y": y, "mask": mask}
    if which == "mask":
        a["mask"] = mask[:-1].clone() if how == "short" else mask.cpu()
    else:
        a[which] = _BAD_RES[how](a[which])
    with pytest.raises(RuntimeError):
        ext.bn_bwd(a["x"], a["dy"], a["y"], a["mask"], d["w"], mean, rstd,
                   True, False)


@gpu
@requires_gpu
def test_bindings_reject_cpu_input():
    ext = _ext()
    d = _valid_args()
    with pytest.raises(RuntimeError):
        ext.bn_fwd_train(d["x"].cpu(), None, d["w"], d["b"], d["rm"], d["rv"],
                         0.1, EPS, True)
    with pytest.raises(RuntimeError):
        ext.bn_fwd_eval(d["x"].cpu(), None, d["w"], d["b"], d["rm"], d["rv"],
                        EPS, True)


@gpu
@requires_gpu
def test_bindings_accept_valid_calls():
    """The checks leave every valid combination alone."""
    ext = _ext()
    for dtype in (BF16, FP32):
        for layout in (NHWC, NCHW):
            d = _valid_args(dtype, (2, 16, 3, 3), layout)
            y, mean, rstd, mask = ext.bn_fwd_train(
                d["x"], d["res"], d["w"], d["b"], d["rm"], d["rv"], 0.1, EPS,
                True)
            ext.bn_bwd(d["x"], d["dy"], y, mask, d["w"], mean, rstd, True,
                       True)
            # dy in the other layout is converted, as before
            ext.bn_bwd(d["x"], _other_layout(d["dy"]), y, mask, d["w"], mean,
                       rstd, True, False)
            ext.bn_fwd_eval(d["x"], d["res"], d["w"], d["b"], d["rm"],
                            d["rv"], EPS, True)
    torch.cuda.synchronize()
