"""The dual BatchNorm join, y = relu(bn_a(xa) + bn_b(xb)), and its backward
(``bn_dual_fwd_train`` / ``bn_dual_bwd`` in csrc/bn_relu.hip) vs a plain fp64
reference, and the fused Bottleneck routed through them vs the same block on
the two-call composition.

Kernel level.  The reference is the textbook helper of test_gpu_bn.py
(``_bn_ref``) chained the way the join is defined: branch b without ReLU, its
unrounded output as the residual of branch a with ReLU, and for the backward
the gated gradient of a as the upstream gradient of b.  Run in fp64 and fp32
on exactly the values the kernels see, it gives the bound of that suite for
every compared quantity,

    bound(q) = 16 * max|ref32(q) - ref64(q)| + half_ulp(out dtype) * |ref64(q)|

Both inputs carry per-channel distinct mean, spread, weight, bias and running
statistics, drawn with different seeds, so swapped channel slots or swapped
branches cannot pass.  Pinned exactly: mask == (y > 0), the two dbeta outputs
equal.  The ReLU gate is the kernel's own in the backward reference; where it
disagrees with fp64 the fp64 pre-activation lies within the forward bound of
0, for at most 0.1 % of the elements.

Block level.  The fused Bottleneck (stride 2 and stride 1) runs on the dual
path with the two entries wrapped, so that the tensors the block hands them
and what they return are on record.  Two whole-block runs cannot be compared
element by element: the stage-A statistics kernels merge per-thread sums
through LDS atomics in arbitrary order, the last bit of a mean moves between
runs, and that moves bf16 roundings upstream of the join.  So the two-call
composition (``bn_fwd_train`` on td, then on t3 with the normalized shortcut
idn as residual; two ``bn_bwd``) is replayed on the recorded t3, td, dy:

  * forward: the pre-activations differ by the rounding of idn to bf16, at
    most half an ulp of idn, and y is rounded to bf16 on both sides:
    |y_dual - y_two| <= half_ulp(idn) + half_ulp(y_dual) + half_ulp(y_two),
    plus 2^-20 (|idn| + |y|) for the last-bit freedom of the fp32 statistics.
    Gate flips can only sit where that bound reaches 0: at most 0.1 %.
  * backward, replayed with the dual pass's own mask so that both sides gate
    alike: the per-channel sums are the same terms in another order,
    |diff| <= 2 M 2^-24 sum|terms| (M terms per channel, both sides); dx
    inherits that through db/M and xhat dg/M and is rounded to bf16 on both
    sides.
  * routing: the block's gradients for bn3 and the downsample BN are the dual
    outputs bit for bit, the running statistics of both BNs match the replay
    to a reordered sum (2^-14 of their scale) and did move.

The same block with ``TFOS_BN_DUAL=off`` must not touch the dual entries, and
its gradients agree with the dual run's in relative L2 to 10 %: gate flips
(at most 0.1 % of the elements, each changing its gradient fully) and the
upstream jitter give a few per cent at most, a tensor routed to the wrong
branch or parameter gives order 100 %.
"""

import copy

import pytest
import torch

from test_gpu_bn import (BF16, EPS, FP32, NHWC, _bits_equal, _bn_ref, _bound,
                         _check, _ext, _half_ulp, _make_inputs, _memory_order,
                         _vec, gpu, requires_gpu)


def _run_dual_case(dtype, shape, const_a=None, const_b=None, momentum=0.1):
    ext = _ext()
    N, C, H, W = shape
    a = _make_inputs(dtype, shape, NHWC, 11, const_a)
    b = _make_inputs(dtype, shape, NHWC, 23, const_b)
    xa, xb, dy = a["x"], b["x"], a["dy"]
    rma, rva = a["rm0"].clone(), a["rv0"].clone()
    rmb, rvb = b["rm0"].clone(), b["rv0"].clone()
    print("\ndual case {} {} const_a={} const_b={}".format(
        str(dtype).replace("torch.", ""), shape, const_a, const_b))
    assert ext.bn_dual_eligible(xa, xb)

    y, mean_a, rstd_a, mean_b, rstd_b, mask = ext.bn_dual_fwd_train(
        xa, xb, a["w"], a["b"], rma, rva, b["w"], b["b"], rmb, rvb,
        momentum, EPS)
    dxa, dxb, dga, dgb, dba, dbb = ext.bn_dual_bwd(
        xa, xb, dy, mask, a["w"], mean_a, rstd_a, b["w"], mean_b, rstd_b)
    torch.cuda.synchronize()
    assert y.dtype == dtype and y.stride() == xa.stride()

    gate = y > 0
    ref = {}
    for dt in (torch.float64, torch.float32):
        rb = _bn_ref(dt, xb, b["w"], b["b"], rm0=b["rm0"], rv0=b["rv0"],
                     momentum=momentum)
        ra = _bn_ref(dt, xa, a["w"], a["b"], res=rb["pre"], dy=dy, relu=True,
                     gate=gate, rm0=a["rm0"], rv0=a["rv0"], momentum=momentum)
        rb_bwd = _bn_ref(dt, xb, b["w"], b["b"], dy=ra["dres"])
        ref[dt] = (ra, rb, rb_bwd)
    (a64, b64, bb64), (a32, b32, bb32) = ref[torch.float64], ref[torch.float32]

    def keep(cc):
        return None if cc is None else torch.arange(C, device="cuda") != cc

    # forward and statistics of both branches
    _check("y", y, a64["y"], a32["y"], dtype)
    _check("mean_a", mean_a, a64["mean"], a32["mean"], FP32)
    _check("mean_b", mean_b, b64["mean"], b32["mean"], FP32)
    _check("rstd_a", rstd_a, a64["rstd"], a32["rstd"], FP32, keep(const_a))
    _check("rstd_b", rstd_b, b64["rstd"], b32["rstd"], FP32, keep(const_b))
    for what, got, r64, r32 in (
            ("running_mean_a", rma, a64, a32), ("running_var_a", rva, a64, a32),
            ("running_mean_b", rmb, b64, b32), ("running_var_b", rvb, b64, b32)):
        key = what[:-2]
        _check(what, got, r64[key], r32[key], FP32)
    # both pairs really moved off their initial values
    assert not torch.equal(rma, a["rm0"]) and not torch.equal(rva, a["rv0"])
    assert not torch.equal(rmb, b["rm0"]) and not torch.equal(rvb, b["rv0"])

    # gate: the mask is y > 0 exactly; against fp64 only within the bound of 0
    vec = _vec(dtype)
    assert mask.dtype == torch.uint8 and mask.numel() == xa.numel() // vec
    bits = (mask.to(torch.int32)[:, None]
            >> torch.arange(vec, device="cuda", dtype=torch.int32)) & 1
    assert torch.equal(bits.reshape(-1).bool(),
                       _memory_order(y, NHWC) > 0), "bitmask != (y > 0)"
    disagree = gate != (a64["pre"] > 0)
    frac = disagree.double().mean().item()
    print("  gate disagreements with fp64: {} ({:.4%})".format(
        int(disagree.sum()), frac))
    ytol = _bound(a64["y"], a32["y"], dtype)
    assert (a64["pre"].abs()[disagree] <= ytol[disagree]).all(), \
        "gate differs from fp64 away from 0"
    assert frac <= 1e-3

    # backward
    assert dxa.dtype == dtype and dxa.stride() == xa.stride()
    assert dxb.dtype == dtype and dxb.stride() == xb.stride()
    _check("dxa", dxa, a64["dx"], a32["dx"], dtype)
    _check("dxb", dxb, bb64["dx"], bb32["dx"], dtype)
    _check("dgamma_a", dga, a64["dgamma"], a32["dgamma"], FP32)
    _check("dgamma_b", dgb, bb64["dgamma"], bb32["dgamma"], FP32)
    _check("dbeta_a", dba, a64["dbeta"], a32["dbeta"], FP32)
    _check("dbeta_b", dbb, bb64["dbeta"], bb32["dbeta"], FP32)
    assert torch.equal(dba, dbb), "the two dbeta outputs differ"
    assert dba.data_ptr() != dbb.data_ptr()
    # inputs are left alone
    fresh = _make_inputs(dtype, shape, NHWC, 11, const_a)
    assert _bits_equal(xa, fresh["x"]) and _bits_equal(dy, fresh["dy"])
    assert _bits_equal(xb, _make_inputs(dtype, shape, NHWC, 23, const_b)["x"])


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [
    (8, 64, 14, 14),      # one vector per thread
    (2, 2048, 7, 7),      # largest C; fp32: one block row is half of C
    (33, 256, 9, 9),      # ragged, several vectors per thread in the reductions
    (16, 64, 66, 66),     # more vectors than 2048 blocks hold: apply/dx stride
], ids=lambda s: "x".join(map(str, s)))
def test_bn_dual_matrix(dtype, shape):
    _run_dual_case(dtype, shape)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_bn_dual_constant_channel(dtype, which):
    """One channel of one input is constant (var = 0): outputs stay finite and
    in bound; only that channel's rstd is left out of the comparison."""
    _run_dual_case(dtype, (8, 64, 14, 14),
                   const_a=1 if which == "a" else None,
                   const_b=2 if which == "b" else None, momentum=0.3)


@gpu
@requires_gpu
def test_bn_dual_ineligible_pairs_are_refused():
    ext = _ext()
    x = torch.randn(4, 64, 8, 8, device="cuda").to(BF16)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert ext.bn_dual_eligible(cl, cl.clone())
    assert not ext.bn_dual_eligible(x, x.clone())                   # NCHW
    assert not ext.bn_dual_eligible(cl, cl.float())                 # dtypes
    odd = torch.randn(4, 24, 8, 8, device="cuda").to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    assert not ext.bn_dual_eligible(odd, odd.clone())               # generic C
    v = torch.ones(24, device="cuda")
    with pytest.raises(RuntimeError):
        ext.bn_dual_fwd_train(odd, odd.clone(), v, v, v.clone(), v.clone(),
                              v, v, v.clone(), v.clone(), 0.1, EPS)


# ---------------------------------------------------------------------------
# block level: _BottleneckFn on the dual path vs the two-call composition
# ---------------------------------------------------------------------------

def _make_block(stride, seed):
    from tensorflowonspark_amd.models.resnet import Bottleneck, conv1x1
    from tensorflowonspark_amd.ops.modules import FusedBN
    torch.manual_seed(seed)
    down = torch.nn.Sequential(conv1x1(64, 256, stride), FusedBN(256))
    blk = Bottleneck(64, 64, stride, down).cuda().to(
        memory_format=torch.channels_last)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for m in blk.modules():          # distinct per-channel affine params
            if hasattr(m, "running_mean") and m.weight is not None:
                m.weight.copy_(torch.rand(m.weight.shape, device="cuda",
                                          generator=gen) * 1.5 + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, device="cuda",
                                        generator=gen) * 2 - 1)
    blk.train()
    assert blk._block_fusable
    return blk


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _run_block(blk, x, dy, monkeypatch, dual):
    monkeypatch.setenv("TFOS_BN_DUAL", "on" if dual else "off")
    ext = _ext()
    rec = {}
    orig_f, orig_b = ext.bn_dual_fwd_train, ext.bn_dual_bwd

    def fwd(*a):
        rec["fwd_in"] = [t.clone() if torch.is_tensor(t) else t for t in a]
        rec["fwd_out"] = orig_f(*a)
        return rec["fwd_out"]

    def bwd(*a):
        rec["bwd_in"] = a
        rec["bwd_out"] = orig_b(*a)
        return rec["bwd_out"]

    monkeypatch.setattr(ext, "bn_dual_fwd_train", fwd)
    monkeypatch.setattr(ext, "bn_dual_bwd", bwd)
    x = x.clone().requires_grad_(True)
    y = blk(x)
    y.backward(dy)
    torch.cuda.synchronize()
    monkeypatch.setattr(ext, "bn_dual_fwd_train", orig_f)
    monkeypatch.setattr(ext, "bn_dual_bwd", orig_b)
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    bufs = {n: b.clone() for n, b in blk.named_buffers()}
    return y.detach(), x.grad.clone(), grads, bufs, rec


@gpu
@requires_gpu
@pytest.mark.parametrize("stride", [2, 1])
def test_bottleneck_dual_vs_two_calls(stride, monkeypatch):
    ext = _ext()
    blk = _make_block(stride, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(4, 64, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    oh = 16 // stride
    dy = torch.randn(4, 256, oh, oh, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    y2, dx2, g2, b2, rec2 = _run_block(copy.deepcopy(blk), x, dy, monkeypatch,
                                       dual=False)
    y1, dx1, g1, b1, rec = _run_block(copy.deepcopy(blk), x, dy, monkeypatch,
                                      dual=True)
    assert not rec2, "TFOS_BN_DUAL=off still ran the dual entries"
    assert set(rec) == {"fwd_in", "fwd_out", "bwd_in", "bwd_out"}

    # ---- forward replay on the recorded t3, td
    (t3, td, w3, bb3, rm3, rv3, wd, bd, rmd, rvd, momentum, eps) = rec["fwd_in"]
    yd, m3, r3, md, rd, k3 = rec["fwd_out"]
    assert _bits_equal(yd, y1)
    idn, md2, rd2, _ = ext.bn_fwd_train(td, None, wd, bd, rmd, rvd, momentum,
                                        eps, False)
    yc, m32, r32, _k = ext.bn_fwd_train(t3, idn, w3, bb3, rm3, rv3, momentum,
                                        eps, True)
    tol = (_half_ulp(idn.double(), BF16) + _half_ulp(y1.double(), BF16)
           + _half_ulp(yc.double(), BF16)
           + 2.0 ** -20 * (idn.double().abs() + y1.double().abs()))
    err = (y1.double() - yc.double()).abs()
    flips = (y1 > 0) != (yc > 0)
    print("\nstride {}: y differs in {} of {} elements, max {:.3e}; worst "
          "err - bound {:.3e}; gate flips {}".format(
              stride, int((err > 0).sum()), err.numel(), err.max().item(),
              (err - tol).max().item(), int(flips.sum())))
    assert (err <= tol).all(), "y: {} elements beyond the idn rounding".format(
        int((err > tol).sum()))
    assert flips.double().mean().item() <= 1e-3

    # ---- routing of the statistics
    names = {"bn3.running_mean": rm3, "bn3.running_var": rv3,
             "downsample.1.running_mean": rmd, "downsample.1.running_var": rvd}
    before = dict(blk.named_buffers())
    for n, replayed in names.items():
        scale = replayed.abs().max().item()
        e = (b1[n] - replayed).abs().max().item()
        print("  {:<28s} max diff {:.3e}  scale {:.3e}".format(n, e, scale))
        assert e <= 2.0 ** -14 * scale, "buffer {} differs".format(n)
        assert not torch.equal(b1[n], before[n]), "{} not updated".format(n)

    # ---- backward replay, gated by the dual pass's own mask
    t3b, tdb, dyb, k3b, w3b, m3b, r3b, wdb, mdb, rdb = rec["bwd_in"]
    assert _bits_equal(dyb, dy) and torch.equal(k3b, k3)
    dt3, dtd, dg3, dgd, db3, dbd = rec["bwd_out"]
    dt3c, dg3c, db3c, dres = ext.bn_bwd(t3, dy, y1, k3, w3, m3, r3, True, True)
    dtdc, dgdc, dbdc = ext.bn_bwd(td, dres, y1,
                                  torch.empty(0, dtype=torch.uint8,
                                              device="cuda"),
                                  wd, md, rd, False, False)
    M = t3.numel() // t3.shape[1]
    u = 2.0 ** -24
    g = torch.where(y1 > 0, dy, torch.zeros_like(dy)).double()

    def bc(v):
        return v.double()[None, :, None, None]

    tol_db = 2 * M * u * g.abs().sum(dim=(0, 2, 3))
    for what, got, ref, t, m, r, w_, dxg, dxr in (
            ("a", dg3, dg3c, t3, m3, r3, w3, dt3, dt3c),
            ("b", dgd, dgdc, td, md, rd, wd, dtd, dtdc)):
        xhat = (t.double() - bc(m)) * bc(r)
        tol_dg = 2 * M * u * (g * xhat).abs().sum(dim=(0, 2, 3))
        e = (got.double() - ref.double()).abs()
        print("  dgamma_{} max diff {:.3e}  (bound min {:.3e})".format(
            what, e.max().item(), tol_dg.min().item()))
        assert (e <= tol_dg).all(), "dgamma_" + what
        tol_dx = (bc(w_ * r).abs() * (bc(tol_db) + xhat.abs() * bc(tol_dg)) / M
                  + _half_ulp(dxg.double(), BF16) + _half_ulp(dxr.double(), BF16)
                  + 2.0 ** -20 * dxr.double().abs())
        e = (dxg.double() - dxr.double()).abs()
        print("  dx_{} max diff {:.3e}, worst err - bound {:.3e}".format(
            what, e.max().item(), (e - tol_dx).max().item()))
        assert (e <= tol_dx).all(), "dx_" + what
    for got, ref in ((db3, db3c), (dbd, dbdc)):
        assert ((got.double() - ref.double()).abs() <= tol_db).all(), "dbeta"
    assert torch.equal(db3, dbd)

    # ---- routing of the gradients: the block returns the dual outputs
    assert torch.equal(g1["bn3.weight"], dg3)
    assert torch.equal(g1["bn3.bias"], db3)
    assert torch.equal(g1["downsample.1.weight"], dgd)
    assert torch.equal(g1["downsample.1.bias"], dbd)

    # ---- whole block against the two-call block
    assert set(g1) == set(g2)
    for what, a, b in [("dx", dx1, dx2), ("y", y1, y2)] + \
            [("grad " + n, g1[n], g2[n]) for n in sorted(g2)]:
        assert torch.isfinite(a).all()
        rel = _rel_l2(a, b)
        print("  {:<28s} rel L2 {:.3e}".format(what, rel))
        assert rel <= 0.1, "{}: rel L2 {:.3e}".format(what, rel)
