"""``TFOS_BN_GATE``: the backward of a fused Bottleneck without a downsample
branch, with the residual gradient gated in the conv1 dgrad epilogue
(``gemm_bt_gate``) instead of written out by ``bn_bwd`` and accumulated into
by ``gemm_bt_acc``.

Block: the identity Bottleneck of tests/test_gpu_calltrace.py's
``block_s1_plain`` (256 -> 64 -> 256 at 4 x 256 x 16 x 16, a 0.5 MB join).

* ``force`` reaches ``gemm_bt_gate`` and no ``gemm_bt_acc``, and calls bn3's
  ``bn_bwd`` with (relu, grad_res) = (True, False); ``off`` and an unset
  variable make the calls of the route before it (``auto`` does not route a
  0.5 MB join).
* The gradients under ``force`` are held to the ``off`` route with the bound
  tests/test_gpu_bn_epilogue.py and tests/test_gpu_bn_dual.py use at block
  level (relative L2 <= 0.1 per tensor) and, where the arithmetic allows it,
  to equality: the recorded ``gemm_bt_gate`` call is replayed as the old
  composition on its own inputs and must match bit for bit, and dx is held
  to the fp64 value of gate(dy) + dt1 @ w1^T on those inputs within the two
  bf16 roundings the kernel makes plus the fp32 accumulation of K products.
  The only thing that may differ between two runs of either route is the
  order of the float atomics in the BN reductions, forward and backward.
* The ``auto`` rule itself, on the CPU.
"""

import copy

import pytest
import torch

from test_gpu_bn import BF16, _bits_equal, _ext, _half_ulp, gpu, requires_gpu
from test_gpu_bn_dual import _rel_l2
from test_gpu_gemm_gate import _gated
from test_gpu_mfma import _assert_bound

ENTRIES = ("bn_bwd", "gemm_bt_acc", "gemm_bt_gate", "gemm_bt_gate_eligible")


def _identity_block(seed):
    from tensorflowonspark_amd.models.resnet import Bottleneck
    torch.manual_seed(seed)
    blk = Bottleneck(256, 64, 1, None).cuda().to(
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


def _run(blk, x, dy, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("TFOS_BN_GATE", raising=False)
    else:
        monkeypatch.setenv("TFOS_BN_GATE", mode)
    ext = _ext()
    rec = []
    orig = {n: getattr(ext, n) for n in ENTRIES}

    def wrap(name):
        def f(*a):
            out = orig[name](*a)
            rec.append((name, a, out))
            return out
        return f

    for n in ENTRIES:
        monkeypatch.setattr(ext, n, wrap(n))
    try:
        x = x.clone().requires_grad_(True)
        y = blk(x)
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        for n in ENTRIES:
            monkeypatch.setattr(ext, n, orig[n])
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    return y.detach(), x.grad.clone(), grads, rec


def _calls(rec):
    """Entry names in order; for bn_bwd with its (relu, grad_res) flags."""
    return [(n,) + tuple(a[-2:]) if n == "bn_bwd" else (n,)
            for n, a, _ in rec]


@pytest.fixture(scope="module")
def case():
    blk = _identity_block(seed=5)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(4, 256, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    dy = torch.randn(4, 256, 16, 16, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    return blk, x, dy


# bn3, bn2, bn1, then the conv1 dgrad that forms dx
OLD_CALLS = [("bn_bwd", True, True), ("bn_bwd", True, False),
             ("bn_bwd", True, False), ("gemm_bt_acc",)]
# a block left on the old route makes no call it did not make before (the
# call-trace golden records every entry), not even the eligibility query
NEW_CALLS = [("gemm_bt_gate_eligible",), ("bn_bwd", True, False),
             ("bn_bwd", True, False), ("bn_bwd", True, False),
             ("gemm_bt_gate",)]


@gpu
@requires_gpu
def test_identity_block_routes(case, monkeypatch):
    blk, x, dy = case
    for mode, want in (("off", OLD_CALLS), (None, OLD_CALLS),
                       ("auto", OLD_CALLS), ("force", NEW_CALLS)):
        _, _, _, rec = _run(copy.deepcopy(blk), x, dy, monkeypatch, mode)
        assert _calls(rec) == want, "TFOS_BN_GATE={}".format(mode)
    monkeypatch.setenv("TFOS_BN_GATE", "on")
    with pytest.raises(ValueError):
        xg = x.clone().requires_grad_(True)
        copy.deepcopy(blk)(xg).backward(dy)


@gpu
@requires_gpu
def test_identity_block_force_vs_off(case, monkeypatch):
    ext = _ext()
    blk, x, dy = case
    y0, dx0, g0, _ = _run(copy.deepcopy(blk), x, dy, monkeypatch, "off")
    y1, dx1, g1, rec = _run(copy.deepcopy(blk), x, dy, monkeypatch, "force")
    assert set(g1) == set(g0)
    # y too: the forward is the same code on both routes, but its BN
    # statistics are float atomics as well and need not repeat bit for bit
    for what, u, v in [("y", y1, y0), ("dx", dx1, dx0)] + \
            [("grad " + n, g1[n], g0[n]) for n in sorted(g0)]:
        assert torch.isfinite(u).all()
        rel = _rel_l2(u, v)
        print("  {:<28s} rel L2 {:.3e}".format(what, rel))
        assert rel <= 0.1, "{}: rel L2 {:.3e}".format(what, rel)

    # ---- the recorded gate call, replayed as the old composition
    (name, (dt1, w1bT, dy2d, k3), dx2d) = rec[-1]
    assert name == "gemm_bt_gate"
    bn3 = next(r for r in rec if r[0] == "bn_bwd")
    t3, dyb, yb, k3b, w3, m3, r3, relu, grad_res = bn3[1]
    assert (relu, grad_res) == (True, False) and len(bn3[2]) == 3
    assert _bits_equal(dyb, dy) and torch.equal(k3b, k3)
    assert _bits_equal(dy2d, dy.permute(0, 2, 3, 1).reshape(-1, 256))
    assert _bits_equal(dx2d.view(4, 16, 16, 256).permute(0, 3, 1, 2), dx1)
    _dt3, _dg, _db, dres = ext.bn_bwd(t3, dy, yb, k3, w3, m3, r3, True, True)
    dres2d = dres.permute(0, 2, 3, 1).reshape(-1, 256)
    gated = _gated(dy2d, k3)
    assert _bits_equal(dres2d, gated), "bn_bwd's gated gradient is not " \
        "dy under the mask bits"
    want = ext.gemm_bt_acc(dt1, w1bT, dres2d.clone())
    assert _bits_equal(dx2d, want), "gemm_bt_gate != gemm_bt_acc on dres"

    # ---- dx against fp64 on the recorded operands, with the bound
    # test_gpu_mfma.py::test_gemm_real holds gemm_bt_acc to on this tile
    S = dt1.double() @ w1bT.double().t()
    ref = S + gated.double()
    absprod = dt1.double().abs() @ w1bT.double().abs().t()
    _assert_bound("gemm_bt_gate in the block", dx2d, ref, absprod,
                  dt1.shape[1], BF16,
                  2.0 ** -24 * ref.abs() + _half_ulp(S, BF16))


def test_auto_rule():
    from tensorflowonspark_amd.ops import modules

    def join(n, c, hw, dtype=BF16):
        return torch.empty(n, c, hw, hw, dtype=dtype, device="meta")

    def mask(t):
        return torch.empty(t.numel() // 8, dtype=torch.uint8, device="meta")

    small = join(4, 256, 16)                     # the block tests' 0.5 MB join
    assert small.numel() * 2 == 512 * 1024
    assert not modules._bn_gate_route("auto", small, mask(small), 64)
    assert modules._bn_gate_route("force", small, mask(small), 64)
    assert not modules._bn_gate_route("off", small, mask(small), 64)
    # no mask in the per-vector byte format (a tier that gates from y), a
    # width with C % 8 != 0, fp32: the old route even under force
    none = torch.empty(0, dtype=torch.uint8, device="meta")
    assert not modules._bn_gate_route("force", small, none, 64)
    odd = join(4, 100, 16)
    assert not modules._bn_gate_route("force", odd, mask(odd), 64)
    f32 = join(4, 256, 16, torch.float32)
    assert not modules._bn_gate_route("force", f32, mask(f32), 64)
    # auto is a size threshold
    for n, c, hw in ((1024, 256, 56), (1024, 512, 28), (1024, 1024, 14),
                     (1024, 2048, 7)):
        t = join(n, c, hw)
        assert modules._bn_gate_route("auto", t, mask(t), c // 4) == \
            (t.numel() * 2 >= modules._BN_GATE_MIN_BYTES)
        assert not modules._bn_gate_route("off", t, mask(t), c // 4)
    assert modules._BN_GATE_MIN_BYTES > 512 * 1024


def test_mode_values(monkeypatch):
    from tensorflowonspark_amd.ops import modules
    monkeypatch.delenv("TFOS_BN_GATE", raising=False)
    assert modules._bn_gate_mode() == "auto"
    for v in ("auto", "off", "force"):
        monkeypatch.setenv("TFOS_BN_GATE", v)
        assert modules._bn_gate_mode() == v
    for v in ("on", "", "1", "Force"):
        monkeypatch.setenv("TFOS_BN_GATE", v)
        with pytest.raises(ValueError):
            modules._bn_gate_mode()
