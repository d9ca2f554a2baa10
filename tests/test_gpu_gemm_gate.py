"""``gemm_bt_gate(a, b, dy, mask)``: the conv1 dgrad of an identity bottleneck
with the residual gradient gated in its epilogue (GATE in csrc/gemm_mfma.hip),
against the composition it replaces.

That composition is ``gemm_bt_acc(a, b, dres)`` on ``dres = dy where the mask
bit is set, +0 elsewhere``: what ``bn_bwd(..., relu, grad_res)`` used to write
out. ``dres`` is built here by a plain torch expression from ``dy`` and the
unpacked mask bits (bit j of byte v gates element 8 v + j of the row-major
[M, N] tensor). Both do bf16(float(bf16(acc)) + float(g)) per element, so the
outputs must agree bit for bit; ``gemm_bt_acc`` itself is pinned against fp64
by tests/test_gpu_mfma.py.

Shapes, from the launcher's rule (tfosr_gemm_bt_gate picks the tile
tfosr_gemm_bt_acc would): N % 128 != 0 and (N % 64 == 0 or N <= 64) takes the
256x64 tile, everything else the 128x128 tile; M >= 1024, N >= 192,
K >= 1024 would take the 256^2 kernel, which has no gating epilogue and is
reported ineligible. M = 421 leaves a ragged last M tile on both (4 tiles of
128 rows, 2 of 256); N = 72 takes the 128x128 tile, whose second column of
waves has only 8 live columns (one 16 B chunk per row, seven skipped); N = 192
is three N tiles of the 256x64 kernel.
"""

import pytest
import torch

from test_gpu_bn import BF16, _bits_equal, _ext, gpu, requires_gpu
from test_gpu_mfma import SKINNY, T128, T256, _gemm_tier

M, K = 421, 64
# (tier, N)
SHAPES = [(SKINNY, 64), (T128, 72), (T128, 128), (SKINNY, 192)]
MASKS = ["random", "zeros", "ones"]

_cache = {}


def _inputs(N):
    """a[M, K], b[N, K], dy[M, N] bf16 on the GPU; computed once per N and
    never written to."""
    if N not in _cache:
        gen = torch.Generator(device="cuda").manual_seed(1000 + N)
        a = torch.randn(M, K, device="cuda", generator=gen).to(BF16)
        b = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5) \
            .to(BF16)
        dy = torch.randn(M, N, device="cuda", generator=gen).to(BF16)
        dy[3, :8] = -0.0          # a gated -0 stays -0, an ungated one is +0
        rnd = torch.randint(0, 256, (M * N // 8,), device="cuda",
                            dtype=torch.uint8, generator=gen)
        _cache[N] = (a, b, dy, rnd)
    return _cache[N]


def _mask(kind, rnd):
    if kind == "random":
        return rnd.clone()
    return torch.full_like(rnd, 0 if kind == "zeros" else 255)


def _gated(dy, mask):
    """dy where its mask bit is set, +0 elsewhere: plain torch."""
    shifts = torch.arange(8, device=mask.device, dtype=torch.int32)
    bits = ((mask.to(torch.int32)[:, None] >> shifts[None, :]) & 1).bool()
    return torch.where(bits.reshape(dy.shape), dy, torch.zeros_like(dy))


def test_shapes_cover_the_launcher_rule():
    for tier, N in SHAPES:
        assert _gemm_tier(M, N, K)[0] == tier and N % 8 == 0
    assert {t for t, _ in SHAPES} == {SKINNY, T128}
    assert M % 128 != 0 and M % 256 != 0 and M > 256
    assert _gemm_tier(1024, 192, 1024)[0] == T256


@gpu
@requires_gpu
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("tier,N", SHAPES,
                         ids=["{}-N{}".format(*s) for s in SHAPES])
def test_gate_equals_acc_on_the_gated_tensor(tier, N, kind):
    ext = _ext()
    a, b, dy, rnd = _inputs(N)
    mask = _mask(kind, rnd)
    dy0, mask0 = dy.clone(), mask.clone()
    assert ext.gemm_bt_gate_eligible(M, N, K)
    dres = _gated(dy, mask)
    if kind == "ones":
        assert _bits_equal(dres, dy)
    elif kind == "zeros":
        assert not dres.view(torch.int16).any()
    want = ext.gemm_bt_acc(a, b, dres.clone())
    got = ext.gemm_bt_gate(a, b, dy, mask)
    torch.cuda.synchronize()
    assert got.shape == (M, N) and got.dtype == BF16 and got.is_contiguous()
    assert got.data_ptr() != dy.data_ptr()
    assert torch.isfinite(got).all()
    assert _bits_equal(got, want), "{} of {} elements differ".format(
        int((got.view(torch.int16) != want.view(torch.int16)).sum()),
        got.numel())
    assert _bits_equal(dy, dy0) and torch.equal(mask, mask0), \
        "gemm_bt_gate wrote to its inputs"
    again = ext.gemm_bt_gate(a, b, dy, mask)
    assert _bits_equal(again, got)


@gpu
@requires_gpu
def test_gate_rejects_bad_arguments():
    ext = _ext()
    a, b, dy, rnd = _inputs(64)
    ext.gemm_bt_gate(a, b, dy, rnd)
    bad = [
        (a.cpu(), b, dy, rnd), (a, b.cpu(), dy, rnd), (a, b, dy.cpu(), rnd),
        (a, b, dy, rnd.cpu()),                               # CPU tensors
        (a.float(), b, dy, rnd), (a, b.half(), dy, rnd),
        (a, b, dy.float(), rnd), (a, b, dy, rnd.to(torch.int8)),   # dtypes
        (a, b, dy, rnd[:-1]), (a, b, dy, torch.cat([rnd, rnd])),   # length
        (a, b, dy[:, :32], rnd), (a, b, dy.t(), rnd),
        (a, b, dy[:-1], rnd), (a.view(1, M, K), b, dy, rnd),
        (a, b, dy, rnd.view(-1, 8)[:, 0]),                   # strided mask
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.gemm_bt_gate(*args)
    # N % 8 != 0: a mask byte would straddle two rows
    n = 60
    assert not ext.gemm_bt_gate_eligible(M, n, K)
    with pytest.raises(RuntimeError):
        ext.gemm_bt_gate(a, b[:n].contiguous(), dy[:, :n].contiguous(),
                         rnd[:M * n // 8].contiguous())
    # the 256^2 kernel's shapes have no gating epilogue
    m2, n2, k2 = 1024, 192, 1024
    assert not ext.gemm_bt_gate_eligible(m2, n2, k2)
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ext.gemm_bt_gate(z(m2, k2, device="cuda", dtype=BF16),
                         z(n2, k2, device="cuda", dtype=BF16),
                         z(m2, n2, device="cuda", dtype=BF16),
                         z(m2 * n2 // 8, device="cuda", dtype=torch.uint8))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            ext.gemm_bt_gate(a, b, dy.to("cuda:1"), rnd)
        with pytest.raises(RuntimeError):
            ext.gemm_bt_gate(a, b, dy, rnd.to("cuda:1"))
