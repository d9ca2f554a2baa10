"""The NHWC row tier of csrc/bn_relu.hip (widths that are a multiple of the
vector but do not divide 2048) against the fp64 reference, bounds and exact
gate checks of test_gpu_bn.py, plus its plan, switch, determinism and its use
by the U-Net's MobileNetV2 block."""

import pytest
import torch

from test_gpu_bn import (BF16, EPS, FF, FP32, FT, GENERIC, NHWC, TF, TT,
                         _check, _eval_ref, _ext, _make_inputs,
                         _run_train_case, gpu, requires_gpu)

# (dtype, shape): see the plan each pins in the ids
SHAPES = [
    pytest.param(BF16, (3, 144, 5, 7),
                 id="bf16-3x144x5x7-cv18-idle-lanes-ragged-last-block"),
    pytest.param(BF16, (2, 576, 4, 4), id="bf16-2x576x4x4-most-idle-lanes"),
    pytest.param(BF16, (2, 960, 3, 3), id="bf16-2x960x3x3-p2"),
    pytest.param(FP32, (1, 960, 2, 2), id="fp32-1x960x2x2-p1-no-cross-lane"),
    pytest.param(BF16, (1, 24, 1, 3), id="bf16-1x24x1x3-m3-below-p"),
    pytest.param(FP32, (2, 40, 3, 5), id="fp32-2x40x3x5-cv10"),
    pytest.param(BF16, (8, 96, 28, 28), id="bf16-8x96x28x28-56-full-blocks"),
]


def _plan(dtype, shape, nhwc=True):
    n, c, h, w = shape
    return _ext().bn_rows_plan(n * c * h * w, c, dtype == BF16, nhwc)


@gpu
@requires_gpu
@pytest.mark.parametrize("relu,add", [FF, TF, TT, FT],
                         ids=["lin", "relu", "relu+res", "lin+res"])
@pytest.mark.parametrize("dtype,shape", SHAPES)
def test_bn_rows_train_matrix(dtype, shape, relu, add, monkeypatch):
    monkeypatch.delenv("TFOS_BN_ROWS", raising=False)
    blocks, lanes, threads = _plan(dtype, shape)
    cv = shape[1] // (8 if dtype == BF16 else 4)
    assert blocks > 0 and lanes == threads // cv and threads <= 256
    if shape == (8, 96, 28, 28):
        assert blocks >= 3
    _run_train_case(dtype, shape, NHWC, relu, add, GENERIC, 0.1)


@gpu
@requires_gpu
@pytest.mark.parametrize("add", [False, True], ids=["lin", "lin+res"])
def test_bn_rows_eval(add, monkeypatch):
    monkeypatch.delenv("TFOS_BN_ROWS", raising=False)
    for p in SHAPES + [pytest.param(FP32, (3, 144, 5, 7))]:
        assert _plan(*p.values)[0] > 0, p.values
    d = _make_inputs(BF16, (3, 144, 5, 7), NHWC, seed=11)
    res = d["res"] if add else None
    y = _ext().bn_fwd_eval(d["x"], res, d["w"], d["b"], d["rm0"], d["rv0"],
                           EPS, False)
    a = (d["x"], d["w"], d["b"], d["rm0"], d["rv0"], res, False)
    print()
    _check("eval y", y, _eval_ref(torch.float64, *a),
           _eval_ref(torch.float32, *a), BF16)


@gpu
@requires_gpu
def test_bn_rows_leaves_other_shapes_alone(monkeypatch):
    monkeypatch.delenv("TFOS_BN_ROWS", raising=False)
    assert _plan(FP32, (2, 1280, 2, 2))[0] == 0      # Cv = 320
    assert _plan(BF16, (4, 12, 7, 7))[0] == 0        # C % V != 0
    assert _plan(BF16, (4, 96, 7, 7), nhwc=False)[0] == 0
    assert _plan(BF16, (4, 64, 7, 7))[0] == 0        # the fast path's
    assert _ext().bn_fast_blocks(4 * 96 * 49, 96, True, True) == 0
    _run_train_case(FP32, (2, 1280, 2, 2), NHWC, True, True, GENERIC)


@gpu
@requires_gpu
def test_bn_rows_switch(monkeypatch):
    shape = (3, 144, 5, 7)
    monkeypatch.setenv("TFOS_BN_ROWS", "off")
    assert _plan(BF16, shape) == (0, 0, 0)
    _run_train_case(BF16, shape, NHWC, True, True, GENERIC)
    monkeypatch.setenv("TFOS_BN_ROWS", "on")
    assert _plan(BF16, shape)[0] > 0
    monkeypatch.setenv("TFOS_BN_ROWS", "rows")
    d = _make_inputs(BF16, shape, NHWC, seed=0)
    with pytest.raises(RuntimeError, match="TFOS_BN_ROWS"):
        _ext().bn_fwd_train(d["x"], None, d["w"], d["b"], d["rm0"].clone(),
                            d["rv0"].clone(), 0.1, EPS, True)
    with pytest.raises(RuntimeError, match="TFOS_BN_ROWS"):
        _ext().bn_fwd_eval(d["x"], None, d["w"], d["b"], d["rm0"], d["rv0"],
                           EPS, True)


@gpu
@requires_gpu
def test_bn_rows_bit_identical_between_runs(monkeypatch):
    monkeypatch.delenv("TFOS_BN_ROWS", raising=False)
    ext = _ext()
    d = _make_inputs(BF16, (8, 96, 28, 28), NHWC, seed=4)

    def run():
        y, mean, rstd, mask = ext.bn_fwd_train(
            d["x"], d["res"], d["w"], d["b"], d["rm0"].clone(),
            d["rv0"].clone(), 0.1, EPS, True)
        dx, dgamma, dbeta, _ = ext.bn_bwd(d["x"], d["dy"], y, mask, d["w"],
                                          mean, rstd, True, True)
        return y, mean, rstd, dx, dgamma, dbeta

    first, second = run(), run()
    for name, a, b in zip(("y", "save_mean", "save_rstd", "dx", "dgamma",
                           "dbeta"), first, second):
        assert torch.equal(a, b), name


@gpu
@requires_gpu
def test_inverted_residual_runs_three_fused_bns(monkeypatch):
    from tensorflowonspark_amd.models.segmentation import InvertedResidual
    monkeypatch.delenv("TFOS_BN_ROWS", raising=False)
    ext = _ext()
    torch.manual_seed(0)
    blk = InvertedResidual(24, 24, 1).cuda().train()
    x = torch.randn(2, 24, 8, 8, device="cuda").contiguous(
        memory_format=torch.channels_last).requires_grad_()
    with_res = []
    orig = ext.bn_fwd_train

    def counted(x_, res, *a):
        with_res.append(res is not None)
        return orig(x_, res, *a)

    monkeypatch.setattr(ext, "bn_fwd_train", counted)
    with torch.autocast("cuda", dtype=BF16):
        y = blk(x)
    y.float().sum().backward()
    assert with_res == [False, False, True]   # expand, depthwise, project
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert x.grad.abs().max() > 0
    for n, p in blk.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
