"""softmax_cross_entropy on CPU tensors vs F.cross_entropy in fp64.

The CPU path is plain PyTorch, so it must agree with ``F.cross_entropy`` to
fp64 rounding wherever the two are defined alike, and differ exactly in the
two documented deviations: an all-ignored ``mean`` is 0 (torch: NaN), and a
target outside [0, C) that is not ``ignore_index`` counts as ignored (torch:
error).
"""

import pytest
import torch
import torch.nn.functional as F

from tensorflowonspark_amd.ops.modules import (SoftmaxCrossEntropy,
                                               softmax_cross_entropy)

# fp64 arithmetic in two different operation orders
TOL = dict(rtol=1e-12, atol=1e-12)


def _case(shape, ignore_index, seed=0):
    """fp64 logits and a target in which about a quarter of the entries,
    the first and the last among them, equal ignore_index."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(*shape, generator=g, dtype=torch.float64) * 3
    c = shape[1]
    tshape = (shape[0],) + tuple(shape[2:])
    target = torch.randint(0, c, tshape, generator=g)
    drop = torch.rand(tshape, generator=g) < 0.25
    drop.view(-1)[0] = True
    drop.view(-1)[-1] = True
    target[drop] = ignore_index
    return logits, target


@pytest.mark.parametrize("shape", [(37, 5), (2, 3, 5, 7)])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("ignore_index", [-100, 255])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_matches_torch_fp64(shape, reduction, ignore_index, eps):
    logits, target = _case(shape, ignore_index)
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    got = softmax_cross_entropy(a, target, reduction=reduction,
                                ignore_index=ignore_index, label_smoothing=eps)
    ref = F.cross_entropy(b, target, reduction=reduction,
                          ignore_index=ignore_index, label_smoothing=eps)
    assert got.dtype == torch.float64 and got.shape == ref.shape
    torch.testing.assert_close(got, ref, **TOL)
    w = torch.randn(ref.shape, dtype=torch.float64,
                    generator=torch.Generator().manual_seed(1))
    (got * w).sum().backward()
    (ref * w).sum().backward()
    torch.testing.assert_close(a.grad, b.grad, **TOL)
    ignored = (target == ignore_index)
    rows = a.grad.movedim(1, -1)[ignored]
    assert rows.numel() > 0 and (rows == 0).all()


def test_defaults_unchanged():
    """Default arguments and in-range targets: the value the function has
    always returned, the mean of the per-row fp32 losses."""
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(16, 10, generator=g)
    target = torch.randint(0, 10, (16,), generator=g)
    for red, ref in (("mean", lambda v: v.mean()), ("sum", lambda v: v.sum()),
                     ("none", lambda v: v)):
        got = softmax_cross_entropy(logits, target, reduction=red)
        want = ref(F.cross_entropy(logits.float(), target, reduction="none"))
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("shape", [(9, 4), (2, 3, 4, 4)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_ignored_mean_is_zero(shape, eps):
    logits, target = _case(shape, 255)
    target.fill_(255)
    a = logits.clone().requires_grad_()
    loss = softmax_cross_entropy(a, target, ignore_index=255,
                                 label_smoothing=eps)
    assert loss.item() == 0.0
    loss.backward()
    assert (a.grad == 0).all()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("bad", [7, -3])
def test_out_of_range_target_is_ignored(reduction, bad):
    logits, target = _case((21, 5), -100)
    target[4] = 2
    bad_target = target.clone()
    bad_target[4] = bad            # neither a class nor ignore_index
    ign_target = target.clone()
    ign_target[4] = -100
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    got = softmax_cross_entropy(a, bad_target, reduction=reduction,
                                label_smoothing=0.1)
    ref = F.cross_entropy(b, ign_target, reduction=reduction,
                          label_smoothing=0.1)
    torch.testing.assert_close(got, ref, **TOL)
    got.sum().backward()
    ref.sum().backward()
    torch.testing.assert_close(a.grad, b.grad, **TOL)
    assert (a.grad[4] == 0).all()


def test_module_wrapper():
    logits, target = _case((2, 3, 5, 7), 255)
    mod = SoftmaxCrossEntropy(reduction="sum", ignore_index=255,
                              label_smoothing=0.1)
    ref = F.cross_entropy(logits, target, reduction="sum", ignore_index=255,
                          label_smoothing=0.1)
    torch.testing.assert_close(mod(logits, target), ref, **TOL)
    assert "ignore_index=255" in repr(mod)
    # defaults are those of the function
    torch.testing.assert_close(
        SoftmaxCrossEntropy()(logits, target.clamp(max=2)),
        softmax_cross_entropy(logits, target.clamp(max=2)), **TOL)


def test_bad_arguments():
    logits, target = _case((4, 3), -100)
    with pytest.raises(ValueError):
        softmax_cross_entropy(logits, target, reduction="avg")
    with pytest.raises(ValueError):
        softmax_cross_entropy(logits, target, label_smoothing=1.5)
    with pytest.raises(ValueError):
        softmax_cross_entropy(logits, target[None])
