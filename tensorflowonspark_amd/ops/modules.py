"""Fused-op modules: HIP/CDNA4 kernels on GPU, plain PyTorch on CPU.

Each op the reference delegated to TensorFlow's runtime (survey §2.3) appears
here as a PyTorch-composable module/function whose CUDA-tensor path calls the
hand-written gfx950 kernel from ``csrc/`` and whose CPU path is the fp32
reference implementation the numerics tests compare against.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import get_ext
from .packplan import (EagerPacks, _class_taps, flipped, im2col,
                       parity_class, rows, rows_t, stem_w224)


def _cl_bf16(t):
    """An upstream gradient as the kernels take it: channels_last bf16."""
    return t.contiguous(memory_format=torch.channels_last).to(torch.bfloat16)


def _cl_alloc(shape, device, dtype=torch.bfloat16, zero=False):
    """A fresh tensor of ``shape`` that is channels_last from birth.

    ``torch.empty(shape).contiguous(memory_format=torch.channels_last)``
    allocates an NCHW tensor, then a second one, and runs a strided permuting
    copy of uninitialised memory between them: a whole-tensor read and write
    per call. The strides here are the ones that expression ends with: where
    NCHW memory already is channels_last-contiguous (one channel, or a 1x1
    image) it kept the NCHW strides, and so does this."""
    shape = tuple(shape)
    nchw_is_cl = len(shape) == 4 and (shape[1] == 1 or shape[2:] == (1, 1))
    t = torch.empty(shape, device=device, dtype=dtype,
                    memory_format=torch.contiguous_format if nchw_is_cl
                    else torch.channels_last)
    return t.zero_() if zero else t


def as2d(t):
    """channels_last [N, C, H, W] viewed as the [N*H*W, C] GEMM operand."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def as4d(t2d, n, h, w):
    return t2d.view(n, h, w, -1).permute(0, 3, 1, 2)


def _use_wrw2(k, cin, cout, mode=None):
    """Does TFOS_WRW (``mode``; None reads the environment) send this shape
    to the transpose-read kernel conv_wrw2? auto (default, and any unknown
    string) routes each shape to the measured-faster implementation (MI355X
    b1024, see profiles/README.md — the in-tree kernel wins on small-channel
    3x3 and is within 0.75-1.2x of the library igemm elsewhere); mfma2
    forces the in-tree kernel, miopen and mfma do not use it."""
    if mode is None:
        mode = os.environ.get("TFOS_WRW", "auto")
    if mode == "mfma2":
        return True
    if mode in ("miopen", "mfma"):
        return False
    return k == 3 and cin <= 64 and cout <= 64


def _wrw_backend(mode, k, cin, cout, stride, fd=1, transposed=False,
                 round1=True):
    """Which implementation computes a conv's weight gradient under
    TFOS_WRW=mode: 'wrw2', 'wrw' or 'lib'. See _weight_grad."""
    ch8 = cin % 8 == 0 and cout % 8 == 0
    if transposed:
        return "lib"
    if ch8 and _use_wrw2(k, cin, cout, mode):
        return "wrw2"
    if round1 and mode == "mfma" and stride == 1 and fd == 1 and ch8:
        return "wrw"
    return "lib"


def _lib_conv_backward(dy, x, weight, stride, pad, fd, transposed, mask):
    """(dx, dw) of a conv from the library, each where mask says so."""
    w4 = weight.to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    gx, gw, _ = torch.ops.aten.convolution_backward(
        dy, x, w4, None, [stride, stride], [pad, pad], [fd, fd], transposed,
        [0, 0], 1, [mask[0], mask[1], False])
    return gx, gw


def _weight_grad(dy, x, weight, k, stride, pad, fd=1, transposed=False,
                 round1=True):
    """dW of a k x k conv (filter dilation fd; ``transposed``: of a
    ConvTranspose2d) from channels_last bf16 dy and the saved input x, in
    the weight's own shape and dtype. The one place TFOS_WRW is acted on:

      conv_wrw2  the transpose-read MFMA kernel (any stride and dilation),
                 where _use_wrw2 says so: under mfma2 always, under auto for
                 3x3 with both channel counts <= 64; channels % 8 == 0
      conv_wrw   the round-1 TN kernel, kept for comparison: only under
                 mfma, stride 1, undilated, channels % 8 == 0, and not
                 where the caller passes round1=False
      library    _lib_conv_backward (aten, on a channels_last bf16 weight):
                 everything else (miopen, most of auto), every transposed conv
    """
    cout, cin = weight.shape[0], weight.shape[1]
    backend = _wrw_backend(os.environ.get("TFOS_WRW", "auto"), k, cin, cout,
                           stride, fd, transposed, round1)
    if backend == "lib":
        dw = _lib_conv_backward(dy, x, weight, stride, pad, fd, transposed,
                                (False, True))[1]
        return dw.to(weight.dtype)
    ext = get_ext(required=True)
    if backend == "wrw2":
        dw = ext.conv_wrw2(dy, x, k, k, stride, pad,
                           **({"fd": fd} if fd != 1 else {}))
    else:
        dw = ext.conv_wrw(dy, x, k, k, pad)
    # [Cout, taps*Cin], tap-major, back to [Cout, Cin, k, k]
    dw = dw.view(cout, cin, 1, 1) if k == 1 else \
        dw.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()
    return dw.to(weight.dtype)


# ---------------------------------------------------------------------------
# Fused BatchNorm + ReLU (training fwd/bwd, inference fwd)
# ---------------------------------------------------------------------------

class _FusedBNFn(torch.autograd.Function):
    """BN (+residual add) (+ReLU) with fused CDNA4 kernels.

    relu gating in backward uses sign(y); with the residual variant the gated
    upstream gradient doubles as the residual-branch gradient (one pass)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var,
                momentum, eps, relu):
        ext = get_ext(required=True)
        y, save_mean, save_rstd, mask = ext.bn_fwd_train(
            x, res, weight, bias, running_mean, running_var, momentum, eps, relu)
        ctx.save_for_backward(x, y, mask, weight, save_mean, save_rstd)
        ctx.relu = relu
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        x, y, mask, weight, save_mean, save_rstd = ctx.saved_tensors
        out = ext.bn_bwd(x, dy, y, mask, weight, save_mean, save_rstd,
                         ctx.relu, ctx.has_res)
        if ctx.has_res:
            dx, dweight, dbias, dres = out
        else:
            (dx, dweight, dbias), dres = out, None
        return dx, dres, dweight, dbias, None, None, None, None, None


class FusedBNReLU(nn.Module):
    """BatchNorm2d (+ residual add) (+ ReLU) in one HBM pass per stage.

    These ops are HBM-bandwidth-bound on MI355X; fusing normalize, residual
    add and activation into the stat/normalize kernels removes whole-tensor
    round trips vs the unfused composition, and the backward emits the
    residual gradient from the same pass that reduces dgamma/dbeta.
    """

    RELU = True
    ADD = False

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x, res=None):
        assert (res is not None) == self.ADD, "residual arg mismatch"
        if x.is_cuda:
            # preserve channels_last; otherwise force standard contiguity
            if not x.is_contiguous(memory_format=torch.channels_last):
                x = x.contiguous()
            if res is not None:
                if x.is_contiguous(memory_format=torch.channels_last):
                    res = res.contiguous(memory_format=torch.channels_last)
                else:
                    res = res.contiguous()
            if self.training:
                self.num_batches_tracked += 1
                return _FusedBNFn.apply(
                    x, res, self.weight, self.bias, self.running_mean,
                    self.running_var, self.momentum, self.eps, self.RELU)
            ext = get_ext(required=True)
            if ext is not None:
                return ext.bn_fwd_eval(x, res, self.weight, self.bias,
                                       self.running_mean, self.running_var,
                                       self.eps, self.RELU)
        # CPU / fallback reference path
        y = F.batch_norm(x, self.running_mean, self.running_var, self.weight,
                         self.bias, self.training, self.momentum, self.eps)
        if res is not None:
            y = y + res
        return F.relu(y, inplace=True) if self.RELU else y

    def extra_repr(self):
        return "{}, eps={}, momentum={}, relu={}, add={}".format(
            self.num_features, self.eps, self.momentum, self.RELU, self.ADD)


class FusedBN(FusedBNReLU):
    """Plain fused BatchNorm2d (no activation)."""
    RELU = False
    ADD = False


class FusedBNAddReLU(FusedBNReLU):
    """y = relu(bn(x) + residual) — the ResNet block tail as one op."""
    RELU = True
    ADD = True


# ---------------------------------------------------------------------------
# Fused softmax cross-entropy (sparse labels, ignore_index, label smoothing)
# ---------------------------------------------------------------------------

_XENT_REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}


class _XentNoneFn(torch.autograd.Function):
    """Per-row loss; backward recomputes the softmax from the saved lse."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, label_smoothing):
        ext = get_ext(required=True)
        loss, lse, _ = ext.xent_dense_fwd(logits, target, ignore_index,
                                          label_smoothing, 0, 0)
        ctx.save_for_backward(logits, lse, target)
        ctx.args = (ignore_index, label_smoothing)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ext = get_ext(required=True)
        logits, lse, target = ctx.saved_tensors
        dlogits = ext.xent_dense_bwd(logits, lse, target,
                                     grad_out.float().contiguous(), None,
                                     ctx.args[0], ctx.args[1], 0, 0)
        return dlogits, None, None, None


class _XentReducedFn(torch.autograd.Function):
    """sum / mean without a per-row loss tensor: the forward leaves the loss
    and the valid-row count on the device, and the backward kernel reads the
    upstream scalar and the count from there."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, label_smoothing, reduction):
        ext = get_ext(required=True)
        loss, lse, nvalid = ext.xent_dense_fwd(logits, target, ignore_index,
                                               label_smoothing, reduction, 0)
        ctx.save_for_backward(logits, lse, target, nvalid)
        ctx.args = (ignore_index, label_smoothing, reduction)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ext = get_ext(required=True)
        logits, lse, target, nvalid = ctx.saved_tensors
        dlogits = ext.xent_dense_bwd(logits, lse, target, grad_out.float(),
                                     nvalid, ctx.args[0], ctx.args[1],
                                     ctx.args[2], 0)
        return dlogits, None, None, None, None


def _xent_cpu(logits, target, reduction, ignore_index, label_smoothing):
    """Plain PyTorch: F.cross_entropy plus the two documented deviations."""
    c = logits.shape[1]
    x = logits if logits.dtype in (torch.float32, torch.float64) \
        else logits.float()
    out_of_range = (target < 0) | (target >= c)
    target = torch.where(out_of_range, torch.full_like(target, ignore_index),
                         target)
    loss = F.cross_entropy(x, target, reduction="none",
                           ignore_index=ignore_index,
                           label_smoothing=label_smoothing)
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    nvalid = (target != ignore_index).sum()
    return loss.sum() / nvalid.clamp(min=1).to(loss.dtype)


def softmax_cross_entropy(logits, target, reduction="mean", ignore_index=-100,
                          label_smoothing=0.0):
    """Sparse softmax cross-entropy (reference workloads:
    ``sparse_categorical_crossentropy``, e.g. ``mnist_spark.py:22``,
    ``resnet_cifar_dist.py:210``), with the arguments and semantics of
    ``F.cross_entropy``.

    ``logits`` is ``(P, C)`` with ``target`` ``(P,)``, or ``(N, C, d1, ...)``
    with ``target`` ``(N, d1, ...)``. On the GPU every shape runs on the
    gfx950 kernels of ``csrc/softmax_xent_dense.hip`` without a copy of the
    logits (2-D, standard-contiguous N-D and channels_last 4-D; any other
    striding is made contiguous first) and without a host synchronisation.
    The loss is fp32.

    Two deliberate deviations from ``F.cross_entropy``, on CPU and GPU alike:

    * ``mean`` over a batch in which every row is ignored is 0 with all-zero
      gradients (torch: NaN), so one all-void batch cannot poison a gradient
      all-reduce;
    * a target outside ``[0, C)`` that is not ``ignore_index`` is treated as
      ignored (torch: device assert); no kernel indexes the logits with it.
    """
    if reduction not in _XENT_REDUCTIONS:
        raise ValueError("reduction must be 'none', 'sum' or 'mean', got {!r}"
                         .format(reduction))
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError("label_smoothing must be in [0, 1], got {}"
                         .format(label_smoothing))
    if logits.dim() < 2 or target.dim() != logits.dim() - 1:
        raise ValueError("expected logits (P, C) or (N, C, d1, ...) and a "
                         "target without the class dimension")
    ignore_index = int(ignore_index)
    label_smoothing = float(label_smoothing)
    if not logits.is_cuda:
        return _xent_cpu(logits, target, reduction, ignore_index,
                         label_smoothing)
    get_ext(required=True)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    if not (logits.is_contiguous() or (
            logits.dim() == 4
            and logits.is_contiguous(memory_format=torch.channels_last))):
        logits = logits.contiguous()
    target = target.contiguous()
    if reduction == "none":
        return _XentNoneFn.apply(logits, target, ignore_index, label_smoothing)
    return _XentReducedFn.apply(logits, target, ignore_index, label_smoothing,
                                _XENT_REDUCTIONS[reduction])


class SoftmaxCrossEntropy(nn.Module):
    """Module form of :func:`softmax_cross_entropy` (same arguments)."""

    def __init__(self, reduction="mean", ignore_index=-100,
                 label_smoothing=0.0):
        super().__init__()
        self.reduction = reduction
        self.ignore_index = ignore_index
        self.label_smoothing = label_smoothing

    def forward(self, logits, target):
        return softmax_cross_entropy(logits, target, self.reduction,
                                     self.ignore_index, self.label_smoothing)

    def extra_repr(self):
        return "reduction={}, ignore_index={}, label_smoothing={}".format(
            self.reduction, self.ignore_index, self.label_smoothing)


# ---------------------------------------------------------------------------
# NHWC uint8 -> NCHW float/bf16 normalize (the DataFeed->GPU ingest kernel)
# ---------------------------------------------------------------------------

def nhwc_pack(images_u8, mean=None, std=None, out_dtype=torch.bfloat16,
              scale=1.0 / 255, channels_last=False):
    """Decode/pack kernel: NHWC uint8 batch -> normalized NCHW tensor.

    GPU path is one fused kernel (read u8 once, write out_dtype once);
    ``channels_last=True`` keeps the memory order (NHWC *is* channels_last), so
    the pack is a pure vectorized normalize. CPU path is the reference
    composition.
    """
    if images_u8.is_cuda:
        ext = get_ext(required=True)
        if ext is not None:
            dev = images_u8.device
            m = mean if mean is not None else torch.zeros(
                images_u8.shape[-1], device=dev)
            s = std if std is not None else torch.ones(
                images_u8.shape[-1], device=dev)
            # the kernel reads C consecutive floats through a raw pointer
            m = torch.as_tensor(m).to(device=dev, dtype=torch.float32) \
                .contiguous()
            s = torch.as_tensor(s).to(device=dev, dtype=torch.float32) \
                .contiguous()
            return ext.nhwc_pack(images_u8.contiguous(), m, s,
                                 float(scale), out_dtype == torch.bfloat16,
                                 channels_last)
    x = images_u8.to(torch.float32) * scale
    if mean is not None:
        x = x - mean
    if std is not None:
        x = x / std
    x = x.permute(0, 3, 1, 2)
    if channels_last:
        return x.contiguous(memory_format=torch.channels_last).to(out_dtype)
    return x.contiguous().to(out_dtype)


# ---------------------------------------------------------------------------
# Fused flat SGD-with-momentum (one kernel per DDP bucket)
# ---------------------------------------------------------------------------

class BucketSGD:
    """SGD(momentum, weight_decay) operating on DDPEngine flat buckets.

    With flattened params+grads, the whole model updates in a handful of
    kernel launches (one per bucket) instead of one per parameter tensor —
    the launch-bound tail of every small-op optimizer loop disappears.
    """

    def __init__(self, engine, lr=0.1, momentum=0.9, weight_decay=0.0,
                 nesterov=False):
        self.engine = engine
        self.lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.nesterov = nesterov
        self._mom = []
        for bucket in engine._buckets:
            self._mom.append(torch.zeros_like(bucket.buffer))

    @torch.no_grad()
    def step(self):
        for bucket, mom in zip(self.engine._buckets, self._mom):
            pf = getattr(bucket, "param_flat", None)
            g = bucket.buffer
            if pf is None:
                # non-flattened params: per-param foreach update
                params = bucket.params
                grads = [bucket.views[p] for p in params]
                moms = []
                off = 0
                for p in params:
                    moms.append(mom[off:off + p.numel()].view_as(p))
                    off += p.numel()
                if self.weight_decay:
                    torch._foreach_add_([g_.view(-1) for g_ in grads],
                                        [p.data.view(-1) for p in params],
                                        alpha=self.weight_decay)
                torch._foreach_mul_(moms, self.momentum)
                torch._foreach_add_(moms, grads)
                upd = moms
                if self.nesterov:
                    upd = torch._foreach_add(grads, moms, alpha=self.momentum)
                torch._foreach_add_([p.data for p in params], upd, alpha=-self.lr)
                continue
            ext = get_ext(required=True) if g.is_cuda else None
            if ext is not None:
                ext.sgd_step(pf, g, mom, self.lr, self.momentum,
                             self.weight_decay, self.nesterov)
            else:
                if self.weight_decay:
                    g = g.add(pf, alpha=self.weight_decay)
                mom.mul_(self.momentum).add_(g)
                upd = g.add(mom, alpha=self.momentum) if self.nesterov else mom
                pf.add_(upd, alpha=-self.lr)

    def zero_grad(self):
        self.engine.zero_grad()


# ---------------------------------------------------------------------------
# Fused NHWC MaxPool2d (argmax saved as a packed window index)
# ---------------------------------------------------------------------------

class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        ext = get_ext(required=True)
        y, idx = ext.maxpool_fwd(x, k, s, p)
        ctx.save_for_backward(idx)
        ctx.params = (x.shape[2], x.shape[3], k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        (idx,) = ctx.saved_tensors
        H, W, k, s, p = ctx.params
        dx = ext.maxpool_bwd(dy, idx, H, W, k, s, p)
        return dx, None, None, None


class FusedMaxPool2d(nn.Module):
    """channels_last MaxPool2d; backward is an atomic-free gather over the
    (at most ceil(K/S)^2) windows covering each input pixel."""

    def __init__(self, kernel_size=3, stride=2, padding=1):
        super().__init__()
        self.k, self.s, self.p = kernel_size, stride, padding

    def forward(self, x):
        if x.is_cuda and x.is_contiguous(memory_format=torch.channels_last) \
                and x.shape[1] % (8 if x.dtype == torch.bfloat16 else 4) == 0 \
                and get_ext(required=True) is not None:
            return _MaxPoolFn.apply(x, self.k, self.s, self.p)
        return F.max_pool2d(x, self.k, self.s, self.p)

    def extra_repr(self):
        return "k={}, s={}, p={}".format(self.k, self.s, self.p)


# ---------------------------------------------------------------------------
# 1x1 convolution as an MFMA GEMM (channels_last)
# ---------------------------------------------------------------------------

class _Conv1x1S2Fn(torch.autograd.Function):
    """Stride-2 1x1 conv (ResNet downsample path) on the implicit-GEMM MFMA
    kernel: forward is taps=1/S=2; backward-data is the input-dilated (D=2)
    variant of the same kernel (dx = scatter of dy @ W, computed gather-side);
    weight-grad: _weight_grad."""

    @staticmethod
    def forward(ctx, x, weight):
        ext = get_ext(required=True)
        if x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        y = ext.conv_mfma(x, rows(weight), weight.shape[0], 1, 1, 2, 0, 1,
                          -1, -1)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        Cout, Cin = weight.shape[0], weight.shape[1]
        dy = _cl_bf16(dy)
        # dx[h,w] = (h,w even) ? dy[h/2,w/2] @ W : 0 — only the even-even
        # parity class has a tap; zero-fill and launch just that class
        dx = _cl_alloc(x.shape, x.device, zero=True)
        _conv_parity(dy, rows_t(weight).view(Cin, 1, 1, Cout), dx, 1, 0)
        return dx, _weight_grad(dy, x, weight, 1, 2, 0)


class _Conv1x1Fn(torch.autograd.Function):
    """Stride-1 1x1 conv on channels_last tensors == GEMM over [N*H*W, Cin].

    forward / input-grad run on the hand-written gfx950 MFMA kernel
    (C = A @ B^T, K-contiguous operands); the weight-grad contraction
    (dW = dy^T @ x, a reduction over the huge M dim): _weight_grad."""

    @staticmethod
    def forward(ctx, x, weight):
        ext = get_ext(required=True)
        N, _, H, W = x.shape
        # channels_last storage viewed as the [M, Cin] activation matrix
        x2d = as2d(x)
        if x2d.dtype != torch.bfloat16:
            x2d = x2d.to(torch.bfloat16)
        w2d = rows(weight)
        y2d = ext.gemm_bt(x2d, w2d, True)
        ctx.save_for_backward(x2d, w2d, weight)
        return as4d(y2d, N, H, W)

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        x2d, w2d, weight = ctx.saved_tensors
        N, _, H, W = dy.shape
        dy = _cl_bf16(dy)
        # dx[M,Cin] = dy[M,Cout] @ W[Cout,Cin]  ->  gemm_bt(dy, W^T)
        dx = as4d(ext.gemm_bt(as2d(dy), rows_t(w2d), True), N, H, W)
        return dx, _weight_grad(dy, as4d(x2d, N, H, W), weight, 1, 1, 0)


class Conv1x1(nn.Module):
    """Pointwise convolution routed to the MFMA GEMM on GPU (stride 1) or the
    implicit-GEMM conv kernel (stride 2 — the ResNet downsample conv).

    Backend select via TFOS_CONV1X1: 'mfma' (default), 'blas'
    (torch.matmul / hipBLASLt for A/B comparison), 'miopen' (F.conv2d).
    Weight kept in Conv2d's [Cout, Cin, 1, 1] shape for state_dict parity.
    """

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.stride = stride
        self.weight = nn.Parameter(torch.empty(cout, cin, 1, 1))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        # stride-2 backward-data needs K = Cout % 32 == 0 as well
        self._s2_ok = stride == 2 and cin % 32 == 0 and cout % 32 == 0

    def forward(self, x):
        backend = os.environ.get("TFOS_CONV1X1", "mfma")
        # the MFMA kernel is bf16-only: a silent downcast would corrupt a
        # claimed-fp32 run, so other dtypes use the library conv
        if x.is_cuda and x.dtype == torch.bfloat16 and backend != "miopen":
            x = x.contiguous(memory_format=torch.channels_last)
            if self.stride == 2:
                if self._s2_ok and get_ext(required=True) is not None:
                    return _Conv1x1S2Fn.apply(x, self.weight)
                return F.conv2d(x, self.weight.to(x.dtype), stride=self.stride)
            if backend == "blas":
                N, Cin, H, W = x.shape
                x2d = x.permute(0, 2, 3, 1).reshape(-1, Cin)
                w = self.weight.view(self.weight.shape[0], Cin)
                if x2d.dtype == torch.bfloat16:
                    w = w.to(torch.bfloat16)
                y2d = x2d @ w.t()
                return y2d.view(N, H, W, -1).permute(0, 3, 1, 2)
            if get_ext(required=True) is not None:
                return _Conv1x1Fn.apply(x, self.weight)
        return F.conv2d(x, self.weight.to(x.dtype), stride=self.stride)

    def extra_repr(self):
        return "{}x{} pointwise s{} (MFMA)".format(
            self.weight.shape[1], self.weight.shape[0], self.stride)


# ---------------------------------------------------------------------------
# 3x3 convolution as an implicit MFMA GEMM (channels_last, stride 1)
# ---------------------------------------------------------------------------

class _Conv3x3Fn(torch.autograd.Function):
    """3x3/pad-1 conv (stride 1 or 2) on channels_last bf16 via the
    4-deep-pipelined implicit-GEMM kernel. dgrad = dilated-input conv of dy
    with the flipped/transposed weight (same kernel, D=S; parity-decomposed
    for stride 2); wrw: _weight_grad."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        ext = get_ext(required=True)
        if x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        y = ext.conv_mfma(x, im2col(weight), weight.shape[0], 3, 3, stride,
                          1, 1, -1, -1)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        S = ctx.stride
        Cout, Cin = weight.shape[0], weight.shape[1]
        dy = _cl_bf16(dy)
        wperm = flipped(weight)
        if S == 2:
            dx = _cl_alloc(x.shape, x.device)
            _conv_parity(dy, wperm, dx, 3, 1)
        else:
            dx = get_ext(required=True).conv_mfma(
                dy, wperm.reshape(Cin, 9 * Cout), Cin, 3, 3, 1, 1, 1,
                x.shape[2], x.shape[3])
        return dx, _weight_grad(dy, x, weight, 3, S, 1), None


class Conv3x3(nn.Module):
    """3x3/pad-1 conv (stride 1 or 2) routed to the implicit-GEMM MFMA kernel.

    Backend select via TFOS_CONV3X3: 'mfma' (default), 'miopen'.
    Weight in Conv2d's [Cout, Cin, 3, 3] shape for state_dict parity.
    """

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.stride = stride
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        self._eligible = cin % 32 == 0 and cout % 32 == 0 and cout >= 64 \
            and stride in (1, 2)

    def forward(self, x):
        backend = os.environ.get("TFOS_CONV3X3", "mfma")
        if x.is_cuda and self._eligible and backend == "mfma" \
                and x.dtype == torch.bfloat16 \
                and get_ext(required=True) is not None:
            x = x.contiguous(memory_format=torch.channels_last)
            return _Conv3x3Fn.apply(x, self.weight, self.stride)
        return F.conv2d(x, self.weight.to(x.dtype), padding=1,
                        stride=self.stride)

    def extra_repr(self):
        return "{}x{} 3x3 s{} (implicit-GEMM MFMA)".format(
            self.weight.shape[1], self.weight.shape[0], self.stride)


# ---------------------------------------------------------------------------
# Atrous (filter-dilated) 3x3 convolution on the same implicit-GEMM kernels
# ---------------------------------------------------------------------------

def live_taps(H, W, k, stride, pad, fd):
    """Filter taps of a k x k conv with filter dilation ``fd`` that reach at
    least one input pixel of an H x W image for some output pixel.

    Returns ``(rows, cols)``, two tuples of tap indices. Tap row ``r`` reads
    input row ``oh*stride - pad + r*fd``; it is dead when that index lies in
    the padding for every output row ``oh``. Pure Python, no tensor needed.
    """
    def axis(L):
        out_len = (L + 2 * pad - fd * (k - 1) - 1) // stride + 1
        live = []
        for t in range(k):
            c = t * fd - pad
            # first output index whose read is not left of the image
            o = 0 if c >= 0 else (-c + stride - 1) // stride
            if o < out_len and o * stride + c < L:
                live.append(t)
        return tuple(live)
    return axis(H), axis(W)


def _atrous_auto(path, M, cin, cout):
    """TFOS_ATROUS=auto policy: is ``path`` ('fwd', 'dgrad' or 'collapse')
    of an atrous conv over M = N*H*W pixels routed to the in-tree kernels?

    Follows the isolated measurement at the DeepLabV3 shapes (b32, 32x32
    map; tools/conv_bench.py --atrous, docs/performance.md "Atrous
    convolutions"), where a path goes in-tree only if its median, weight
    re-layout included, was no slower than the library's:

      collapse (rate 36)       7x faster forward, 6x dgrad      -> in-tree
      512->512 d2   fwd/dgrad  0.17 / 0.19 vs 0.27 / 0.25 ms    -> in-tree
      2048->256     dgrad      0.33 vs 0.44 ms                  -> in-tree
      2048->256     fwd        0.54 vs 0.51 ms                  -> library

    The one losing launch is the one with 128 workgroups (256-row x
    256-column tiles, Cout = 256) on a 256-CU chip; every winning launch
    has at least 256. That count is the rule, so shapes that were not
    measured stay on the library unless they fill the chip as well."""
    if path == "collapse":
        return True
    n_out = cout if path == "fwd" else cin
    tile_n = 256 if n_out >= 192 else 128
    n_wg = ((M + 255) // 256) * ((n_out + tile_n - 1) // tile_n)
    return n_wg >= 256


def _atrous_route(N, H, W, cin, cout, fd):
    """(collapse, fwd_in_tree, dgrad_in_tree) for TFOS_ATROUS, or None for
    the plain library conv."""
    mode = os.environ.get("TFOS_ATROUS", "auto")
    if mode == "miopen":
        return None
    if mode not in ("auto", "mfma"):
        raise ValueError("TFOS_ATROUS must be auto, mfma or miopen, got "
                         + repr(mode))
    centre_only = live_taps(H, W, 3, 1, fd, fd) == ((1,), (1,))
    if mode == "mfma":
        return centre_only, True, True
    M = N * H * W
    if centre_only and _atrous_auto("collapse", M, cin, cout):
        return True, True, True
    fwd = _atrous_auto("fwd", M, cin, cout)
    dgrad = _atrous_auto("dgrad", M, cin, cout)
    if not (fwd or dgrad):
        return None
    return False, fwd, dgrad


class _AtrousConv3x3Fn(torch.autograd.Function):
    """3x3 conv with filter dilation fd, stride 1, padding fd, on
    channels_last bf16. Forward is the implicit-GEMM kernel with tap offsets
    (r*fd, s*fd); dgrad is the SAME kernel run on dy with the flipped and
    transposed weight, dilation fd and pad 2*fd - fd = fd; wrw: _weight_grad
    with the same tap offsets. A forward or dgrad routed to the library goes
    through aten."""

    @staticmethod
    def forward(ctx, x, weight, fd, fwd_in_tree, dgrad_in_tree):
        if fwd_in_tree:
            y = get_ext(required=True).conv_mfma(
                x, im2col(weight), weight.shape[0], 3, 3, 1, fd, 1, -1, -1,
                fd=fd)
        else:
            y = F.conv2d(x, weight.to(torch.bfloat16), None, 1, fd, fd)
        ctx.save_for_backward(x, weight)
        ctx.fd = fd
        ctx.dgrad_in_tree = dgrad_in_tree
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        fd = ctx.fd
        Cout, Cin = weight.shape[0], weight.shape[1]
        dy = _cl_bf16(dy)
        dx = dw = None
        if ctx.needs_input_grad[0] and ctx.dgrad_in_tree:
            dx = get_ext(required=True).conv_mfma(
                dy, flipped(weight).reshape(Cin, 9 * Cout), Cin, 3, 3,
                1, 2 * fd - fd, 1, x.shape[2], x.shape[3], fd=fd)
        elif ctx.needs_input_grad[0]:
            dx = _lib_conv_backward(dy, x, weight, 1, fd, fd, False,
                                    (True, False))[0]
        if ctx.needs_input_grad[1]:
            dw = _weight_grad(dy, x, weight, 3, 1, fd, fd)
        return dx, dw, None, None, None


class _AtrousCollapsedFn(torch.autograd.Function):
    """Atrous 3x3 conv whose dilation is at least the image size (padding =
    dilation, stride 1): the eight outer taps only ever read padding, so the
    conv IS the 1x1 conv of the centre tap. Forward, dgrad and wrw are the
    Conv1x1 paths on weight[:, :, 1, 1]; dW is exactly zero at the dead
    taps."""

    @staticmethod
    def forward(ctx, x, weight):
        Cout, Cin = weight.shape[0], weight.shape[1]
        wc = weight[:, :, 1, 1].contiguous().view(Cout, Cin, 1, 1)
        return _Conv1x1Fn.forward(ctx, x, wc)

    @staticmethod
    def backward(ctx, dy):
        dx, dwc = _Conv1x1Fn.backward(ctx, dy)
        dw = dwc.new_zeros(dwc.shape[0], dwc.shape[1], 3, 3)
        dw[:, :, 1, 1] = dwc[:, :, 0, 0]
        return dx, dw


class DilatedConv3x3(nn.Conv2d):
    """Atrous 3x3 conv (stride 1, padding = dilation >= 2, no bias) routed to
    the in-tree MFMA kernels.

    A subclass of nn.Conv2d so that parameter names, shapes, the default
    initialisation and the RNG draw order are exactly those of the
    ``nn.Conv2d(cin, cout, 3, padding=d, dilation=d, bias=False)`` it stands
    in for. Backend select via TFOS_ATROUS: 'auto' (default: each of
    forward, dgrad and the dead-tap collapse goes in-tree only where it was
    measured no slower than the library), 'mfma' (in-tree, collapse
    included), 'miopen' (library conv). When the dilation reaches the image
    size only the centre tap is live and the conv runs as a 1x1 GEMM.
    """

    def __init__(self, in_channels, out_channels, dilation=2, device=None,
                 dtype=None):
        if int(dilation) < 2:
            raise ValueError("DilatedConv3x3 needs dilation >= 2 "
                             "(use Conv3x3 for an undilated conv)")
        super().__init__(in_channels, out_channels, 3, stride=1,
                         padding=int(dilation), dilation=int(dilation),
                         bias=False, device=device, dtype=dtype)
        self._eligible = in_channels % 32 == 0 and out_channels % 32 == 0 \
            and out_channels >= 64

    def forward(self, x):
        if x.is_cuda and self._eligible and x.dtype == torch.bfloat16 \
                and x.dim() == 4:
            fd = self.dilation[0]
            route = _atrous_route(x.shape[0], x.shape[2], x.shape[3],
                                  self.in_channels, self.out_channels, fd)
            if route is not None and get_ext(required=True) is not None:
                x = x.contiguous(memory_format=torch.channels_last)
                collapse, fwd_in_tree, dgrad_in_tree = route
                if collapse:
                    return _AtrousCollapsedFn.apply(x, self.weight)
                return _AtrousConv3x3Fn.apply(x, self.weight, fd,
                                              fwd_in_tree, dgrad_in_tree)
        return super().forward(x)

    def __prepare_scriptable__(self):
        # the scripter must not compile the routed forward: hand it a plain
        # conv that shares the weight and carries dilation and padding
        _SCRIPT_CLONE_KEEPALIVE.append(self)
        new = nn.Conv2d(self.in_channels, self.out_channels, 3, stride=1,
                        padding=self.padding, dilation=self.dilation,
                        bias=False)
        new.weight = self.weight
        new.train(self.training)
        return new


# ---------------------------------------------------------------------------
# Depthwise 3x3 convolution (csrc/dwconv3x3.hip)
# ---------------------------------------------------------------------------

_DW_DIRECTIONS = ("fwd", "dgrad", "wrw")


def _dw_auto(direction, N, C, H, W, stride):
    """TFOS_DW=auto policy: is ``direction`` ('fwd', 'dgrad' or 'wrw') of a
    depthwise 3x3 conv over an N x C x H x W input routed to the in-tree
    kernels?

    Follows the isolated measurement of the 17 depthwise layers of
    unet_mobilenet at b64 and b1024 @128^2 (tools/dw_bench.py,
    docs/performance.md "Depthwise convolutions"), where a (shape,
    direction) goes in-tree only if its median was no slower than the
    library's in that run. _dw_table() is that table.

    A shape that was not measured takes the decision of the measured shape
    with the same stride whose input element count N*C*H*W is nearest (in
    ratio), not the library: these are streaming kernels, and how they
    stand against the library follows the tensor size. A stride that was
    never measured (there is none among {1, 2}) stays on the library."""
    rows = [r for r in _dw_table() if r[4] == stride]
    if not rows:
        return False
    want = float(max(1, N * C * H * W))

    def dist(r):
        have = float(r[0] * r[1] * r[2] * r[3])
        return max(have / want, want / have)

    exact = [r for r in rows if r[:4] == (N, C, H, W)]
    row = exact[0] if exact else min(rows, key=dist)
    return row[5 + _DW_DIRECTIONS.index(direction)]


def _dw_table():
    """(N, C, H, W, stride, fwd, dgrad, wrw) per measured layer: True where
    tools/dw_bench.py measured the in-tree kernel no slower than the library
    on the MI355X (docs/performance.md "Depthwise convolutions"; the run is
    profiles/unet_dw_bench.json, whose "auto" column this repeats)."""
    T = True   # no pair lost: 2.4x to 18x (fwd, dgrad), 8x and up (wrw)
    return (
        (64, 32, 64, 64, 1, T, T, T),
        (64, 96, 64, 64, 2, T, T, T),
        (64, 144, 32, 32, 1, T, T, T),
        (64, 144, 32, 32, 2, T, T, T),
        (64, 192, 16, 16, 1, T, T, T),
        (64, 192, 16, 16, 2, T, T, T),
        (64, 384, 8, 8, 1, T, T, T),
        (64, 576, 8, 8, 1, T, T, T),
        (64, 576, 8, 8, 2, T, T, T),
        (64, 960, 4, 4, 1, T, T, T),
        (1024, 32, 64, 64, 1, T, T, T),
        (1024, 96, 64, 64, 2, T, T, T),
        (1024, 144, 32, 32, 1, T, T, T),
        (1024, 144, 32, 32, 2, T, T, T),
        (1024, 192, 16, 16, 1, T, T, T),
        (1024, 192, 16, 16, 2, T, T, T),
        (1024, 384, 8, 8, 1, T, T, T),
        (1024, 576, 8, 8, 1, T, T, T),
        (1024, 576, 8, 8, 2, T, T, T),
        (1024, 960, 4, 4, 1, T, T, T),
    )


def _dw_route(N, C, H, W, stride):
    """(fwd_in_tree, dgrad_in_tree, wrw_in_tree) for TFOS_DW, or None for
    the plain library conv."""
    mode = os.environ.get("TFOS_DW", "auto")
    if mode == "miopen":
        return None
    if mode == "hip":
        return True, True, True
    if mode != "auto":
        raise ValueError("TFOS_DW must be auto, hip or miopen, got "
                         + repr(mode))
    route = tuple(_dw_auto(d, N, C, H, W, stride) for d in _DW_DIRECTIONS)
    return route if any(route) else None


class _DepthwiseFn(torch.autograd.Function):
    """Depthwise 3x3 conv (padding 1, stride 1 or 2) on channels_last bf16
    or fp32 with the module's fp32 weight. Each of forward, dgrad and wrw
    runs in-tree or through the library as its flag says; the library sees
    the weight cast to the activation dtype, the value the kernels round to
    on load."""

    @staticmethod
    def forward(ctx, x, weight, stride, fwd_in_tree, dgrad_in_tree,
                wrw_in_tree):
        if fwd_in_tree:
            y = get_ext(required=True).dwconv3x3_fwd(x, weight, stride)
        else:
            y = F.conv2d(x, weight.to(x.dtype), None, stride, 1, 1,
                         x.shape[1])
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.in_tree = (dgrad_in_tree, wrw_in_tree)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        stride = ctx.stride
        dgrad_in_tree, wrw_in_tree = ctx.in_tree
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # an expanded (stride-0) gradient, as from y.sum().backward(),
        # becomes a real channels_last tensor here
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if need_dx and dgrad_in_tree:
            dx = get_ext(required=True).dwconv3x3_dgrad(
                dy, weight, stride, x.shape[2], x.shape[3])
        if need_dw and wrw_in_tree:
            dw = get_ext(required=True).dwconv3x3_wrw(dy, x, stride)
        lib_dx = need_dx and dx is None
        lib_dw = need_dw and dw is None
        if lib_dx or lib_dw:
            gx, gw, _ = torch.ops.aten.convolution_backward(
                dy, x, weight.to(x.dtype), None, [stride, stride], [1, 1],
                [1, 1], False, [0, 0], x.shape[1], [lib_dx, lib_dw, False])
            if lib_dx:
                dx = gx
            if lib_dw:
                dw = gw.to(weight.dtype)
        return dx, dw, None, None, None, None


class DepthwiseConv3x3(nn.Conv2d):
    """Depthwise 3x3 conv (groups == channels, padding 1, stride 1 or 2, no
    bias) routed to the in-tree streaming kernels.

    A subclass of nn.Conv2d so that parameter name, shape, the default
    initialisation and the RNG draw order are exactly those of the
    ``nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)`` it stands in
    for. Backend select via TFOS_DW: 'auto' (default: each of forward, dgrad
    and wrw goes in-tree only where it was measured no slower than the
    library, see _dw_auto), 'hip' (all three in-tree), 'miopen' (library
    conv). CPU tensors, dtypes other than bf16/fp32 and channel counts that
    are no multiple of the 16-byte vector (8 for bf16, 4 for fp32) stay on
    the library path.
    """

    def __init__(self, channels, stride=1, device=None, dtype=None):
        if int(stride) not in (1, 2):
            raise ValueError("DepthwiseConv3x3 needs stride 1 or 2, got "
                             + repr(stride))
        super().__init__(channels, channels, 3, stride=int(stride), padding=1,
                         groups=channels, bias=False, device=device,
                         dtype=dtype)

    def forward(self, x):
        if x.is_cuda and x.dim() == 4 and self.weight.dtype == torch.float32:
            # under autocast the library conv would run in the autocast
            # dtype whatever x is; so does this path
            dt = torch.get_autocast_dtype("cuda") \
                if torch.is_autocast_enabled("cuda") else x.dtype
            C = self.in_channels
            vec = {torch.bfloat16: 8, torch.float32: 4}.get(dt)
            if vec is not None and C % vec == 0 and x.numel() > 0:
                route = _dw_route(x.shape[0], C, x.shape[2], x.shape[3],
                                  self.stride[0])
                if route is not None and get_ext(required=True) is not None:
                    x = x.to(dt).contiguous(memory_format=torch.channels_last)
                    return _DepthwiseFn.apply(x, self.weight, self.stride[0],
                                              *route)
        return super().forward(x)

    def __prepare_scriptable__(self):
        # the scripter must not compile the routed forward: hand it a plain
        # grouped conv that shares the weight
        _SCRIPT_CLONE_KEEPALIVE.append(self)
        new = nn.Conv2d(self.in_channels, self.out_channels, 3,
                        stride=self.stride, padding=1, groups=self.groups,
                        bias=False)
        new.weight = self.weight
        new.train(self.training)
        return new


def _parity_launch(x, class_weight, out, k, pp, accum):
    """One conv_par launch per non-empty output parity class, each with only
    its valid taps; class_weight(ph, pw, rl, sl) is [OC, nr, ns, KC]."""
    ext = get_ext(required=True)
    for (ph, pw), (rl, sl) in _class_taps(k, pp).items():
        if not rl or not sl or ph >= out.shape[2] or pw >= out.shape[3]:
            continue
        wk = class_weight(ph, pw, rl, sl)
        ext.conv_par(x, wk.reshape(wk.shape[0], -1), out,
                     [r for r in rl for _ in sl], [s for _ in rl for s in sl],
                     pp, accum)
    return out


def _conv_parity_packed(x, packs, prefix, out, k, pp, accum=False):
    """_conv_parity with per-class weights already laid out: packs[
    '<prefix>_<ph><pw>'] shaped [OC, nr, ns, KC] (PackPlan views or
    EagerPacks)."""
    return _parity_launch(
        x, lambda ph, pw, rl, sl: packs["{}_{}{}".format(prefix, ph, pw)],
        out, k, pp, accum)


def _conv_parity(x, wperm, out, k, pp, accum=False):
    """Parity-decomposed conv over a 2x-dilated input: four class launches,
    each with only its valid taps (vs the plain D=2 kernel whose taps miss
    the stored rows 3/4 of the time — 4x wasted MFMA work).

    x: stored (undilated) input [N,KC,h,w] cl bf16; wperm: [OC, k, k, KC]
    direct-conv weight (already flipped/swapped for the backward-data or
    transposed-conv use); out: [N, OC, OH, OW] cl bf16 (every pixel of every
    non-empty class gets written; for k==1 zero-fill `out` first —
    odd-parity classes have no taps)."""
    return _parity_launch(
        x, lambda ph, pw, rl, sl: parity_class(wperm, rl, sl),
        out, k, pp, accum)


# ---------------------------------------------------------------------------
# Transposed convolution (U-Net/DeepLab decoders) as a dilated-input conv
# ---------------------------------------------------------------------------

class _ConvT2dFn(torch.autograd.Function):
    """ConvTranspose2d (stride 2) == conv over the zero-dilated input:
    y = conv(x_dil(D=2), W^swap-flip, S=1, P'=k-1-P). Backward-data is the
    plain stride-2 conv of dy with the unswapped weight — both directions run
    on the same implicit-GEMM MFMA kernel (reference workload: pix2pix
    upsample k4 s2 + Conv2DTranspose k3 s2, segmentation_spark.py:85-97)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, output_padding):
        _, Cout, KH, KW = weight.shape
        if x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        # W'[cout][r][s][cin] = W[cin][cout][KH-1-r][KW-1-s]
        wperm = flipped(weight)
        H, W = x.shape[2], x.shape[3]
        OH = (H - 1) * stride - 2 * padding + KH + output_padding
        OW = (W - 1) * stride - 2 * padding + KW + output_padding
        y = _cl_alloc((x.shape[0], Cout, OH, OW), x.device)
        if KH % 2 or output_padding:  # some classes empty -> zero base
            y.zero_()
        _conv_parity(x, wperm, y, KH, KH - 1 - padding)
        ctx.save_for_backward(x, weight)
        ctx.params = (stride, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        x, weight = ctx.saved_tensors
        S, P = ctx.params
        Cin, _, KH, KW = weight.shape
        dy = _cl_bf16(dy)
        # dx = plain stride-S conv of dy with W (no flip/swap)
        dx = ext.conv_mfma(dy, im2col(weight), Cin, KH, KW, S, P, 1,
                           x.shape[2], x.shape[3])
        dw = _weight_grad(dy, x, weight, KH, S, P, transposed=True)
        return dx, dw, None, None, None


class ConvTranspose2dMFMA(nn.Module):
    """Transposed conv routed to the implicit-GEMM MFMA kernel on GPU.

    Weight kept in nn.ConvTranspose2d's [Cin, Cout, K, K] layout for
    state_dict parity; bias unsupported (decoders here use BN right after).
    """

    def __init__(self, cin, cout, kernel_size=4, stride=2, padding=1,
                 output_padding=0):
        super().__init__()
        self.stride, self.padding = stride, padding
        self.output_padding = output_padding
        self.weight = nn.Parameter(torch.empty(cin, cout, kernel_size,
                                               kernel_size))
        nn.init.kaiming_normal_(self.weight, mode="fan_in", nonlinearity="relu")
        # fwd K = taps*Cin, dgrad K = taps*Cout — both must be 32-multiples
        self._eligible = cin % 32 == 0 and cout % 32 == 0 and stride == 2

    def forward(self, x):
        # tiny decoders (e.g. 4x4 spatial at the U-Net bottom) under-fill the
        # 256-row implicit-GEMM tiles; those stay on the library conv
        big = x.shape[0] * x.shape[2] * x.shape[3] * 4 >= 32768
        if x.is_cuda and self._eligible and big \
                and x.dtype == torch.bfloat16 \
                and os.environ.get("TFOS_CONVT", "mfma") == "mfma" \
                and get_ext(required=True) is not None:
            x = x.contiguous(memory_format=torch.channels_last)
            return _ConvT2dFn.apply(x, self.weight, self.stride, self.padding,
                                    self.output_padding)
        return F.conv_transpose2d(x, self.weight.to(x.dtype),
                                  stride=self.stride, padding=self.padding,
                                  output_padding=self.output_padding)

    def extra_repr(self):
        return "{}->{} k{} s{} p{} (implicit-GEMM MFMA)".format(
            self.weight.shape[0], self.weight.shape[1], self.weight.shape[2],
            self.stride, self.padding)


# ---------------------------------------------------------------------------
# MFMA GEMM (bf16 inputs, fp32 accumulate) for Dense layers / serving
# ---------------------------------------------------------------------------

def gemm_bf16(a, b):
    """C[m,n] = A[m,k] @ B[k,n] with bf16 inputs, fp32 accumulation.

    GPU path: hand-written MFMA (16x16x32 bf16) LDS-tiled kernel for gfx950.
    CPU path: torch.matmul in fp32.
    """
    if a.is_cuda:
        ext = get_ext(required=True)
        if ext is not None:
            return ext.gemm_bf16(a.contiguous(), b.contiguous())
    return (a.float() @ b.float())


class _GemmBTFn(torch.autograd.Function):
    """Autograd-composable C[M,N] = A[M,K] @ B[N,K]^T on the MFMA kernel.

    dA re-runs the same kernel (dA = dC @ B, K-contiguous after a small
    transpose of B); dB — a contraction over the M dim — uses the library
    GEMM per the kernel-usage policy."""

    @staticmethod
    def forward(ctx, a, b):
        ext = get_ext(required=True)
        a = a.to(torch.bfloat16).contiguous()
        b = b.to(torch.bfloat16).contiguous()
        ctx.save_for_backward(a, b)
        return ext.gemm_bt(a, b, True)

    @staticmethod
    def backward(ctx, dc):
        ext = get_ext(required=True)
        a, b = ctx.saved_tensors
        dc = dc.to(torch.bfloat16).contiguous()
        da = ext.gemm_bt(dc, b.t().contiguous(), True)
        db = (dc.float().t() @ a.float()).to(b.dtype)
        return da, db


class DenseMFMA(nn.Module):
    """Dense/Linear layer on the MFMA GEMM (survey §2.3 GEMM/Dense row:
    reference ``Dense(64, relu)``/``Dense(10)``, ``mnist_spark.py:17-19``).
    Weight/bias layout matches nn.Linear for state_dict parity."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.zeros(out_features)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and self.weight.shape[1] % 32 == 0 \
                and get_ext(required=True) is not None:
            y = _GemmBTFn.apply(x, self.weight)
            if self.bias is not None:
                y = y + self.bias.to(y.dtype)
            return y
        return F.linear(x, self.weight.to(x.dtype),
                        None if self.bias is None else self.bias.to(x.dtype))

    def __prepare_scriptable__(self):
        # TorchScript export swaps in the equivalent nn.Linear (the custom
        # kernel dispatch isn't scriptable; serving runs the library op)
        m = nn.Linear(self.weight.shape[1], self.weight.shape[0],
                      bias=self.bias is not None)
        m.weight = self.weight
        if self.bias is not None:
            m.bias = self.bias
        m.train(self.training)
        return m


class Conv2dIm2colMFMA(nn.Module):
    """Small-Cin conv (e.g. MNIST's Conv2D(1->32, k3)) via im2col into the
    MFMA GEMM, K zero-padded to a 32-multiple. The unfold/pad are tiny at
    MNIST scale; the matmul — the hot part — runs on the in-tree kernel.
    Weight/bias layout matches nn.Conv2d."""

    def __init__(self, cin, cout, kernel_size, bias=True):
        super().__init__()
        self.k = kernel_size
        self.weight = nn.Parameter(torch.empty(cout, cin, kernel_size,
                                               kernel_size))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and get_ext(required=True) is not None:
            N, Cin, H, W = x.shape
            Cout = self.weight.shape[0]
            OH, OW = H - self.k + 1, W - self.k + 1
            K = Cin * self.k * self.k
            Kpad = (K + 31) // 32 * 32
            cols = F.unfold(x, self.k)                    # [N, K, L]
            a = cols.transpose(1, 2).reshape(-1, K)       # [N*L, K]
            a = F.pad(a, (0, Kpad - K))
            w2 = F.pad(self.weight.view(Cout, K), (0, Kpad - K))
            y2 = _GemmBTFn.apply(a, w2)                   # [N*L, Cout]
            if self.bias is not None:
                y2 = y2 + self.bias.to(y2.dtype)
            return y2.view(N, OH * OW, Cout).transpose(1, 2) \
                .reshape(N, Cout, OH, OW)
        b = None if self.bias is None else self.bias.to(x.dtype)
        return F.conv2d(x, self.weight.to(x.dtype), b)

    def __prepare_scriptable__(self):
        m = nn.Conv2d(self.weight.shape[1], self.weight.shape[0], self.k,
                      bias=self.bias is not None)
        m.weight = self.weight
        if self.bias is not None:
            m.bias = self.bias
        m.train(self.training)
        return m


class BucketAdam:
    """Adam(W) over DDPEngine flat buckets — one fused kernel per bucket on
    GPU (fp32 m/v state), torch ops on CPU. ``decoupled=True`` = AdamW."""

    def __init__(self, engine, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, decoupled=False):
        self.engine = engine
        self.lr = lr
        self.b1, self.b2 = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.decoupled = decoupled
        self.step_count = 0
        self._m = [torch.zeros_like(b.buffer) for b in engine._buckets]
        self._v = [torch.zeros_like(b.buffer) for b in engine._buckets]

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        for bucket, m, v in zip(self.engine._buckets, self._m, self._v):
            pf = bucket.param_flat
            g = bucket.buffer
            assert pf is not None, "BucketAdam requires flatten_params=True"
            ext = get_ext(required=True) if g.is_cuda else None
            if ext is not None:
                ext.adam_step(pf, g, m, v, self.lr, self.b1, self.b2, self.eps,
                              self.weight_decay, self.step_count, self.decoupled)
                continue
            grad = g if self.decoupled or not self.weight_decay \
                else g.add(pf, alpha=self.weight_decay)
            m.mul_(self.b1).add_(grad, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(grad, grad, value=1 - self.b2)
            bc1 = 1 - self.b1 ** self.step_count
            bc2 = 1 - self.b2 ** self.step_count
            upd = (m / bc1) / ((v / bc2).sqrt() + self.eps)
            if self.decoupled and self.weight_decay:
                upd = upd + self.weight_decay * pf
            pf.add_(upd, alpha=-self.lr)

    def zero_grad(self):
        self.engine.zero_grad()


# ---------------------------------------------------------------------------
# Fully-fused ResNet Bottleneck (manual backward, zero autograd glue)
# ---------------------------------------------------------------------------

def _bn_epi_mode():
    """TFOS_BN_EPI: where the fused bottleneck's BatchNorms take their batch
    statistics from. 'off': always the separate pass over the conv output
    (stats_nhwc_fast); 'force': the conv kernel's statistics epilogue wherever
    the dispatched kernel has one; 'auto' (default): per shape, _bn_epi_auto.
    """
    mode = os.environ.get("TFOS_BN_EPI", "auto")
    if mode not in ("auto", "off", "force"):
        raise ValueError("TFOS_BN_EPI must be auto, off or force, got "
                         + repr(mode))
    return mode


# smallest conv output, in bytes, that TFOS_BN_EPI=auto routes: the smallest
# tensor of the measurement below (1024 x 512 x 7 x 7 bf16, 51 MB)
_BN_EPI_MIN_BYTES = 1024 * 512 * 7 * 7 * 2


def _bn_epi_auto(kind, M, K, cout):
    """TFOS_BN_EPI=auto policy for one (conv, BN) pair: ``kind`` 'gemm' (a
    1x1 stride-1 conv through gemm_bt) or 'conv' (conv_mfma), M output
    pixels, K = taps * Cin, cout output channels.

    Follows the per-pair measurement at the ResNet-50 batch-1024 shapes
    (tools/bn_bench.py --epilogue; docs/performance.md "BN statistics from
    the conv epilogues"): conv + statistics pass + merge against conv with
    the epilogue + tile merge, medians of 9 alternating rounds, a pair being
    ahead when it wins by more than either side's max - min over the rounds.

      gemm_bt, 128^2 and 256x64 tiles (9 shapes)     10-28 % ahead  -> epilogue
      conv_mfma, 256x256 tile (Cout >= 192)          4-13 % ahead   -> epilogue
      conv_mfma, 256x128 tile (Cout < 192): 64->64 @56 loses 4.6 %, the two
        128->128 shapes win by less than the spread                 -> pass

    The 256x128 conv kernel has 4 waves stacked in M per column group and
    spends in its epilogue what the pass over a 64- or 128-channel tensor
    costs; it stays on the separate pass. Shapes that gemm_bt sends to its
    256^2 kernel have no epilogue and come back without partials whatever
    this says. Nothing smaller than the smallest tensor measured is routed:
    at a few MB the pass runs from cache and launch count decides."""
    if M * cout * 2 < _BN_EPI_MIN_BYTES:
        return False
    return kind == "gemm" or cout >= 192


def _bn_epi_route(mode, kind, M, K, cout, ext=None):
    """Does the (conv, BN) pair take the statistics-epilogue route? Under
    'auto' and 'force' alike only where the BN that follows is on the NHWC
    fast path (fewer than 2^31 elements, C % 8 == 0, C | 2048: what
    ``ext.bn_fast_blocks`` answers): bn_fwd_train_pre takes nothing else, and
    the generic kernels behind bn_fwd_train keep every other width working.
    Without ``ext`` only the mode and the shape policy are consulted."""
    if mode == "off":
        return False
    if ext is not None and ext.bn_fast_blocks(M * cout, cout, True, True) <= 0:
        return False
    return mode == "force" or _bn_epi_auto(kind, M, K, cout)


class _BottleneckFn(torch.autograd.Function):
    """One autograd node for the whole bottleneck block.

    Eager autograd accumulates the residual-join gradients (the block input
    feeds both conv1 and the identity/downsample path) with whole-tensor adds
    — 8.4 ms/step of CUDAFunctor_add at ResNet-50 b1024 (profiles/README
    r01). The manual backward instead makes the conv1 (and downsample)
    backward-data kernels accumulate straight into the residual gradient
    buffer (gemm_bt_acc / conv_mfma_acc epilogues), so no separate add runs.

    Tensors bf16 channels_last; BN stats/params fp32. Training mode only;
    saved set (t*, a*, masks, stats) matches what the unfused composition
    saves, so peak memory is unchanged.

    With a downsample branch the block ends in y = relu(bn3(t3) + bnd(td)).
    The dual BN entries (bn_dual_fwd_train / bn_dual_bwd) compute that join
    and its backward with one read of each stream per pass: the normalized
    shortcut is never written, read back or saved, and the gated gradient is
    not written out and re-read by the second BN. The shortcut is then not
    rounded to bf16 before the add, so y can differ from the two-call
    composition by a bf16 ulp. ``TFOS_BN_DUAL=off`` or an ineligible pair
    (bn_dual_eligible) keeps the two-call composition.
    """

    @staticmethod
    def forward(ctx, x, w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2,
                w3, g3, b3, rm3, rv3, wd, gd, bd, rmd, rvd,
                stride, momentum, eps, packs=None):
        ext = get_ext(required=True)
        N, Cin, H, W = x.shape
        C1, C2, C3 = w1.shape[0], w2.shape[0], w3.shape[0]
        # packed bf16 weights, by PackPlan key: the plan's views when supplied
        # (one kernel for the whole model per optimizer step), else each
        # layout computed eagerly where it is first read
        ctx.packs = packs
        if packs is None:
            packs = EagerPacks(w1, w2, w3, wd, stride)
        # TFOS_BN_EPI: a conv routed to its statistics-epilogue variant hands
        # the BN that follows the tile partials of its output (part, rows), and
        # that BN merges them instead of reading the tensor back; part is None
        # for a conv left on the plain kernel or dispatched to a kernel
        # without the epilogue, and its BN then runs the separate pass.
        epi = _bn_epi_mode()

        def gemm(a2d, wb):
            if _bn_epi_route(epi, "gemm", a2d.shape[0], wb.shape[1],
                             wb.shape[0], ext):
                return ext.gemm_bt_stats(a2d, wb)
            return ext.gemm_bt(a2d, wb, True), None, 0

        def conv(a, wk, cout, k, s, p, m_out):
            if _bn_epi_route(epi, "conv", m_out, k * k * a.shape[1], cout,
                             ext):
                return ext.conv_mfma_stats(a, wk, cout, k, k, s, p, 1, -1, -1)
            return ext.conv_mfma(a, wk, cout, k, k, s, p, 1, -1, -1), None, 0

        def bn(t, res, part, rows, g, b, rm, rv, relu):
            if part is not None:
                return ext.bn_fwd_train_pre(t, res, part, rows, g, b, rm, rv,
                                            momentum, eps, relu)
            return ext.bn_fwd_train(t, res, g, b, rm, rv, momentum, eps, relu)

        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        t1, p1, n1 = gemm(as2d(x), packs["w1b"].reshape(C1, Cin))
        t1 = as4d(t1, N, H, W)
        a1, m1, r1, k1 = bn(t1, None, p1, n1, g1, b1, rm1, rv1, True)
        t2, p2, n2 = conv(a1, packs["w9"].reshape(C2, 9 * C1), C2, 3, stride,
                          1, N * OH * OW)
        a2, m2, r2, k2 = bn(t2, None, p2, n2, g2, b2, rm2, rv2, True)
        assert (OH, OW) == (t2.shape[2], t2.shape[3])
        t3, p3, n3 = gemm(as2d(a2), packs["w3b"].reshape(C3, C2))
        t3 = as4d(t3, N, OH, OW)

        if wd is not None:
            wdb = packs["wdb"].reshape(C3, Cin)
            if stride == 1:
                td, pd, nd = gemm(as2d(x), wdb)
                td = as4d(td, N, H, W)
            else:
                td, pd, nd = conv(x, wdb, C3, 1, stride, 0, N * OH * OW)
            dual = os.environ.get("TFOS_BN_DUAL", "on") != "off" \
                and ext.bn_dual_eligible(t3, td)
            if dual:
                # y = relu(bn3(t3) + bnd(td)) in one pass: the normalized
                # shortcut is neither written nor saved
                if p3 is not None or pd is not None:
                    y, m3, r3, md, rd, k3 = ext.bn_dual_fwd_train_pre(
                        t3, td, p3, n3, pd, nd, g3, b3, rm3, rv3, gd, bd,
                        rmd, rvd, momentum, eps)
                else:
                    y, m3, r3, md, rd, k3 = ext.bn_dual_fwd_train(
                        t3, td, g3, b3, rm3, rv3, gd, bd, rmd, rvd, momentum,
                        eps)
                opt = [td, md, rd]
            else:
                idn, md, rd, _kd = bn(td, None, pd, nd, gd, bd, rmd, rvd,
                                      False)
                opt = [td, idn, md, rd]
        else:
            dual = False
            idn = x
            opt = []
        if not dual:
            y, m3, r3, k3 = bn(t3, idn, p3, n3, g3, b3, rm3, rv3, True)

        ctx.save_for_backward(x, w1, g1, t1, a1, m1, r1, k1,
                              w2, g2, t2, a2, m2, r2, k2,
                              w3, g3, t3, m3, r3, k3, y, wd, gd, *opt)
        ctx.meta = (stride, wd is not None, dual)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        (x, w1, g1, t1, a1, m1, r1, k1, w2, g2, t2, a2, m2, r2, k2,
         w3, g3, t3, m3, r3, k3, y, wd, gd, *opt) = ctx.saved_tensors
        stride, has_down, dual = ctx.meta
        packs = ctx.packs
        if packs is None:       # from the saved weights, as forward's was
            packs = EagerPacks(w1, w2, w3, wd, stride)
        N, Cin, H, W = x.shape
        C1, C2, C3 = w1.shape[0], w2.shape[0], w3.shape[0]
        OH, OW = t2.shape[2], t2.shape[3]
        dy = _cl_bf16(dy)

        def cl(t):
            return t.contiguous(memory_format=torch.channels_last)

        def wrw(dyt, xt, w, k, s_):
            # the fused block has never taken the round-1 conv_wrw kernel:
            # under TFOS_WRW=mfma its weight gradients stay on the library
            return _weight_grad(dyt, xt, w, k, s_, k // 2, round1=False)

        # block tail: bn3(+res+relu) backward -> dt3 plus the gated residual
        # gradient dres (doubles as the dx accumulation buffer below)
        if dual:
            # both BNs of the join from one read of dy: dres never exists
            td, md, rd = opt
            dt3, dtd, dg3, dgd, db3, dbd = ext.bn_dual_bwd(
                t3, td, dy, k3, g3, m3, r3, gd, md, rd)
        else:
            dt3, dg3, db3, dres = ext.bn_bwd(t3, dy, y, k3, g3, m3, r3,
                                             True, True)
        dt3 = cl(dt3)

        # conv3 (1x1): dgrad + wrw
        da2 = cl(as4d(ext.gemm_bt(as2d(dt3), packs["w3bT"].reshape(C2, C3),
                                  True), N, OH, OW))
        dw3 = wrw(dt3, a2, w3, 1, 1)

        # bn2+relu backward
        dt2, dg2, db2 = ext.bn_bwd(t2, da2, a2, k2, g2, m2, r2, True, False)
        dt2 = cl(dt2)

        # conv2 (3x3, stride s): dgrad (parity-decomposed for s2) + wrw
        if stride == 2:
            da1 = _cl_alloc((N, C1, H, W), x.device)
            _conv_parity_packed(dt2, packs, "w9p", da1, 3, 1)
        else:
            da1 = ext.conv_mfma(dt2, packs["w9p"].reshape(C1, 9 * C2), C1,
                                3, 3, 1, 1, 1, H, W)
        dw2 = wrw(dt2, a1, w2, 3, stride)

        # bn1+relu backward
        dt1, dg1, db1 = ext.bn_bwd(t1, da1, a1, k1, g1, m1, r1, True, False)
        dt1 = cl(dt1)

        # conv1 (1x1) wrw
        dw1 = wrw(dt1, x, w1, 1, 1)

        w1bT = packs["w1bT"].reshape(Cin, C1)
        if has_down:
            if not dual:
                td, idn, md, rd = opt
                # downsample path: bnd backward (no relu) then conv dgrad
                dtd, dgd, dbd = ext.bn_bwd(td, dres, idn,
                                           torch.empty(0, dtype=torch.uint8,
                                                       device=td.device),
                                           gd, md, rd, False, False)
            dtd = cl(dtd)
            dwd = wrw(dtd, x, wd, 1, stride)
            # dx = conv1_dgrad, then downsample dgrad ACCUMULATES into it
            dx = cl(as4d(ext.gemm_bt(as2d(dt1), w1bT, True), N, H, W))
            wdbT = packs["wdbT"].reshape(Cin, C3)
            if stride == 1:
                ext.gemm_bt_acc(as2d(dtd), wdbT, as2d(dx))
            else:
                # even-even parity class only; odd pixels' contribution is 0
                ext.conv_par(dtd, wdbT, dx, [0], [0], 0, True)
        else:
            # dx = dres + conv1_dgrad — accumulate straight into dres
            dx = dres
            ext.gemm_bt_acc(as2d(dt1), w1bT, as2d(dx))
            dwd = dgd = dbd = None

        return (dx, dw1, dg1, db1, None, None, dw2, dg2, db2, None, None,
                dw3, dg3, db3, None, None, dwd, dgd, dbd, None, None,
                None, None, None, None)


# ---------------------------------------------------------------------------
# ResNet stem: 7x7/s2/p3 conv on the implicit-GEMM kernel via an NHWC4 view
# ---------------------------------------------------------------------------

class _StemConvFn(torch.autograd.Function):
    """7x7/s2/p3 stem conv (Cin=3) on in-tree kernels.

    The input is packed once to a spatially pre-padded NHWC4 image
    ([N,4,H+6,W+6], channel 3 zero); each filter ROW becomes one uniform
    32-wide K-step (8 px x 4 ch, the 8th px's weight columns are zero), so the
    generic implicit-GEMM kernel runs it with zero guard loads at 1.52x the
    minimal FLOPs (vs 10.7x for a pad-to-32 im2col). The weight gradient runs
    on the same NHWC4 view through the wrw kernel. dgrad is not computed (the
    stem is the first layer; inputs don't carry grad)."""

    @staticmethod
    def forward(ctx, x, weight, w224=None):
        ext = get_ext(required=True)
        N, _, H, W = x.shape
        Cout = weight.shape[0]
        x4 = _cl_alloc((N, 4, H + 6, W + 6), x.device, zero=True)
        x4[:, :3, 3:H + 3, 3:W + 3] = x
        if w224 is None:
            w224 = stem_w224(weight)
        y = ext.conv_stem(x4, w224.reshape(Cout, 224).contiguous(), Cout)
        ctx.save_for_backward(x4, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = get_ext(required=True)
        x4, weight = ctx.saved_tensors
        dw224 = ext.conv_stem_wrw(_cl_bf16(dy), x4)  # [Cout, 224] fp32
        Cout = weight.shape[0]
        dw = dw224.view(Cout, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2)
        return None, dw.contiguous().to(weight.dtype), None


class StemConv7x7(nn.Module):
    """ResNet-50 stem conv (7x7, stride 2, pad 3, Cin=3) on the MFMA kernels.

    Library fallback on CPU / non-bf16 / when the input requires grad (the
    kernel path does not produce dx — it is the first layer)."""

    def __init__(self, cin=3, cout=64):
        super().__init__()
        assert cin == 3
        self.weight = nn.Parameter(torch.empty(cout, cin, 7, 7))
        nn.init.kaiming_normal_(self.weight, mode="fan_out",
                                nonlinearity="relu")

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 and not x.requires_grad \
                and os.environ.get("TFOS_STEM", "mfma") == "mfma" \
                and get_ext(required=True) is not None:
            x = x.contiguous(memory_format=torch.channels_last)
            packs = getattr(self, "_tfos_packs", None)
            return _StemConvFn.apply(x, self.weight,
                                     packs["w224"] if packs else None)
        return F.conv2d(x, self.weight.to(x.dtype), stride=2, padding=3)

    def extra_repr(self):
        return "3->{} 7x7 s2 (NHWC4 implicit-GEMM MFMA)".format(
            self.weight.shape[0])


# ---------------------------------------------------------------------------
# TorchScript export support: every fused/MFMA module (and the blocks built
# from them) swaps to an equivalent plain-op module at scripting time, so
# TFNode.export_saved_model produces a loadable TorchScript model for ANY
# in-repo architecture (TFModel.transform / serving / tfosr_infer CLI).
# ---------------------------------------------------------------------------

# torch.jit.script's __prepare_scriptable__ recursion memoizes modules by
# id(); once a replaced original is garbage-collected its id can be recycled
# by a freshly created clone, and the memo then resolves the NEW module to
# the OLD replacement (observed: a stem-conv clone landing where a BatchNorm
# belonged). Keeping every original alive until the export finishes makes id
# reuse impossible. export_saved_model drains this list.
_SCRIPT_CLONE_KEEPALIVE = []


def _bn_clone(src):
    _SCRIPT_CLONE_KEEPALIVE.append(src)
    bn = nn.BatchNorm2d(src.num_features, eps=src.eps, momentum=src.momentum)
    with torch.no_grad():
        bn.weight.copy_(src.weight)
        bn.bias.copy_(src.bias)
        bn.running_mean.copy_(src.running_mean)
        bn.running_var.copy_(src.running_var)
        bn.num_batches_tracked.copy_(src.num_batches_tracked)
    bn.train(src.training)
    return bn


def _conv_clone(m):
    """nn.Conv2d equivalent of Conv1x1 / Conv3x3 / StemConv7x7 (or passthrough
    for an already-plain conv)."""
    if isinstance(m, nn.Conv2d):
        return m
    _SCRIPT_CLONE_KEEPALIVE.append(m)
    k = m.weight.shape[2]
    stride = getattr(m, "stride", 1)
    if isinstance(m, StemConv7x7):
        stride, pad = 2, 3
    else:
        pad = 1 if k == 3 else 0
    new = nn.Conv2d(m.weight.shape[1], m.weight.shape[0], k, stride=stride,
                    padding=pad, bias=False)
    new.weight = m.weight
    new.train(m.training)
    return new


def _convT_clone(m):
    if isinstance(m, nn.ConvTranspose2d):
        return m
    _SCRIPT_CLONE_KEEPALIVE.append(m)
    new = nn.ConvTranspose2d(m.weight.shape[0], m.weight.shape[1],
                             m.weight.shape[2], stride=m.stride,
                             padding=m.padding,
                             output_padding=m.output_padding, bias=False)
    new.weight = m.weight
    new.train(m.training)
    return new


def _fusedbn_prepare(self):
    _SCRIPT_CLONE_KEEPALIVE.append(self)
    bn = _bn_clone(self)
    if self.RELU:
        out = nn.Sequential(bn, nn.ReLU(inplace=True))
        out.train(self.training)
        return out
    return bn


# FusedBNAddReLU takes (x, res) — its parents (the residual blocks) provide
# their own scriptable clones below, so only the one-arg variants get hooks.
def _maxpool_prepare(self):
    _SCRIPT_CLONE_KEEPALIVE.append(self)
    return nn.MaxPool2d(self.k, self.s, self.p)


FusedMaxPool2d.__prepare_scriptable__ = _maxpool_prepare
FusedBNReLU.__prepare_scriptable__ = _fusedbn_prepare
FusedBN.__prepare_scriptable__ = _fusedbn_prepare
Conv1x1.__prepare_scriptable__ = lambda self: _conv_clone(self)
Conv3x3.__prepare_scriptable__ = lambda self: _conv_clone(self)
StemConv7x7.__prepare_scriptable__ = lambda self: _conv_clone(self)
ConvTranspose2dMFMA.__prepare_scriptable__ = lambda self: _convT_clone(self)
