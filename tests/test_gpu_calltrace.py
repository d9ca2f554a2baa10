"""Call traces of the conv modules and the fused Bottleneck: which extension
entries a forward + backward reaches, in which order, with which arguments.

A recorder wraps every entry of the HIP extension and notes, per call, the
entry name, shape/stride/dtype of every tensor argument and every non-tensor
argument. The weight operand of ``gemm_bt*``, ``conv_mfma*``, ``conv_par`` and
``conv_stem`` is hashed as well (weights here are small multiples of 2^-10,
exact in bf16, so the hash does not depend on how a re-layout rounds).
Activations are not hashed: the BN reductions use LDS float atomics.

``golden/calltrace.json`` holds the traces this file recorded at the commit
before the weight layouts and the weight-gradient routing were gathered into
one definition each; ``PYTHONPATH=. python tests/test_gpu_calltrace.py
OUT.json`` on a GPU writes such a file. A trace that differs from it is a behaviour change:
a weight gradient routed to the library shows up as the absence of a
``conv_wrw*`` entry, a changed re-layout as another weight hash.
"""

import hashlib
import json
import os
import sys

import pytest
import torch

from test_gpu_bn import BF16, _ext, gpu, requires_gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "calltrace.json")
MODES = ("auto", "mfma2", "mfma", "miopen")
HASHED = ("gemm_bt", "conv_mfma", "conv_par", "conv_stem")
# routing switches other than TFOS_WRW: at their defaults
DEFAULTED = ("TFOS_BN_EPI", "TFOS_BN_DUAL", "TFOS_CONV1X1", "TFOS_CONV3X3",
             "TFOS_CONVT", "TFOS_STEM", "TFOS_FUSED_BLOCK", "TFOS_PACK_PLAN")


def _fill(p, salt):
    """Deterministic weights on a 2^-10 grid in (-0.125, 0.125)."""
    idx = torch.arange(p.numel(), dtype=torch.int64) + salt
    v = ((idx * 40503) % 251 - 125).to(torch.float32) / 1024
    with torch.no_grad():
        p.copy_(v.view(p.shape))


def _describe(a):
    if torch.is_tensor(a):
        return "{}{}/{}".format(str(a.dtype).replace("torch.", ""),
                                list(a.shape), list(a.stride()))
    if isinstance(a, (list, tuple)):
        return [_describe(v) for v in a]
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    return repr(a)


def _hash(t):
    raw = t.detach().contiguous().view(torch.int16).cpu().numpy().tobytes()
    return hashlib.sha1(raw).hexdigest()[:16]


def _record(mp, fn):
    """Run fn() with every extension entry wrapped; returns the trace."""
    ext = _ext()
    trace = []
    names = [n for n in dir(ext)
             if not n.startswith("_") and callable(getattr(ext, n))]
    orig = {n: getattr(ext, n) for n in names}

    def wrap(name):
        def f(*a, **kw):
            call = [name, [_describe(v) for v in a],
                    {k: _describe(v) for k, v in sorted(kw.items())}]
            if name.startswith(HASHED) and name != "conv_stem_wrw":
                call.append(_hash(a[1]))
            trace.append(call)
            return orig[name](*a, **kw)
        return f

    for n in names:
        mp.setattr(ext, n, wrap(n))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        for n in names:
            mp.setattr(ext, n, orig[n])
    return trace, out


def _conv(kind, **kw):
    def make():
        from tensorflowonspark_amd.ops import modules
        return getattr(modules, kind)(**kw)
    return make


def _block(cin, stride, down):
    def make():
        from tensorflowonspark_amd.models.resnet import Bottleneck, conv1x1
        from tensorflowonspark_amd.ops.modules import FusedBN
        ds = torch.nn.Sequential(conv1x1(cin, 256, stride), FusedBN(256)) \
            if down else None
        return Bottleneck(cin, 64, stride, ds)
    return make


# name: (module factory, input shape, TFOS_ATROUS, is a Bottleneck)
CASES = {
    "conv1x1_s1": (_conv("Conv1x1", cin=64, cout=96, stride=1),
                   (2, 64, 16, 16), None, False),
    "conv1x1_s2": (_conv("Conv1x1", cin=64, cout=96, stride=2),
                   (2, 64, 16, 16), None, False),
    "conv3x3_s1": (_conv("Conv3x3", cin=64, cout=96, stride=1),
                   (2, 64, 16, 16), None, False),
    "conv3x3_s2": (_conv("Conv3x3", cin=64, cout=96, stride=2),
                   (2, 64, 16, 16), None, False),
    "atrous_d2": (_conv("DilatedConv3x3", in_channels=64, out_channels=96,
                        dilation=2), (2, 64, 16, 16), "mfma", False),
    "atrous_d16": (_conv("DilatedConv3x3", in_channels=64, out_channels=96,
                         dilation=16), (2, 64, 16, 16), "mfma", False),
    "convt_k4": (_conv("ConvTranspose2dMFMA", cin=64, cout=96, kernel_size=4,
                       stride=2, padding=1), (2, 64, 64, 64), None, False),
    "convt_k3_op1": (_conv("ConvTranspose2dMFMA", cin=64, cout=96,
                           kernel_size=3, stride=2, padding=1,
                           output_padding=1), (2, 64, 64, 64), None, False),
    "stem": (_conv("StemConv7x7"), (2, 3, 32, 32), None, False),
    "block_s1_down": (_block(64, 1, True), (4, 64, 16, 16), None, True),
    "block_s2_down": (_block(64, 2, True), (4, 64, 16, 16), None, True),
    "block_s1_plain": (_block(256, 1, False), (4, 256, 16, 16), None, True),
}


def _trace(mp, case, mode, packed=False):
    """Forward + backward of one case under TFOS_WRW=mode; returns the trace
    after checking that outputs and gradients are finite and well-shaped."""
    make, shape, atrous, is_block = CASES[case]
    for k in DEFAULTED:
        mp.delenv(k, raising=False)
    mp.setenv("TFOS_WRW", mode)
    if atrous is None:
        mp.delenv("TFOS_ATROUS", raising=False)
    else:
        mp.setenv("TFOS_ATROUS", atrous)
    m = make()
    for i, p in enumerate(m.parameters()):
        if p.dim() == 4:
            _fill(p, 7 * i + 1)
    # parameters stay NCHW-contiguous, the storage order PackPlan gathers from
    m = m.cuda().train()
    if packed:
        from tensorflowonspark_amd.ops import packplan
        plan = packplan.build_resnet_plan(torch.nn.Sequential(m), "cuda")
        assert plan is not None and plan.run_if_stale()
        assert getattr(m, "_tfos_packs", None)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(*shape, device="cuda", generator=gen).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    x.requires_grad_(case != "stem")     # the stem kernel path has no dx

    def run():
        y = m(x)
        dy = torch.randn(y.shape, device="cuda", generator=gen).to(BF16) \
            .contiguous(memory_format=torch.channels_last)
        y.backward(dy)
        return y

    trace, y = _record(mp, run)
    assert y.dtype == BF16 and torch.isfinite(y).all()
    if case != "stem":
        assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype, n
        assert torch.isfinite(p.grad).all(), n
    return trace


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "call {}:\n  got  {}\n  want {}".format(i, g, w)
    return "{} calls, expected {}: {}".format(
        len(got), len(want), [c[0] for c in got])


@gpu
@requires_gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_call_trace(case, mode, golden, monkeypatch):
    want = golden["{}/{}".format(case, mode)]
    got = json.loads(json.dumps(_trace(monkeypatch, case, mode)))
    assert got == want, _first_difference(got, want)
    if CASES[case][3]:
        # PackPlan views attached: same entries, arguments and weight bits
        packed = json.loads(json.dumps(
            _trace(monkeypatch, case, mode, packed=True)))
        assert packed == got, _first_difference(packed, got)


if __name__ == "__main__":
    out, bad = {}, []
    with pytest.MonkeyPatch.context() as mp:
        for case in sorted(CASES):
            for mode in MODES:
                key = "{}/{}".format(case, mode)
                out[key] = _trace(mp, case, mode)
                if CASES[case][3]:
                    packed = _trace(mp, case, mode, packed=True)
                    if packed != out[key]:
                        bad.append(key + " packed: "
                                   + _first_difference(packed, out[key]))
                print(key, [c[0] for c in out[key]], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    sys.exit("\n".join(bad) if bad else 0)
