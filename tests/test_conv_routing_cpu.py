"""The weight-gradient routing table and the lazily computed eager weight
layouts of the fused Bottleneck (CPU only: neither needs a kernel)."""

import pytest
import torch
import torch.nn as nn

from tensorflowonspark_amd.models.resnet import Bottleneck, conv1x1
from tensorflowonspark_amd.ops import modules, packplan
from tensorflowonspark_amd.ops.modules import FusedBN

BF16 = torch.bfloat16

# backend per (stride, fd) in the order (1,1) (1,2) (2,1) (2,2):
# 2 = conv_wrw2, 1 = round-1 conv_wrw, L = library. Written out from the
# routing each conv Function carried before there was one router: conv_wrw2
# where channels % 8 == 0 and _use_wrw2 (mfma2: always; auto and unknown
# strings: 3x3 with both channel counts <= 64); conv_wrw only under mfma at
# stride 1, undilated, channels % 8 == 0; the library otherwise.
SD = ((1, 1), (1, 2), (2, 1), (2, 2))
NAMES = {"2": "wrw2", "1": "wrw", "L": "lib"}
AUTO = {(1, 64, 64): "LLLL", (1, 64, 256): "LLLL", (1, 128, 128): "LLLL",
        (1, 60, 64): "LLLL", (3, 64, 64): "2222", (3, 64, 256): "LLLL",
        (3, 128, 128): "LLLL", (3, 60, 64): "LLLL"}
EXPECT = {
    "auto": AUTO,
    "no-such-mode": AUTO,
    "mfma2": {(1, 64, 64): "2222", (1, 64, 256): "2222",
              (1, 128, 128): "2222", (1, 60, 64): "LLLL",
              (3, 64, 64): "2222", (3, 64, 256): "2222",
              (3, 128, 128): "2222", (3, 60, 64): "LLLL"},
    "mfma": {(1, 64, 64): "1LLL", (1, 64, 256): "1LLL",
             (1, 128, 128): "1LLL", (1, 60, 64): "LLLL",
             (3, 64, 64): "1LLL", (3, 64, 256): "1LLL",
             (3, 128, 128): "1LLL", (3, 60, 64): "LLLL"},
    "miopen": {(1, 64, 64): "LLLL", (1, 64, 256): "LLLL",
               (1, 128, 128): "LLLL", (1, 60, 64): "LLLL",
               (3, 64, 64): "LLLL", (3, 64, 256): "LLLL",
               (3, 128, 128): "LLLL", (3, 60, 64): "LLLL"},
}


@pytest.mark.parametrize("mode", sorted(EXPECT))
def test_wrw_backend_table(mode):
    for (k, cin, cout), row in EXPECT[mode].items():
        for (stride, fd), want in zip(SD, row):
            what = (mode, k, cin, cout, stride, fd)
            assert modules._wrw_backend(mode, k, cin, cout, stride, fd) \
                == NAMES[want], what
            # a transposed conv: always the library
            assert modules._wrw_backend(mode, k, cin, cout, stride, fd,
                                        transposed=True) == "lib", what
            # the fused Bottleneck never takes the round-1 kernel
            no_r1 = modules._wrw_backend(mode, k, cin, cout, stride, fd,
                                         round1=False)
            assert no_r1 == NAMES["L" if want == "1" else want], what


def test_use_wrw2_reads_the_environment(monkeypatch):
    monkeypatch.delenv("TFOS_WRW", raising=False)
    assert modules._use_wrw2(3, 64, 64) and not modules._use_wrw2(3, 64, 128)
    monkeypatch.setenv("TFOS_WRW", "mfma2")
    assert modules._use_wrw2(1, 256, 1024)
    for mode in ("mfma", "miopen"):
        monkeypatch.setenv("TFOS_WRW", mode)
        assert not modules._use_wrw2(3, 64, 64)
    monkeypatch.setenv("TFOS_WRW", "no-such-mode")      # treated as auto
    assert modules._use_wrw2(3, 64, 64) and not modules._use_wrw2(1, 64, 64)


EAGER = ("rows", "rows_t", "im2col", "flipped", "parity_class")


def _counted(monkeypatch):
    calls = dict.fromkeys(EAGER, 0)

    def wrap(name, fn):
        def f(*a):
            calls[name] += 1
            return fn(*a)
        return f

    for name in EAGER:
        monkeypatch.setattr(packplan, name, wrap(name, getattr(packplan, name)))
    return calls


@pytest.mark.parametrize("stride,down", [(1, False), (2, True)])
def test_eager_packs_are_lazy_and_match_the_plan_keys(stride, down,
                                                      monkeypatch):
    torch.manual_seed(4)
    ds = nn.Sequential(conv1x1(64, 256, stride), FusedBN(256)) if down \
        else None
    blk = Bottleneck(256 if not down else 64, 64, stride, ds)
    assert blk._block_fusable
    assert packplan.build_resnet_plan(nn.Sequential(blk), "cpu") is not None
    w1, w2, w3 = (torch.randn_like(c.weight)
                  for c in (blk.conv1, blk.conv2, blk.conv3))
    wd = torch.randn_like(ds[0].weight) if down else None
    cin = w1.shape[1]

    calls = _counted(monkeypatch)
    packs = packplan.EagerPacks(w1, w2, w3, wd, stride)
    assert set(packs) == set(blk._tfos_packs)
    assert len(packs) == len(blk._tfos_packs)
    assert sum(calls.values()) == 0, calls      # nothing computed yet

    wperm = w2.flip(2, 3).permute(1, 2, 3, 0).to(BF16).contiguous()
    want = {
        "w1b": w1.view(64, cin).to(BF16).contiguous(),
        "w9": w2.permute(0, 2, 3, 1).reshape(64, 576).to(BF16).contiguous(),
        "w3b": w3.view(256, 64).to(BF16).contiguous(),
        "w3bT": w3.view(256, 64).to(BF16).t().contiguous(),
        "w1bT": w1.view(64, cin).to(BF16).t().contiguous(),
    }
    if stride == 1:
        want["w9p"] = wperm
    else:
        for ph in (0, 1):
            for pw in (0, 1):
                taps = [(r, s) for r in range(3) for s in range(3)
                        if (ph - 1 + r) % 2 == 0 and (pw - 1 + s) % 2 == 0]
                want["w9p_{}{}".format(ph, pw)] = torch.stack(
                    [wperm[:, r, s, :] for r, s in taps], dim=1)
    if down:
        want["wdb"] = wd.view(256, 64).to(BF16).contiguous()
        want["wdbT"] = wd.view(256, 64).to(BF16).t().contiguous()
    assert set(want) == set(packs)

    # one key: one eager form runs, once, however often the key is read
    for _ in range(2):
        assert torch.equal(packs["w1b"], want["w1b"])
    assert calls == {"rows": 1, "rows_t": 0, "im2col": 0, "flipped": 0,
                     "parity_class": 0}
    for key, ref in want.items():
        got = packs[key]
        assert got.dtype == BF16 and got.is_contiguous(), key
        assert got.numel() == ref.numel(), key
        assert torch.equal(got.reshape(ref.shape), ref), key
        assert packs[key] is got, key
    n_t = 3 if down else 2                  # rows_t goes through rows
    assert calls == {"rows": (3 if down else 2) + n_t, "rows_t": n_t,
                     "im2col": 1, "flipped": 1,
                     "parity_class": 4 if stride == 2 else 0}
