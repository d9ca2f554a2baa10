"""TFOS_CONVT_WRW routing, the convt_wrw launch plan and the exact-probe
premise, without a GPU."""

import pytest
import torch

from convt_wrw_cases import CASES, case, exact_premise
from tensorflowonspark_amd.ops import get_ext
from tensorflowonspark_amd.ops import modules as M


def test_auto_is_an_exact_class_match_with_a_minimum_batch(monkeypatch):
    for row in M._ctw_table():                 # the shipped table's own rows
        assert M._ctw_auto(row[4], *row[:4]) and len(row) == 5
    monkeypatch.setattr(M, "_ctw_table", lambda: ((152, 64, 32, 32, 64),
                                                  (320, 512, 4, 4, 1024)))
    assert M._ctw_auto(64, 152, 64, 32, 32)
    assert M._ctw_auto(65, 152, 64, 32, 32)
    assert not M._ctw_auto(63, 152, 64, 32, 32)
    assert not M._ctw_auto(64, 320, 512, 4, 4)
    assert M._ctw_auto(1024, 320, 512, 4, 4)
    for near in ((160, 64, 32, 32), (152, 72, 32, 32), (152, 64, 32, 31),
                 (152, 64, 16, 32), (64, 96, 64, 64)):
        assert not M._ctw_auto(4096, *near)    # no nearest-shape rule


def test_route_reads_the_switch_at_call_time(monkeypatch):
    x = torch.zeros(2, 16, 3, 3, dtype=torch.bfloat16)
    monkeypatch.setenv("TFOS_CONVT_WRW", "fast")
    with pytest.raises(ValueError, match="TFOS_CONVT_WRW"):
        M._ctw_route(x, (6, 6), 16, 8, 4, 2, 1)
    for mode in ("hip", "miopen", "auto"):     # a CPU tensor never goes in-tree
        monkeypatch.setenv("TFOS_CONVT_WRW", mode)
        assert M._ctw_route(x, (6, 6), 16, 8, 4, 2, 1) is False
    # TFOS_CONVT_WRW leaves _wrw_backend alone: transposed is always "lib"
    assert M._wrw_backend("mfma2", 4, 64, 96, 2, transposed=True) == "lib"


def test_plan_modes():
    plan = get_ext(required=True).convt_wrw_plan
    for name, ((N, cin, cout, H, W), reaches) in CASES.items():
        p = plan(N, H, W, cin, cout)
        G = N * H
        assert p["eligible"] and reaches(p, G), (name, p)
        assert p["block_rows"] <= p["slab_rows"] or p["slabs"] == 1
        assert (p["slabs"] - 1) * p["slab_rows"] < G <= p["slabs"] * p["slab_rows"]
        assert p["grid"] == p["slabs"] * 4 * p["tiles"]
        assert p["lds_bytes"] == ((2 * p["block_rows"] + 1) * W + 1) * 144
        assert p["ws_bytes"] == (p["slabs"] > 1) * p["slabs"] * 64 * cin * cout
    # the U-Net classes: up1 is all tiles, up4 all pixels; workspace bounded
    up1, up4 = plan(64, 4, 4, 320, 512), plan(64, 32, 32, 152, 64)
    assert up1["slabs"] == 1 and up1["tiles"] == 40
    assert up4["slabs"] > 16 and up4["tiles"] == 3 and up4["grid"] >= 512
    for N in (64, 1024):
        for cin, cout, hw in ((320, 512, 4), (608, 256, 8), (288, 128, 16),
                              (152, 64, 32)):
            p = plan(N, hw, hw, cin, cout)
            assert p["ws_bytes"] <= 32 << 20 and p["lds_bytes"] <= 160 * 1024
    assert not plan(1, 1, 379, 8, 8)["eligible"]
    assert plan(1, 1, 378, 8, 8)["lds_bytes"] <= 160 * 1024
    with pytest.raises(RuntimeError, match="multiples of 8"):
        plan(1, 4, 4, 12, 8)


def test_exact_probe_premise():
    for shape, _ in CASES.values():
        assert exact_premise(*shape) < 2 ** 24
    shape = CASES["n3_cout_tail_24"][0]
    _, _, ref, aref = case(shape, True)
    assert torch.equal(ref, ref.round()) and aref.max() <= exact_premise(*shape)
    # every (ci, co) pair has a filter of its own
    assert len({tuple(f.flatten().tolist()) for f in ref.flatten(0, 1)}) == 32 * 24
