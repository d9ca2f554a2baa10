"""The measured-table routing of the streaming ops, held to recorded answers.

``golden/routes.json`` holds what ``_dw_auto``, ``_pw_auto``, ``_cth_auto``
and ``_ub_auto`` (per direction) and the matching ``_xx_route`` under ``auto``
answered at the commit before the four nearest-row rules became one function,
plus ``_ctw_auto`` at the cases of test_convt_wrw_cpu.py. The shapes, per op:
every table row, every row with N + 1 and with N halved, the geometric
midpoint in size between size-adjacent rows and one step of N to either side
of it (where the tie-break lives), one shape far below the smallest row and
one far above the largest, and for depthwise a stride without rows.
``PYTHONPATH=. python tests/test_routes_cpu.py OUT.json`` writes such a file.
An answer that differs from it is a routing change.

Also here: every routing switch read from the environment rejects an unknown
value by name and takes each documented one.
"""

import json
import math
import os
import sys

import pytest
import torch

import tensorflowonspark_amd.ops.modules as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "routes.json")

# op: (table, switch, directions (None: _auto takes none), key columns,
#      size of a key, the key of batch n whose other sizes are smallest)
OPS = {
    "dw": ("_dw_table", "TFOS_DW", ("fwd", "dgrad", "wrw"), 5,
           lambda k: k[0] * k[1] * k[2] * k[3],
           lambda n, row: (n, 1, 1, 1, row[4])),
    "pw": ("_pw_table", "TFOS_PW", None, 5,
           lambda k: k[0] * k[3] * k[4] * (k[1] + k[2]),
           lambda n, row: (n, 1, 1, 1, 1)),
    "cth": ("_cth_table", "TFOS_CONVT_HEAD", ("fwd", "dgrad", "wrw"), 5,
            lambda k: k[0] * k[1] * k[3] * k[4],
            lambda n, row: (n, 1, row[2], 1, 1)),
    "ub": ("_ub_table", "TFOS_UPSAMPLE", ("fwd", "bwd"), 6,
           lambda k: k[0] * k[1] * k[4] * k[5],
           lambda n, row: (n, 1, 1, 1, 1, 1)),
}


def _shapes(op):
    """The argument tuples of one op, in a fixed order, without repeats."""
    table, _, _, nkey, size, unit = OPS[op]
    rows = getattr(M, table)()
    out = []
    for r in rows:
        k = tuple(r[:nkey])
        out += [k, (k[0] + 1,) + k[1:], (k[0] // 2,) + k[1:]]
    # dw only ever compares rows of one stride (column 4)
    groups = sorted({r[4] for r in rows}) if op == "dw" else [None]
    for g in groups:
        grp = [r for r in rows if g is None or r[4] == g]
        sizes = sorted({size(r) for r in grp})
        step = size(unit(1, grp[0]))
        for lo, hi in zip(sizes, sizes[1:]):
            n = int(math.sqrt(lo * hi)) // step
            out += [unit(n + d, grp[0]) for d in (-1, 0, 1)]
        out += [unit(1, grp[0]), unit(sizes[-1] * 4096 // step, grp[0])]
    if op == "dw":
        out.append(tuple(rows[0][:4]) + (3,))
    seen = set()
    return [k for k in out if not (k in seen or seen.add(k))]


def _answers(op, args, mp):
    _, switch, directions, _, _, _ = OPS[op]
    auto = getattr(M, "_{}_auto".format(op))
    mp.setenv(switch, "auto")
    route = getattr(M, "_{}_route".format(op))(*args)
    got = list(auto(*args)) if directions is None \
        else [auto(d, *args) for d in directions]
    return [list(args), got, None if route is None else list(route)]


# N, cin, cout, H, W on the shipped _ctw_table
CTW = [(64, 152, 64, 32, 32), (65, 152, 64, 32, 32), (63, 152, 64, 32, 32),
       (64, 320, 512, 4, 4), (1024, 320, 512, 4, 4), (4096, 160, 64, 32, 32),
       (4096, 152, 72, 32, 32), (4096, 152, 64, 32, 31),
       (4096, 152, 64, 16, 32), (4096, 64, 96, 64, 64)]


def _ctw_cases():
    out = list(CTW)
    for r in M._ctw_table():
        out += [(r[4],) + tuple(r[:4]), (r[4] - 1,) + tuple(r[:4]),
                (r[4] + 1,) + tuple(r[:4])]
    return out


def _record(mp):
    out = {op: [_answers(op, a, mp) for a in _shapes(op)] for op in OPS}
    out["ctw"] = [[list(a), M._ctw_auto(*a)] for a in _ctw_cases()]
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("op", sorted(OPS))
def test_auto_and_route_answer_as_recorded(op, golden, monkeypatch):
    assert len(golden[op]) >= 3 * len(getattr(M, OPS[op][0])())
    for args, auto, route in golden[op]:
        got = _answers(op, tuple(args), monkeypatch)
        assert got == [args, auto, route], (op, args)


def test_ctw_auto_answers_as_recorded(golden):
    assert len(golden["ctw"]) >= len(CTW)
    for args, want in golden["ctw"]:
        assert M._ctw_auto(*args) is want, args


def test_the_file_covers_the_shapes_listed_above(golden):
    # a table that grew without a new recording fails here, not silently
    for op in OPS:
        assert [c[0] for c in golden[op]] == [list(a) for a in _shapes(op)]
    assert [c[0] for c in golden["ctw"]] == [list(a) for a in _ctw_cases()]


_CPU_X = torch.zeros(2, 16, 3, 3, dtype=torch.bfloat16)
SWITCHES = {
    "TFOS_DW": (("auto", "hip", "miopen"),
                lambda: M._dw_route(64, 32, 64, 64, 1)),
    "TFOS_PW": (("auto", "hip", "miopen"),
                lambda: M._pw_route(64, 32, 16, 64, 64)),
    "TFOS_CONVT_HEAD": (("auto", "hip", "miopen"),
                        lambda: M._cth_route(64, 80, 3, 64, 64)),
    "TFOS_UPSAMPLE": (("auto", "hip", "aten"),
                      lambda: M._ub_route(32, 21, 32, 32, 512, 512)),
    "TFOS_CONVT_WRW": (("auto", "hip", "miopen"),
                       lambda: M._ctw_route(_CPU_X, (6, 6), 16, 8, 4, 2, 1)),
    "TFOS_ATROUS": (("auto", "mfma", "miopen"),
                    lambda: M._atrous_route(2, 16, 16, 64, 96, 2)),
    "TFOS_BN_EPI": (("auto", "off", "force"), lambda: M._bn_epi_mode()),
    "TFOS_BN_GATE": (("auto", "off", "force"), lambda: M._bn_gate_mode()),
    "TFOS_STEM_POOL": (("on", "off"), lambda: M._stem_pool_mode()),
}


@pytest.mark.parametrize("var", sorted(SWITCHES))
def test_switch_rejects_an_unknown_value_by_name(var, monkeypatch):
    values, read = SWITCHES[var]
    monkeypatch.setenv(var, "bogus")
    with pytest.raises(ValueError, match=var + " must be .* or " + values[-1]
                       + ", got 'bogus'"):
        read()
    for v in values:
        monkeypatch.setenv(var, v)
        read()
    monkeypatch.delenv(var)
    read()


if __name__ == "__main__":
    with pytest.MonkeyPatch.context() as mp:
        recorded = _record(mp)
    with open(sys.argv[1], "w") as f:
        json.dump(recorded, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
