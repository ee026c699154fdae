"""revs_net_prices / revs_net_prices_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records have
the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_net_prices\s*\(", ops) and re.search(r"\bint64_t revs_net_prices_scratch\s*\(", ops)
    for name in ("revs_net_prices", "revs_net_prices_scratch"):
        assert name not in boundary
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_prices"][1]) == 30
    decl = re.search(r"\bint revs_net_prices\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == 30
    assert "price_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    import revs_admm_amd.prices as prices
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    assert hasattr(AdmmEngine, "price_report") and hasattr(AdmmEnsemble, "price_reports")
    assert all(hasattr(prices, k) for k in ("PriceReport", "native_prices_device", "price_report_device", "report_for_tree"))


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    out = []
    for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body):
        out += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    return out


def test_record_layouts():
    from revs_admm_amd._lib import PRICE_DAY_DTYPE, PRICE_NODE_DAY_DTYPE, PRICE_SLOT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    off = lambda dt: {k: dt.fields[k][1] for k in dt.names}
    assert PRICE_SLOT_DTYPE.itemsize == 96 and "} revs_price_slot_t;                  /* 96 bytes */" in hdr
    assert off(PRICE_SLOT_DTYPE) == dict(delivered=0, energy_pay=8, loss_pay=16, cong_pay=24, rent_total=32, price_max=40,
                                         price_min=48, cong_max=56, price_max_index=64, price_min_index=68,
                                         cong_max_index=72, n_priced=76, n_rows=80, n_bad=84, reserved=88)
    assert _fields(hdr, "revs_price_slot_t") == list(PRICE_SLOT_DTYPE.names)
    assert PRICE_NODE_DAY_DTYPE.itemsize == 32 and "} revs_price_node_day_t;              /* 32 bytes */" in hdr
    assert off(PRICE_NODE_DAY_DTYPE) == dict(paid=0, cong_paid=8, peak_price=16, peak_slot=24, reserved=28)
    assert _fields(hdr, "revs_price_node_day_t") == list(PRICE_NODE_DAY_DTYPE.names)
    assert PRICE_DAY_DTYPE.itemsize == 160 and "} revs_price_day_t;                   /* 160 bytes */" in hdr
    assert off(PRICE_DAY_DTYPE) == dict(energy_pay=0, loss_pay=8, cong_pay=16, rent_total=24, peak_price=32, top_rent=40,
                                        top_index=104, peak_slot=136, peak_index=140, n_bad_slots=144, n_cong_slots=148,
                                        reserved=152)
    assert _fields(hdr, "revs_price_day_t") == list(PRICE_DAY_DTYPE.names)
    assert PRICE_DAY_DTYPE["top_index"].shape == (8,) and PRICE_DAY_DTYPE["top_rent"].shape == (8,)


def test_scratch_size(lib):
    size = lambda S, T, n: 32 * S * T * n + 96 * S * T + 8 * S * n
    assert lib.revs_net_prices_scratch(5, 24, 1696) == size(5, 24, 1696)
    assert lib.revs_net_prices_scratch(4096, 192, 16384) == size(4096, 192, 16384)
    assert lib.revs_net_prices_scratch(1, 1, 8) % 16 == 0
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_prices_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), node_g=64, node_y=64, scale=None, cost=64, lmask=None, nmask=None, nop=None,
          n_out=8, vset2=1.0, with_loss=1, hours=1.0, cap=float("inf"), price=64, cong=None, lossp=None, line_y=None,
          rent=None, drop=None, flow=None, summary=None, slot=None, node_day=None, line_day=None, day=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    return lib.revs_net_prices(S, m, T, tr, node_g, node_y, scale, cost, lmask, nmask, nop, n_out, vset2, with_loss, hours,
                               cap, price, cong, lossp, line_y, rent, drop, flow, summary, slot, node_day, line_day, day,
                               scratch, None)


def test_net_prices_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    # net_tree_checks' cases
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_prices: S={S}".encode() in err()
    for T in (0, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    for m in (0, 65536):
        assert _call(lib, m=m) == -1 and f"m={m}".encode() in err()
    assert _call(lib, node_g=None) == -1 and b"node_g" in err()
    assert _call(lib, tree=None) == -1 and b"tree of 0 nodes" in err()
    assert _call(lib, tree=(12, 64, 64)) == -1 and b"tree of 12 nodes" in err()            # not padded
    assert _call(lib, tree=(16392, 64, 64)) == -1 and b"tree of 16392 nodes" in err()
    assert _call(lib, tree=(8200, 64, 64)) == -1 and b"tree of 8200 nodes" in err()        # a multiple of 16 beyond 8192
    assert _call(lib, tree=(8, None, 64)) == -1 and _call(lib, tree=(8, 64, None)) == -1
    for n_out in (0, 9, -1):
        assert _call(lib, n_out=n_out) == -1 and f"n_out={n_out}".encode() in err()
    # the multipliers and the tariff
    assert _call(lib, node_y=None) == -1 and b"node_y" in err()
    assert _call(lib, cost=None) == -1 and b"cost" in err()
    # the scalars: vset2 only with the loss term; price_cap may be +-inf
    for bad in (nan, inf, -inf, 0.0, -1.0):
        assert _call(lib, vset2=bad) == -1 and b"vset2 must be finite and > 0" in err()
        assert _call(lib, hours=bad) == -1 and b"slot_hours must be finite and > 0" in err()
    assert _call(lib, cap=nan) == -1 and b"price_cap is a NaN" in err()
    # outputs and their scratch
    assert _call(lib, price=None) == -1 and b"every output is NULL" in err()
    for kw in (dict(summary=96), dict(node_day=32), dict(line_day=24), dict(day=160), dict(price=None, day=160)):
        assert _call(lib, **kw) == -1 and b"need scratch" in err()
        assert _call(lib, scratch=24, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.prices import native_prices_device, price_report_device, scales_of
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        price_report_device(g.float(), g, feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        price_report_device(g, g)
    cost = np.ones(4)
    for kw, msg in ((dict(vset=0.0), "vset"), (dict(slot_hours=-1.0), "slot_hours"), (dict(price_cap=float("nan")), "price_cap"),
                    (dict(cost=None), "cost is required"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
                    (dict(scale=np.ones(3)), "scale")):
        with pytest.raises(ValueError, match=msg):
            native_prices_device(None, g.device, None, None, None, 3, g, g, **dict(dict(cost=cost), **kw))
    with pytest.raises(ValueError, match="node_y"):
        native_prices_device(None, g.device, None, None, None, 3, g, g[:1], cost=cost)
    assert scales_of(0.5, 3).tolist() == [0.5] * 3 and scales_of([0.0, 1.0], 2).tolist() == [0.0, 1.0]


def test_report_methods_on_the_host():
    """reinforcement_value() = 2 s Y flow, shares() in %, top_lines: formed on the host from the report's fields."""
    from revs_admm_amd._lib import LOSS_LINE_DAY_DTYPE, PRICE_DAY_DTYPE, PRICE_NODE_DAY_DTYPE, PRICE_SLOT_DTYPE
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.prices import PriceReport
    day = np.zeros((), PRICE_DAY_DTYPE)
    day["energy_pay"], day["loss_pay"], day["cong_pay"] = 70.0, 10.0, 20.0
    day["top_index"], day["top_rent"] = [3, 1] + [-1] * 6, [2.0, 0.5] + [np.nan] * 6
    Y, flow = np.array([[0.5, 0.0]]), np.array([[3.0, 1.0]])
    rep = PriceReport(None, None, None, Y, None, None, flow, np.zeros(2, SUMMARY_DTYPE), np.zeros(2, PRICE_SLOT_DTYPE),
                      np.zeros(1, PRICE_NODE_DAY_DTYPE), np.zeros(1, LOSS_LINE_DAY_DTYPE), day, 0.25, 1.0, 12.0)
    assert rep.reinforcement_value().tolist() == [[0.75, 0.0]]
    assert rep.shares() == dict(energy=70.0, loss=10.0, congestion=20.0) and rep.top_lines == [(3, 2.0), (1, 0.5)]
    rep.line_y = None
    with pytest.raises(ValueError, match="arrays=True"):
        rep.reinforcement_value()
