"""revs_net_risk / revs_net_risk_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records have the
documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
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
    assert re.search(r"\bint revs_net_risk\s*\(", ops) and re.search(r"\bint64_t revs_net_risk_scratch\s*\(", ops)
    for name in ("revs_net_risk", "revs_net_risk_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_risk"][1]) == 26
    decl = re.search(r"\bint revs_net_risk\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == 26
    assert "risk_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    assert re.search(r"#define REVS_RISK_MAX_COMMON 2\b", ops) and _lib.RISK_MAX_COMMON == 2


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    return [re.sub(r"\[\d+\]", "", f.strip()) for f in re.findall(r"(?:double|int32_t)\s+([^;]+);", body)]


def test_record_layouts():
    from revs_admm_amd._lib import RISK_DAY_DTYPE, RISK_SLOT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    assert RISK_SLOT_DTYPE.itemsize == 64 and RISK_DAY_DTYPE.itemsize == 32
    assert re.search(r"\} revs_risk_slot_t;\s*/\* 64 bytes \*/", hdr) and re.search(r"\} revs_risk_day_t;\s*/\* 32 bytes \*/", hdr)
    assert _fields(hdr, "revs_risk_slot_t") == list(RISK_SLOT_DTYPE.names)
    assert _fields(hdr, "revs_risk_day_t") == list(RISK_DAY_DTYPE.names)
    assert {k: RISK_SLOT_DTYPE.fields[k][1] for k in RISK_SLOT_DTYPE.names} == dict(
        expected=0, z_min=8, sd_at=16, drop_at=24, sd_max=32, n_risky=40, n_det=44, z_min_index=48, n_bad=52, reserved=56)
    assert {k: RISK_DAY_DTYPE.fields[k][1] for k in RISK_DAY_DTYPE.names} == dict(prob_max=0, z_min=8, expected_slots=16,
                                                                                 prob_max_slot=24, n_risky=28)
    assert RISK_SLOT_DTYPE["reserved"].shape == (2,)


def test_scratch_size(lib):
    f = lambda S, T, n: 24 * S * T * n
    assert lib.revs_net_risk_scratch(5, 24, 1696) == f(5, 24, 1696)
    assert lib.revs_net_risk_scratch(4096, 192, 16384) == f(4096, 192, 16384)
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    assert "24 S T tree_n" in hdr
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_risk_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), aux=(64, 64, None, 0), node_g=64, node_var=None, common=None, K=0, w2=64,
          limit=None, outm=None, nop=None, n_out=8, drop_max=0.1, z_max=1.645, sd=64, z=None, prob=None, dropq=None, drop=None,
          slot=None, summary=None, day=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import HeadroomAux, Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    ax = None if aux is None else C.byref(HeadroomAux(*aux))
    return lib.revs_net_risk(S, m, T, tr, ax, node_g, node_var, common, K, w2, limit, outm, nop, n_out, drop_max, z_max, sd, z,
                             prob, dropq, drop, slot, summary, day, scratch, None)


def test_net_risk_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    # revs_net_headroom's list
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_risk: S={S}".encode() in err()
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
    assert _call(lib, aux=None) == -1 and b"null aux" in err()
    assert _call(lib, aux=(None, 64, None, 0)) == -1 and b"null aux" in err()
    assert _call(lib, aux=(64, None, None, 0)) == -1 and b"null aux" in err()
    for nj in (-1, 14):
        assert _call(lib, aux=(64, 64, 64, nj)) == -1 and f"n_jump={nj}".encode() in err()
    assert _call(lib, aux=(64, 64, None, 2)) == -1 and b"jump is NULL" in err()
    for bad in (nan, inf, -inf):
        assert _call(lib, drop_max=bad) == -1 and b"drop_max is not finite" in err()
    assert _call(lib, sd=None) == -1 and b"every output is NULL" in err()
    # its own
    for K in (-1, 3, 1 << 20):
        assert _call(lib, common=64, K=K) == -1 and f"K={K} outside 0..2".encode() in err()
    for K in (1, 2):
        assert _call(lib, K=K) == -1 and b"node_common is NULL with K > 0" in err()
    assert _call(lib, w2=None) == -1 and b"w2" in err()
    for bad in (nan, inf, -inf, -0.5):
        assert _call(lib, z_max=bad) == -1 and b"z_max must be finite and >= 0" in err()
    # staged outputs and their scratch; the slot record needs none (refused further on only for want of a device)
    for kw in (dict(summary=96), dict(sd=None, day=32)):
        assert _call(lib, **kw) == -1 and b"need scratch" in err()
        assert _call(lib, scratch=8, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.risk import common_spec, risk_report_device, z_of
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        risk_report_device(g.float(), feeder=feeder)
    with pytest.raises(ValueError, match="contiguous"):
        risk_report_device(g.transpose(1, 2), feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        risk_report_device(g)
    with pytest.raises(ValueError, match="either as feeder"):
        risk_report_device(g, feeder=feeder, tree=(None, None, 3))
    for bad in (0.0, -0.1, 0.6, float("nan")):
        with pytest.raises(ValueError, match="p_max must lie in"):
            z_of(bad)
    assert abs(z_of(0.05) - 1.6448536269514722) < 1e-12 and z_of(0.5) == 0.0
    with pytest.raises(ValueError, match="at most 2 shared factors"):
        common_spec("risk_report", [("load", 0.1)] * 3)
    with pytest.raises(ValueError, match="a shared factor is"):
        common_spec("risk_report", ["load"])
    with pytest.raises(ValueError, match="a shared factor is"):
        common_spec("risk_report", [("pv", 0.1)])
    assert common_spec("risk_report", None) == [] and len(common_spec("risk_report", [("ev", 0.2), np.zeros((3, 4))])) == 2
