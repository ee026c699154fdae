"""revs_net_attribution / revs_net_attribution_scratch (include/revs_admm_ops.h) are declared, exported and bound, the
records have the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
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
    assert re.search(r"\bint revs_net_attribution\s*\(", ops) and re.search(r"\bint64_t revs_net_attribution_scratch\s*\(", ops)
    for name in ("revs_net_attribution", "revs_net_attribution_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_attribution"][1]) == 25
    decl = re.search(r"\bint revs_net_attribution\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == 25
    assert "attribution_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    return [re.sub(r"\[\d+\]", "", f.strip()) for f in re.findall(r"(?:double|int32_t)\s+([^;]+);", body)]


def test_record_layouts():
    from revs_admm_amd._lib import ATTR_DAY_DTYPE, ATTR_SLOT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    assert ATTR_SLOT_DTYPE.itemsize == 192 and ATTR_DAY_DTYPE.itemsize == 32
    assert re.search(r"\} revs_attr_slot_t;\s*/\* 192 bytes \*/", hdr) and re.search(r"\} revs_attr_day_t;\s*/\* 32 bytes \*/", hdr)
    assert _fields(hdr, "revs_attr_slot_t") == list(ATTR_SLOT_DTYPE.names)
    assert _fields(hdr, "revs_attr_day_t") == list(ATTR_DAY_DTYPE.names)
    assert {k: ATTR_SLOT_DTYPE.fields[k][1] for k in ATTR_SLOT_DTYPE.names} == dict(
        drop_watch=0, excess=8, total=16, ev_total=24, class_total=32, top_value=64, top_index=128, watch=160, n_reach=164,
        n_big=168, n_can=172, n_bad=176, reserved=180)
    assert {k: ATTR_DAY_DTYPE.fields[k][1] for k in ATTR_DAY_DTYPE.names} == dict(sum=0, ev_sum=8, peak=16, peak_slot=24,
                                                                                 n_big=28)
    assert ATTR_SLOT_DTYPE["class_total"].shape == (4,) and ATTR_SLOT_DTYPE["top_value"].shape == (8,)
    assert ATTR_SLOT_DTYPE["top_index"].shape == (8,) and ATTR_SLOT_DTYPE["reserved"].shape == (3,)


def test_scratch_size(lib):
    f = lambda S, T, n: 17 * S * T * n + 192 * S * T
    assert lib.revs_net_attribution_scratch(5, 24, 1696) == f(5, 24, 1696)
    assert lib.revs_net_attribution_scratch(4096, 192, 16384) == f(4096, 192, 16384)
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    assert "17 S T tree_n" in hdr and "+ 192 S T" in hdr
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_attribution_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), aux=(64, 64, None, 0), node_g=64, node_ev=None, limit=None, outm=None,
          cls=None, n_cls=0, nop=None, n_out=8, watch=-1, drop_max=0.1, frac=0.01, sens=64, contrib=None, evc=None, drop=None,
          slot=None, summary=None, day=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import HeadroomAux, Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    ax = None if aux is None else C.byref(HeadroomAux(*aux))
    return lib.revs_net_attribution(S, m, T, tr, ax, node_g, node_ev, limit, outm, cls, n_cls, nop, n_out, watch, drop_max,
                                    frac, sens, contrib, evc, drop, slot, summary, day, scratch, None)


def test_net_attribution_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    # revs_net_headroom's list
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_attribution: S={S}".encode() in err()
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
    assert _call(lib, sens=None) == -1 and b"every output is NULL" in err()
    # its own
    for w in (-2, 8, 1 << 20):
        assert _call(lib, watch=w) == -1 and f"watch_pos={w}".encode() in err()
    for bad in (nan, inf, -inf, -0.5):
        assert _call(lib, frac=bad) == -1 and b"frac must be finite and >= 0" in err()
    for n_cls in (-1, 5):
        assert _call(lib, cls=64, n_cls=n_cls) == -1 and f"C={n_cls}".encode() in err()
    assert _call(lib, n_cls=2) == -1 and b"class_of_pos is NULL" in err()
    assert _call(lib, evc=64) == -1 and b"ev_contrib_out needs node_ev" in err()
    # outputs and their scratch
    for kw in (dict(slot=192), dict(summary=96), dict(sens=None, day=32)):
        assert _call(lib, **kw) == -1 and b"need scratch" in err()
        assert _call(lib, scratch=8, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.attribution import attribution_report_device
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        attribution_report_device(g.float(), feeder=feeder)
    with pytest.raises(ValueError, match="contiguous"):
        attribution_report_device(g.transpose(1, 2), feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        attribution_report_device(g)
    with pytest.raises(ValueError, match="either as feeder"):
        attribution_report_device(g, feeder=feeder, tree=(None, None, 3))


def test_class_array_takes_a_class_out_of_range_as_no_class():
    """attribution.class_array refuses only a wrong length before tree_reports.position_classes: 4 or more, like a
    negative entry, is no class (255), not an error."""
    import torch
    from revs_admm_amd.attribution import class_array
    from revs_admm_amd.feeder import feeder_tree
    parent = np.array([-1, 0, 1, 1, 0])
    th = feeder_tree(parent, np.ones(5), np.array([-1, 0, -1, 1, 2]), np.ones(3, bool))
    order = np.asarray(th["order"])
    real = order < 5
    dev = torch.device("cpu")
    cls = np.array([1, 4, -1, 0, 9])
    by_pos, n_cls = class_array(dev, th, 5, cls)
    want = np.where((cls >= 0) & (cls < 4), cls, 255)
    assert n_cls == 2 and (by_pos.numpy() == np.where(real, want[np.where(real, order, 0)], 255)).all()
    assert class_array(dev, th, 5, np.full(5, 7))[1] == 0
    with pytest.raises(ValueError, match=r"attribution report: classes must have one entry per tree node \(5\), got \(4,\)"):
        class_array(dev, th, 5, np.zeros(4, int))
