"""revs_net_headroom / revs_net_headroom_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records
have the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
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
    assert re.search(r"\bint revs_net_headroom\s*\(", ops) and re.search(r"\bint64_t revs_net_headroom_scratch\s*\(", ops)
    for name in ("revs_net_headroom", "revs_net_headroom_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_headroom"][1]) == 21
    assert "headroom_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.HEADROOM_MAX_JUMP == 13 and "#define REVS_HEADROOM_MAX_JUMP 13" in ops


def test_record_layouts():
    from revs_admm_amd._lib import HEADROOM_DAY_DTYPE, HeadroomAux
    from revs_admm_amd.network import SUMMARY_DTYPE
    assert HEADROOM_DAY_DTYPE.itemsize == 16 and SUMMARY_DTYPE.itemsize == 96
    assert {k: HEADROOM_DAY_DTYPE.fields[k][1] for k in HEADROOM_DAY_DTYPE.names} == dict(min=0, slot=8, n_short=12)
    assert SUMMARY_DTYPE.fields["reserved"][1] == 84           # (n_unlimited is reserved[0])
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} revs_headroom_day_t;", hdr).group(1), flags=re.S)
    assert [f.strip() for f in re.findall(r"(?:double|int32_t)\s+([^;]+);", body)] == ["min", "slot", "n_short"]
    body = re.search(r"typedef struct \{([^}]*)\} revs_headroom_aux_t;", hdr).group(1)
    assert re.findall(r"\b(\w+);", body) == ["parent_pos", "wc", "jump", "n_jump"] == [f[0] for f in HeadroomAux._fields_]
    assert C.sizeof(HeadroomAux) == 32


def test_scratch_size(lib):
    assert lib.revs_net_headroom_scratch(5, 24, 1696) == 8 * 5 * 24 * 1696
    assert lib.revs_net_headroom_scratch(4096, 192, 16384) == 8 * 4096 * 192 * 16384
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_headroom_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), aux=(64, 64, None, 0), node_g=64, rating=None, limit=None, outm=None,
          nop=None, n_out=8, drop_max=0.1, need=4.8, head=64, lim=None, drop=None, flow=None, summary=None, day=None,
          scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import HeadroomAux, Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    ax = None if aux is None else C.byref(HeadroomAux(*aux))
    return lib.revs_net_headroom(S, m, T, tr, ax, node_g, rating, limit, outm, nop, n_out, drop_max, need, head, lim, drop,
                                 flow, summary, day, scratch, None)


def test_net_headroom_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_headroom: S={S}".encode() in err()
    # every case of revs_net_report
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
    # the aux struct
    assert _call(lib, aux=None) == -1 and b"null aux" in err()
    assert _call(lib, aux=(None, 64, None, 0)) == -1 and b"null aux" in err()
    assert _call(lib, aux=(64, None, None, 0)) == -1 and b"null aux" in err()
    for nj in (-1, 14):
        assert _call(lib, aux=(64, 64, 64, nj)) == -1 and f"n_jump={nj}".encode() in err()
    assert _call(lib, aux=(64, 64, None, 2)) == -1 and b"jump is NULL" in err()
    # the limits
    for bad in (nan, inf, -inf):
        assert _call(lib, drop_max=bad) == -1 and b"drop_max is not finite" in err()
        assert _call(lib, need=bad) == -1 and b"need must be finite" in err()
    assert _call(lib, need=-0.5) == -1 and b"need must be finite and >= 0" in err()
    # outputs and their scratch
    assert _call(lib, head=None) == -1 and b"every output is NULL" in err()
    assert _call(lib, summary=96) == -1 and b"need scratch" in err()
    assert _call(lib, head=None, day=16) == -1 and b"need scratch" in err()
    assert _call(lib, summary=96, scratch=8) == -1 and b"16-byte aligned" in err()
    assert _call(lib, head=None, day=16, scratch=24) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.headroom import headroom_report_device
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        headroom_report_device(g.float(), feeder=feeder)
    with pytest.raises(ValueError, match="contiguous"):
        headroom_report_device(g.transpose(1, 2), feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        headroom_report_device(g)
    with pytest.raises(ValueError, match="either as feeder"):
        headroom_report_device(g, feeder=feeder, tree=(None, None, 3))


def test_position_mask_reads_none_as_the_nodes_with_a_row():
    """headroom.position_mask is tree_reports.position_mask with none="rows": None is the nodes that carry a row, a
    selection is that selection, by position; a boolean mask's length is not checked here (who=None)."""
    import torch
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.headroom import position_mask
    parent, cons_of = np.array([-1, 0, 1, 1, 0]), np.array([-1, 0, -1, 1, 2])     # rows at the nodes 1, 3 and 4
    th = feeder_tree(parent, np.ones(5), cons_of, np.ones(3, bool))
    order = np.asarray(th["order"])
    real = order < 5
    dev = torch.device("cpu")
    with_row = np.isin(order, [1, 3, 4]) & real
    assert (position_mask(dev, th, 5, None).numpy() == with_row).all() and with_row.sum() == 3
    want = real & np.isin(order, [0, 2])
    assert (position_mask(dev, th, 5, [0, 2]).numpy() == want).all()
    assert (position_mask(dev, th, 5, np.array([True, False, True, False, False])).numpy() == want).all()
    assert position_mask(dev, th, 5, None).dtype == torch.uint8
