"""revs_net_powerflow / revs_net_powerflow_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records
have the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = 27


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_net_powerflow\s*\(", ops) and re.search(r"\bint64_t revs_net_powerflow_scratch\s*\(", ops)
    for name in ("revs_net_powerflow", "revs_net_powerflow_scratch"):
        assert name not in boundary
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_powerflow"][1]) == N_ARGS
    decl = re.search(r"\bint revs_net_powerflow\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == N_ARGS
    assert len(_lib.SIGNATURES["revs_net_powerflow_scratch"][1]) == 3
    assert "powerflow_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "#define REVS_PF_MAX_ITER 64" in ops and _lib.PF_MAX_ITER == 64


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    out = []
    for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body):
        out += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    return out


def test_record_layouts():
    from revs_admm_amd._lib import PF_DAY_DTYPE, PF_NODE_DAY_DTYPE, PF_SLOT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    off = lambda dt: {k: dt.fields[k][1] for k in dt.names}
    assert PF_SLOT_DTYPE.itemsize == 80 and "} revs_pf_slot_t;                     /* 80 bytes */" in hdr
    assert off(PF_SLOT_DTYPE) == dict(loss_total=0, qloss_total=8, delivered=16, supplied=24, volt_min=32, err_max=40,
                                      volt_min_index=48, err_index=52, n_below=56, n_below_lin=60, n_missed=64, iters=68,
                                      status=72, reserved=76)
    assert _fields(hdr, "revs_pf_slot_t") == list(PF_SLOT_DTYPE.names)
    assert PF_NODE_DAY_DTYPE.itemsize == 24 and "} revs_pf_node_day_t;                 /* 24 bytes */" in hdr
    assert off(PF_NODE_DAY_DTYPE) == dict(volt_min=0, slot=8, slots_below=12, slots_missed=16, reserved=20)
    assert _fields(hdr, "revs_pf_node_day_t") == list(PF_NODE_DAY_DTYPE.names)
    assert PF_DAY_DTYPE.itemsize == 64 and "} revs_pf_day_t;                      /* 64 bytes */" in hdr
    assert off(PF_DAY_DTYPE) == dict(energy_lost=0, energy_delivered=8, cost=16, volt_min=24, volt_min_slot=32,
                                     volt_min_index=36, n_below=40, n_below_lin=44, n_missed=48, iters_max=52, n_bad_slots=56,
                                     reserved=60)
    assert _fields(hdr, "revs_pf_day_t") == list(PF_DAY_DTYPE.names)


def test_scratch_size(lib):
    size = lambda S, T, n: 6 * 8 * S * T * n + 80 * S * T
    assert lib.revs_net_powerflow_scratch(5, 24, 1696) == size(5, 24, 1696)
    assert lib.revs_net_powerflow_scratch(4096, 192, 16384) == size(4096, 192, 16384)
    assert lib.revs_net_powerflow_scratch(1, 1, 8) % 16 == 0
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_powerflow_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), node_g=64, xw=None, tan_phi=0.0, nmask=None, nop=None, n_out=8, vset2=1.0,
          vmin=0.95, tol=1e-12, max_iter=32, hours=1.0, cost=None, volt=64, volt_lin=None, flow=None, loss=None, qflow=None,
          summary=None, slot=None, node_day=None, day=None, scratch=64):
    # (non-null "pointers" that are never dereferenced: every call here is refused before any launch)
    from revs_admm_amd._lib import Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    return lib.revs_net_powerflow(S, m, T, tr, node_g, xw, tan_phi, nmask, nop, n_out, vset2, vmin, tol, max_iter, hours, cost,
                                  volt, volt_lin, flow, loss, qflow, summary, slot, node_day, day, scratch, None)


def test_net_powerflow_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    # the shared tree and size checks
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_powerflow: S={S}".encode() in err()
    for T in (0, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    for m in (0, 65536):
        assert _call(lib, m=m) == -1 and f"m={m}".encode() in err()
    assert _call(lib, node_g=None) == -1 and b"node_g" in err()
    assert _call(lib, tree=None) == -1 and b"tree of 0 nodes" in err()
    assert _call(lib, tree=(12, 64, 64)) == -1 and b"tree of 12 nodes" in err()
    assert _call(lib, tree=(16392, 64, 64)) == -1 and b"tree of 16392 nodes" in err()
    assert _call(lib, tree=(8200, 64, 64)) == -1 and b"tree of 8200 nodes" in err()
    assert _call(lib, tree=(8, None, 64)) == -1 and _call(lib, tree=(8, 64, None)) == -1
    for n_out in (0, 9, -1):
        assert _call(lib, n_out=n_out) == -1 and f"n_out={n_out}".encode() in err()
    # the scalars
    for bad in (nan, inf, -inf, 0.0, -1.0):
        assert _call(lib, vset2=bad) == -1 and b"vset2 must be finite and > 0" in err()
        assert _call(lib, hours=bad) == -1 and b"slot_hours must be finite and > 0" in err()
        assert _call(lib, tol=bad) == -1 and b"tol must be finite and > 0" in err()
    for bad in (nan, inf, -inf):
        assert _call(lib, vmin=bad) == -1 and b"vmin must be finite" in err()
        assert _call(lib, tan_phi=bad, xw=64) == -1 and b"tan_phi must be finite" in err()
    for bad in (0, -1, 65, 1 << 20):
        assert _call(lib, max_iter=bad) == -1 and f"max_iter={bad} outside 1..64".encode() in err()
    # the reactive part needs the reactances
    assert _call(lib, tan_phi=0.3) == -1 and b"tan_phi != 0 needs xw" in err()
    assert _call(lib, qflow=64) == -1 and b"qflow_out needs xw" in err()
    assert _call(lib, xw=72) == -1 and b"xw must be 16-byte aligned" in err()
    # outputs and the scratch
    assert _call(lib, volt=None) == -1 and b"every output is NULL" in err()
    for kw in (dict(summary=96), dict(node_day=24), dict(day=64), dict(volt=None, day=64), dict()):
        assert _call(lib, scratch=None, **kw) == -1 and b"scratch" in err()
        assert _call(lib, scratch=24, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.powerflow import native_powerflow_device, powerflow_report_device, tan_phi_of
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        powerflow_report_device(g.float(), feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        powerflow_report_device(g)
    for kw, msg in ((dict(vset=0.0), "vset"), (dict(slot_hours=-1.0), "slot_hours"), (dict(tol=0.0), "tol"),
                    (dict(vmin=float("nan")), "vmin"), (dict(max_iter=65), "max_iter"), (dict(max_iter=0), "max_iter"),
                    (dict(power_factor=0.0), "power_factor"), (dict(power_factor=1.5), "power_factor")):
        with pytest.raises(ValueError, match=msg):
            native_powerflow_device(None, g.device, None, None, None, 3, g, **kw)
    assert tan_phi_of(1.0) == 0.0 and abs(tan_phi_of(0.95) - 0.3286841051788632) < 1e-15


def test_reactances_are_laid_out_as_the_weights():
    """position_xw lays 2 x out by tree["order"] exactly as feeder_tree lays out w = 2 r, 0 at the padding positions."""
    import torch
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.powerflow import position_xw
    parent, er = np.array([-1, 0, 1, 1, 0]), np.array([0.5, 0.25, 1.0, 2.0, 4.0])
    th = feeder_tree(parent, er, np.array([-1, 0, -1, 1, 2]), np.ones(3, bool))
    dev = torch.device("cpu")
    assert position_xw(dev, th, 5, None) is None
    assert (position_xw(dev, th, 5, er).numpy() == th["w"]).all()
    for bad in (np.ones(4), np.array([1.0, 1.0, np.nan, 1.0, 1.0])):
        with pytest.raises(ValueError, match="one finite reactance per tree node"):
            position_xw(dev, th, 5, bad)


def test_feeder_reactances_walks_as_feeder_arrays_does():
    import networkx as nx
    from revs_admm_amd.lpsolver import feeder_arrays, feeder_reactances
    g = nx.Graph()
    for n, lab in ((0, "S"), (1, "T"), (2, "H"), (3, "H"), (4, "R")):
        g.add_node(n, label=lab)
    for u, v, r in ((0, 1, 0.1), (1, 4, 0.2), (4, 2, 0.3), (4, 3, 0.4)):
        g.add_edge(u, v, r=r, x=10.0 * r)
    res = [2, 3]
    assert (feeder_reactances(g, res) == 10.0 * feeder_arrays(g, res)[1]).all()
    del g.edges[1, 4]["x"]
    assert feeder_reactances(g, res) is None
