"""revs_net_losses / revs_net_losses_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records have
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
    assert re.search(r"\bint revs_net_losses\s*\(", ops) and re.search(r"\bint64_t revs_net_losses_scratch\s*\(", ops)
    for name in ("revs_net_losses", "revs_net_losses_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_losses"][1]) == 25
    decl = re.search(r"\bint revs_net_losses\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == 25
    assert "losses_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    out = []
    for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body):
        out += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    return out


def test_record_layouts():
    from revs_admm_amd._lib import LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    off = lambda dt: {k: dt.fields[k][1] for k in dt.names}
    assert LOSS_SLOT_DTYPE.itemsize == 64 and "} revs_loss_slot_t;                   /* 64 bytes */" in hdr
    assert off(LOSS_SLOT_DTYPE) == dict(total=0, delivered=8, class_total=16, mlf_max=48, mlf_max_index=56, n_bad=60)
    assert _fields(hdr, "revs_loss_slot_t") == list(LOSS_SLOT_DTYPE.names)
    assert LOSS_LINE_DAY_DTYPE.itemsize == 24 and "} revs_loss_line_day_t;               /* 24 bytes */" in hdr
    assert off(LOSS_LINE_DAY_DTYPE) == dict(energy=0, peak=8, peak_slot=16, reserved=20)
    assert _fields(hdr, "revs_loss_line_day_t") == list(LOSS_LINE_DAY_DTYPE.names)
    assert LOSS_DAY_DTYPE.itemsize == 192 and "} revs_loss_day_t;                    /* 192 bytes */" in hdr
    assert off(LOSS_DAY_DTYPE) == dict(energy=0, delivered=8, class_energy=16, cost=48, peak=56, top_energy=64, top_index=128,
                                       peak_slot=160, n_bad_slots=164, reserved=168)
    assert _fields(hdr, "revs_loss_day_t") == list(LOSS_DAY_DTYPE.names)
    assert LOSS_SLOT_DTYPE["class_total"].shape == (4,) and LOSS_DAY_DTYPE["top_index"].shape == (8,)


def test_scratch_size(lib):
    size = lambda S, T, n: 8 * S * T * n + 64 * S * T + 8 * S * n
    assert lib.revs_net_losses_scratch(5, 24, 1696) == size(5, 24, 1696)
    assert lib.revs_net_losses_scratch(4096, 192, 16384) == size(4096, 192, 16384)
    assert lib.revs_net_losses_scratch(1, 1, 8) % 16 == 0
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_net_losses_scratch(*bad) == 0, bad


def _call(lib, S=2, m=8, T=24, tree=(8, 64, 64), node_g=64, lmask=None, nmask=None, cls=None, C_=0, nop=None, n_out=8,
          vset2=1.0, hours=1.0, loss_max=float("inf"), cost=None, loss=64, mlf=None, drop=None, flow=None, summary=None,
          slot=None, line_day=None, day=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import Tree
    tr = None if tree is None else C.byref(Tree(*tree))
    return lib.revs_net_losses(S, m, T, tr, node_g, lmask, nmask, cls, C_, nop, n_out, vset2, hours, loss_max, cost, loss,
                               mlf, drop, flow, summary, slot, line_day, day, scratch, None)


def test_net_losses_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    # every case revs_net_headroom refuses for S, m, T, the tree and n_out
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_net_losses: S={S}".encode() in err()
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
    # the scalars: finite and > 0; loss_max may be +inf
    for bad in (nan, inf, -inf, 0.0, -1.0):
        assert _call(lib, vset2=bad) == -1 and b"vset2 must be finite and > 0" in err()
        assert _call(lib, hours=bad) == -1 and b"slot_hours must be finite and > 0" in err()
    for bad in (nan, -inf, 0.0, -1.0):
        assert _call(lib, loss_max=bad) == -1 and b"loss_max must be > 0" in err()
    # the classes
    for c in (-1, 5):
        assert _call(lib, C_=c, cls=64) == -1 and f"C={c}".encode() in err()
    assert _call(lib, C_=2) == -1 and b"line_class is NULL" in err()
    # outputs and their scratch
    assert _call(lib, loss=None) == -1 and b"every output is NULL" in err()
    for kw in (dict(summary=96), dict(line_day=24), dict(day=192), dict(loss=None, day=192)):
        assert _call(lib, **kw) == -1 and b"need scratch" in err()
        assert _call(lib, scratch=24, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.losses import loss_report_device, native_losses_device
    g = torch.zeros(2, 3, 4, dtype=torch.float64)
    feeder = (np.array([-1, 0, 1]), np.ones(3), np.arange(3))
    with pytest.raises(ValueError, match="contiguous"):
        loss_report_device(g.float(), feeder=feeder)
    with pytest.raises(ValueError, match="contiguous"):
        loss_report_device(g.transpose(1, 2), feeder=feeder)
    with pytest.raises(ValueError, match="either as feeder"):
        loss_report_device(g)
    with pytest.raises(ValueError, match="either as feeder"):
        loss_report_device(g, feeder=feeder, tree=(None, None, 3))
    for kw, msg in ((dict(vset=0.0), "vset"), (dict(slot_hours=-1.0), "slot_hours"), (dict(loss_max=float("nan")), "loss_max")):
        with pytest.raises(ValueError, match=msg):
            native_losses_device(None, g.device, None, None, None, 3, g, **kw)


def test_position_builders_of_the_loss_report():
    """losses._position_bytes is tree_reports.position_mask with none="no array" and the length check of a boolean mask;
    losses._position_classes refuses a class of 4 or more, and a wrong length, before tree_reports.position_classes."""
    import torch
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.losses import _position_bytes, _position_classes
    parent = np.array([-1, 0, 1, 1, 0])
    th = feeder_tree(parent, np.ones(5), np.array([-1, 0, -1, 1, 2]), np.ones(3, bool))
    order = np.asarray(th["order"])
    real = order < 5
    dev = torch.device("cpu")
    assert _position_bytes(dev, th, 5, None, "lines") is None
    assert (_position_bytes(dev, th, 5, [1, 4], "lines").numpy() == (real & np.isin(order, [1, 4]))).all()
    with pytest.raises(ValueError, match=r"loss report: a boolean nodes mask must have one entry per tree node \(5\)"):
        _position_bytes(dev, th, 5, np.ones(4, bool), "nodes")
    assert _position_classes(dev, th, 5, None) == (None, 0)
    cls = np.array([0, 2, -1, 1, -7])
    by_pos, n_cls = _position_classes(dev, th, 5, cls)
    assert n_cls == 3 and (by_pos.numpy() == np.where(real, np.where(cls < 0, 255, cls)[np.where(real, order, 0)], 255)).all()
    assert _position_classes(dev, th, 5, np.full(5, -1))[1] == 0
    for bad in (np.array([0, 1, 2, 3, 4]), np.zeros(4, int)):
        with pytest.raises(ValueError, match=r"loss report: classes must hold one class below 4 \(or -1\) per tree node \(5\)"):
            _position_classes(dev, th, 5, bad)
