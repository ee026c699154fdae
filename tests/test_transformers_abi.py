"""revs_xf_report / revs_xf_report_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records have
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
    assert re.search(r"\bint revs_xf_report\s*\(", ops) and re.search(r"\bint64_t revs_xf_report_scratch\s*\(", ops)
    for name in ("revs_xf_report", "revs_xf_report_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_xf_report"][1]) == 31
    decl = re.search(r"\bint revs_xf_report\s*\(([^;]*)\);", ops).group(1)
    assert len(decl.split(",")) == 31
    assert "transformer_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES


def _fields(hdr, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1), flags=re.S)
    out = []
    for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body):
        out += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    return out


def test_record_layouts():
    from revs_admm_amd._lib import XF_DAY_DTYPE, XF_FLEET_DTYPE, XfModel
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    off = lambda dt: {k: dt.fields[k][1] for k in dt.names}
    assert XF_DAY_DTYPE.itemsize == 64 and "} revs_xf_day_t;                      /* 64 bytes */" in hdr
    assert off(XF_DAY_DTYPE) == dict(peak_ratio=0, peak_hot=8, energy_kwh=16, age_hours=24, lol_percent=32, feqa=40,
                                     peak_ratio_slot=48, peak_hot_slot=52, n_over_slots=56, n_hot_slots=60)
    assert _fields(hdr, "revs_xf_day_t") == list(XF_DAY_DTYPE.names)
    assert XF_FLEET_DTYPE.itemsize == 160 and XF_FLEET_DTYPE.itemsize % 16 == 0
    assert "} revs_xf_fleet_t;                    /* 160 bytes */" in hdr
    assert off(XF_FLEET_DTYPE) == dict(lol_sum=0, lol_max=8, energy_kwh=16, feqa_mean=24, top_lol=32, top_index=96, n_xf=128,
                                       n_nan=132, n_overloaded=136, n_hot=140, n_aging=144, reserved=148)
    assert _fields(hdr, "revs_xf_fleet_t") == list(XF_FLEET_DTYPE.names)
    assert XF_FLEET_DTYPE["top_index"].shape == (8,) and XF_FLEET_DTYPE["top_lol"].shape == (8,)
    assert C.sizeof(XfModel) == 64 and "} revs_xf_model_t;                    /* 64 bytes */" in hdr
    assert _fields(hdr, "revs_xf_model_t") == [k for k, _ in XfModel._fields_]
    assert [getattr(XfModel, k).offset for k, _ in XfModel._fields_] == list(range(0, 64, 8))


def test_scratch_size(lib):
    size = lambda S, T, K: 16 * S * T * K + 64 * S * K
    assert lib.revs_xf_report_scratch(5, 24, 462) == size(5, 24, 462)
    assert lib.revs_xf_report_scratch(4096, 192, 65535) == size(4096, 192, 65535)
    assert lib.revs_xf_report_scratch(1, 1, 1) % 16 == 0
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 65536), (-1, 24, 8), (1, 24, -8)):
        assert lib.revs_xf_report_scratch(*bad) == 0, bad


GOOD_MODEL = dict(dto_r=55.0, dhs_r=25.0, loss_ratio=5.0, n=0.8, m=0.8, aging_B=15000.0, theta_ref=110.0,
                  normal_life_hours=180000.0)


def _call(lib, S=2, m=8, T=24, K=3, nnz=6, node_g=64, xf_ptr=64, xf_rows=64, rated=64, ambient=64, model=GOOD_MODEL,
          hours=1.0, q=1, decay_to=0.7, decay_w=0.0, cyclic=1, to0=0.0, w0=0.0, over=1.0, hot_limit=110.0, load=64,
          ratio=None, top_oil=None, hot=None, faa=None, sum_ratio=None, sum_hot=None, day=None, fleet=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd._lib import XfModel
    mdl = None if model is None else C.byref(XfModel(*[model[k] for k, _ in XfModel._fields_]))
    return lib.revs_xf_report(S, m, T, K, nnz, node_g, xf_ptr, xf_rows, rated, ambient, mdl, hours, q, decay_to, decay_w,
                              cyclic, to0, w0, over, hot_limit, load, ratio, top_oil, hot, faa, sum_ratio, sum_hot, day,
                              fleet, scratch, None)


def test_xf_report_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_xf_report: S={S}".encode() in err()
    for T in (0, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    for m in (0, 65536):
        assert _call(lib, m=m, nnz=0) == -1 and f"m={m}".encode() in err()
    for K in (0, 65536, -1):
        assert _call(lib, K=K) == -1 and f"K={K}".encode() in err()
    for nnz in (-1, 9):
        assert _call(lib, nnz=nnz) == -1 and f"nnz={nnz}".encode() in err()
    # the required pointers; xf_rows only with members
    for kw in ("node_g", "xf_ptr", "rated", "ambient", "model"):
        assert _call(lib, **{kw: None}) == -1 and b"null pointer argument" in err(), kw
    assert _call(lib, xf_rows=None) == -1 and b"xf_rows" in err()
    # the model: finite, and positive where it must be (theta_ref: above -273)
    for k in GOOD_MODEL:
        for bad in (nan, inf, -inf) + ((-273.0,) if k == "theta_ref" else (0.0, -1.0)):
            assert _call(lib, model=dict(GOOD_MODEL, **{k: bad})) == -1 and f"model {k} must be".encode() in err(), (k, bad)
    assert _call(lib, model=dict(GOOD_MODEL, theta_ref=-20.0), scratch=None, load=None) == -1 and b"every output is NULL" in err()
    # the scalars
    for bad in (nan, inf, -inf, 0.0, -1.0):
        assert _call(lib, hours=bad) == -1 and b"slot_hours must be finite and > 0" in err()
    for q in (0, 17, -1):
        assert _call(lib, q=q) == -1 and f"substeps={q}".encode() in err()
    for bad in (nan, 1.0, -1e-9, inf):
        assert _call(lib, decay_to=bad) == -1 and b"decay_to outside [0, 1)" in err()
        assert _call(lib, decay_w=bad) == -1 and b"decay_w outside [0, 1)" in err()
    for c in (-1, 2):
        assert _call(lib, cyclic=c) == -1 and f"cyclic={c}".encode() in err()
    for bad in (nan, inf):
        assert _call(lib, cyclic=0, to0=bad) == -1 and b"to0 and w0 must be finite" in err()
        assert _call(lib, cyclic=0, w0=bad) == -1 and b"to0 and w0 must be finite" in err()
    assert _call(lib, over=nan) == -1 and b"no NaN" in err()
    assert _call(lib, hot_limit=nan) == -1 and b"no NaN" in err()
    # outputs and their scratch
    assert _call(lib, load=None) == -1 and b"every output is NULL" in err()
    for kw in (dict(sum_ratio=96), dict(sum_hot=96), dict(fleet=160), dict(load=None, fleet=160)):
        assert _call(lib, **kw) == -1 and b"need scratch" in err()
        assert _call(lib, scratch=24, **kw) == -1 and b"16-byte aligned" in err()


def test_python_entry_checks_its_arguments():
    import torch
    from revs_admm_amd.transformers import ThermalModel, native_transformers_device, transformer_report_device
    g = torch.zeros(2, 6, 4, dtype=torch.float64)
    xf_of, kva = np.array([0, 0, 1, -1, 2, 2]), np.array([10.0, 10.0, 25.0])
    with pytest.raises(ValueError, match="contiguous"):
        transformer_report_device(g.float(), xf_of, kva)
    with pytest.raises(ValueError, match="contiguous"):
        transformer_report_device(g.transpose(1, 2), xf_of, kva)
    with pytest.raises(ValueError, match="one integer per row"):
        transformer_report_device(g, xf_of[:5], kva)
    with pytest.raises(ValueError, match="one integer per row"):
        transformer_report_device(g, xf_of.astype(np.float64), kva)
    with pytest.raises(ValueError, match="xf_of outside"):
        transformer_report_device(g, np.array([0, 0, 1, -1, 2, 3]), kva)
    with pytest.raises(ValueError, match="xf_of outside"):
        transformer_report_device(g, np.array([0, 0, 1, -2, 2, 2]), kva)
    with pytest.raises(ValueError, match="pf must lie"):
        transformer_report_device(g, xf_of, kva, pf=0.0)
    ptr_, rows = np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 2, 4, 5], np.int32)
    call = lambda **kw: native_transformers_device(None, g.device, None, g, ptr_, rows, kva, np.full(4, 30.0), **kw)
    for kw, msg in ((dict(slot_hours=-1.0), "slot_hours"), (dict(substeps=0), "substeps"), (dict(substeps=17), "substeps"),
                    (dict(initial="warm"), "initial"), (dict(initial=(float("nan"), 0.0)), "initial"),
                    (dict(over_ratio=float("nan")), "no NaN"), (dict(model=ThermalModel(n=0.0)), "model n"),
                    (dict(model=ThermalModel(tau_to=0.0)), "tau_to"), (dict(model=ThermalModel(tau_w=-1.0)), "tau_w"),
                    (dict(out=torch.zeros(2, 3, 5, dtype=torch.float64)), "out must be")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="ambient"):
        native_transformers_device(None, g.device, None, g, ptr_, rows, kva, np.full(3, 30.0))
    with pytest.raises(ValueError, match="one rating per transformer"):
        native_transformers_device(None, g.device, None, g, ptr_, rows, kva[:2], np.full(4, 30.0))
