"""revs_net_across / revs_net_across_scratch (include/revs_admm_ops.h) are declared, exported and bound, the record has
the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
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
    assert re.search(r"\bint revs_net_across\s*\(", ops) and re.search(r"\bint64_t revs_net_across_scratch\s*\(", ops)
    for name in ("revs_net_across", "revs_net_across_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_across"][1]) == 17
    assert "across_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.ACROSS_MAX_BANDS == 8 and "#define REVS_ACROSS_MAX_BANDS 8" in ops


def test_record_layout():
    from revs_admm_amd._lib import ACROSS_DTYPE
    assert ACROSS_DTYPE.itemsize == 96
    want = dict(min=0, q1=8, median=16, q3=24, max=32, mean=40, count=48, n_nan=52, n_violations=56, worst_scenario=60,
                band_count=64)
    assert {k: ACROSS_DTYPE.fields[k][1] for k in ACROSS_DTYPE.names} == want
    assert ACROSS_DTYPE["band_count"].shape == (8,) and ACROSS_DTYPE["band_count"].base == np.dtype("<i4")
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} revs_net_across_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for part in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in part.split(",")]
    assert fields == ["min", "q1", "median", "q3", "max", "mean", "count", "n_nan", "n_violations", "worst_scenario",
                      "band_count[8]"]


def test_scratch_size(lib):
    assert lib.revs_net_across_scratch(5, 1696) == 8 * 5 * 1696
    assert lib.revs_net_across_scratch(4096, 65535) == 8 * 4096 * 65535
    for bad in ((0, 8), (4097, 8), (-1, 8), (1, 0), (1, 65536), (1, -4)):
        assert lib.revs_net_across_scratch(*bad) == 0, bad


def _across(lib, S=2, n_out=8, T=24, values=64, keep=None, group=(0, 0), G=1, lo=0.95, hi=1.05, sense=-1, band=(0.95,),
            slot=96, daily=None, exposure=None, scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch; group and band are HOST arrays)
    hg = None if group is None else np.asarray(group, np.int32)
    hb = None if band is None else np.asarray(band, np.float64)
    return lib.revs_net_across(S, n_out, T, values, keep, None if hg is None else hg.ctypes.data, G, lo, hi, sense,
                               None if hb is None else hb.ctypes.data, 0 if hb is None else len(hb), slot, daily,
                               exposure, scratch, None)


def test_net_across_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    inf, nan = float("inf"), float("nan")
    for S in (0, -3, 4097):
        assert _across(lib, S=S) == -1 and f"revs_net_across: S={S}".encode() in err()
    for T in (0, 193):
        assert _across(lib, T=T) == -1 and f"T={T}".encode() in err()
    for n in (0, -1, 65536):
        assert _across(lib, n_out=n) == -1 and f"n_out={n}".encode() in err()
    assert _across(lib, S=4096, n_out=32768, T=16, group=(0,) * 4096) == -1 and b"S*n_out*T" in err()     # 2^31 exactly
    assert _across(lib, S=4096, n_out=65535, T=192, group=(0,) * 4096) == -1 and b"2^31" in err()
    for G in (0, -1, 3):
        assert _across(lib, G=G) == -1 and f"G={G}".encode() in err()
    assert _across(lib, group=None) == -1 and b"group is NULL" in err()
    assert _across(lib, group=(0, 1)) == -1 and b"group[1]=1" in err()
    assert _across(lib, group=(-2, 0)) == -1 and b"group[0]=-2" in err()
    assert _across(lib, band=(0.9,) * 9) == -1 and b"B=9" in err()
    for bad in (nan, inf, -inf):
        assert _across(lib, band=(0.92, bad)) == -1 and b"band[1] is not finite" in err()
    for sense in (0, 2, -2):
        assert _across(lib, sense=sense) == -1 and f"sense={sense}".encode() in err()
    assert _across(lib, lo=1.06) == -1 and b"lo > hi" in err()
    assert _across(lib, lo=nan) == -1 and b"lo > hi" in err()
    assert _across(lib, hi=nan) == -1 and b"lo > hi" in err()
    assert _across(lib, values=None) == -1 and b"values" in err()
    assert _across(lib, slot=None) == -1 and b"every output is NULL" in err()
    assert _across(lib, daily=96) == -1 and b"need scratch" in err()
    assert _across(lib, slot=None, exposure=32) == -1 and b"need scratch" in err()
    assert _across(lib, daily=96, scratch=136) == -1 and b"16-byte aligned" in err()
    assert _across(lib, slot=None, exposure=32, scratch=8) == -1 and b"16-byte aligned" in err()


def test_band_needs_its_array(lib):
    """B > 0 with band NULL cannot be said through _across (B is the array's length): the call itself."""
    g = np.zeros(2, np.int32)
    assert lib.revs_net_across(2, 8, 24, 64, None, g.ctypes.data, 1, 0.95, 1.05, -1, None, 2, 96, None, None, None,
                               None) == -1
    assert b"band is NULL" in lib.revs_last_error()


def test_across_report_device_checks_its_arguments():
    import torch
    from revs_admm_amd.study import across_report_device, study_report
    v = torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="contiguous"):
        across_report_device(v.float(), None, [0, 0])
    with pytest.raises(ValueError, match="contiguous"):
        across_report_device(v.transpose(1, 2), None, [0, 0])
    with pytest.raises(ValueError, match="differ in shape"):
        across_report_device(v, torch.zeros(2, 3, 5, dtype=torch.float64), [0, 0])
    with pytest.raises(ValueError, match="need groups"):
        across_report_device(v, None, None)
    with pytest.raises(ValueError, match="no scenario is in a group"):
        across_report_device(v, None, [-1, -1])
    with pytest.raises(ValueError, match="integers >= -1"):
        across_report_device(v, None, [0])
    with pytest.raises(ValueError, match="finite bands"):
        across_report_device(v, None, [0, 0], bands=(0.9,) * 9)
    with pytest.raises(ValueError, match="finite bands"):
        across_report_device(v, None, [0, 0], loading_bands=(np.inf,))
    with pytest.raises(ValueError, match="one entry per node"):
        across_report_device(v, v, [0, 0], rated=np.ones(4))
    par, er, cons = np.array([-1, 0]), np.ones(2), np.arange(2)
    with pytest.raises(ValueError, match="across=True.*pass groups"):
        study_report(par, er, cons, np.zeros((2, 2, 3)), across=True)
