"""revs_net_study / revs_net_study_scratch (include/revs_admm_ops.h) are declared, exported and bound, the pooled
record has the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
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
    assert re.search(r"\bint revs_net_study\s*\(", ops) and re.search(r"\bint64_t revs_net_study_scratch\s*\(", ops)
    for name in ("revs_net_study", "revs_net_study_scratch"):
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_net_study"][1]) == 24
    assert "network_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES
    assert (_lib.STUDY_MAX_S, _lib.STUDY_MAX_BANDS) == (4096, 8)
    assert "#define REVS_STUDY_MAX_S 4096" in ops and "#define REVS_STUDY_MAX_BANDS 8" in ops


def test_pooled_record_layout():
    """revs_net_pooled_t: revs_net_summary_t's fields with worst_scenario in place of the first reserved word."""
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.study import POOLED_DTYPE
    assert POOLED_DTYPE.itemsize == 96
    for k in SUMMARY_DTYPE.names[:-1]:
        assert POOLED_DTYPE.fields[k][:2] == SUMMARY_DTYPE.fields[k][:2], k
    assert POOLED_DTYPE.fields["worst_scenario"][1] == SUMMARY_DTYPE.fields["reserved"][1] == 84
    assert POOLED_DTYPE.fields["reserved"][1] == 88
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} revs_net_pooled_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for part in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in part.split(",")]
    assert fields == ["min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi", "worst_value", "count", "n_fliers",
                      "n_violations", "n_nan", "worst_index", "worst_scenario", "reserved[2]"]


def test_scratch_size(lib):
    assert lib.revs_net_study_scratch(5, 24, 1696) == 2 * 5 * 24 * 1696 * 8
    assert lib.revs_net_study_scratch(64, 96, 16384) == 2 * 64 * 96 * 16384 * 8 == 1610612736
    assert lib.revs_net_study_scratch(4096, 192, 16384) == 2 * 4096 * 192 * 16384 * 8      # (beyond 32 bits)
    for bad in ((0, 24, 8), (4097, 24, 8), (1, 0, 8), (1, 193, 8), (1, 24, 0), (1, 24, 16385), (-1, 24, 8)):
        assert lib.revs_net_study_scratch(*bad) == 0, bad


def _study(lib, S=2, m=4, T=24, n=8, tree=True, pack=16, w=16, node_g=32, n_out=8, vset=1.0, vmin=0.95, vmax=1.05,
           group=(0, 0), G=1, band=(0.95,), flow=None, loading=None, volt=None, summary=64, pooled=None, counts=None,
           scratch=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch; group and band are HOST arrays)
    from revs_admm_amd import _lib
    tr = C.byref(_lib.Tree(n, pack, w)) if tree else None
    hg = None if group is None else np.asarray(group, np.int32)
    hb = None if band is None else np.asarray(band, np.float64)
    B = 0 if hb is None else len(hb)
    return lib.revs_net_study(S, m, T, tr, node_g, 48, None, None, n_out, vset, vmin, vmax,
                              None if hg is None else hg.ctypes.data, G, None if hb is None else hb.ctypes.data, B,
                              flow, loading, volt, summary, pooled, counts, scratch, None)


def test_net_study_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for S in (0, -3, 4097):
        assert _study(lib, S=S, group=None, G=0) == -1 and f"S={S}".encode() in err()
    assert _study(lib, G=3) == -1 and b"G=3" in err()
    assert _study(lib, G=-1) == -1 and b"G=-1" in err()
    assert _study(lib, band=(0.9,) * 9) == -1 and b"B=9" in err()
    assert _study(lib, group=(0, 1), G=1) == -1 and b"group[1]=1" in err()
    assert _study(lib, group=(-2, 0), G=1) == -1 and b"group[0]=-2" in err()
    assert _study(lib, group=None, G=1) == -1 and b"group is NULL" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _study(lib, band=(0.92, bad)) == -1 and b"band[1] is not finite" in err()
    assert _study(lib, summary=None) == -1 and b"every output is NULL" in err()
    assert _study(lib, summary=None, counts=80, band=None) == -1 and b"every output is NULL" in err()    # (counts of no band)
    assert _study(lib, pooled=96) == -1 and b"pooled_out needs scratch" in err()
    assert _study(lib, pooled=96, scratch=128, group=None, G=0) == -1 and b"pooled_out with G == 0" in err()
    assert _study(lib, pooled=96, scratch=136) == -1 and b"16-byte aligned" in err()
    # every check revs_net_report makes, under this entry point's name
    for T in (0, 193):
        assert _study(lib, T=T) == -1 and f"revs_net_study: T={T}".encode() in err()
    assert _study(lib, m=0) == -1 and b"m=0" in err()
    assert _study(lib, node_g=None) == -1 and b"null pointer" in err()
    assert _study(lib, tree=False) == -1 and _study(lib, pack=None) == -1 and _study(lib, w=None) == -1
    assert _study(lib, n=16392) == -1 and b"16384" in err()
    assert _study(lib, n=12) == -1 and b"multiple of 8" in err()
    assert _study(lib, n_out=0) == -1 and _study(lib, n_out=9) == -1 and b"n_out" in err()
    assert _study(lib, vmin=1.06) == -1 and b"vmin > vmax" in err()
    assert _study(lib, vset=float("nan")) == -1 and b"vset" in err()


def test_study_report_checks_its_arguments():
    from revs_admm_amd.study import study_report
    par, er, cons = np.array([-1, 0]), np.ones(2), np.arange(2)
    with pytest.raises(ValueError, match="scenarios, rows, slots"):
        study_report(par, er, cons, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="finite bands"):
        study_report(par, er, cons, np.zeros((1, 2, 3)), bands=(0.9,) * 9)
    with pytest.raises(ValueError, match="finite bands"):
        study_report(par, er, cons, np.zeros((1, 2, 3)), bands=(np.nan,))
    with pytest.raises(ValueError, match="integers >= -1"):
        study_report(par, er, cons, np.zeros((2, 2, 3)), groups=[0])
    with pytest.raises(ValueError, match="integers >= -1"):
        study_report(par, er, cons, np.zeros((2, 2, 3)), groups=[0, -2])
