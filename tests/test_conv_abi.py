"""revs_conv_report / revs_conv_report_scratch (include/revs_admm_ops.h) are declared, exported and bound, the records
have the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("revs_conv_report", "revs_conv_report_scratch")


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib, build
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_conv_report\s*\(", ops) and re.search(r"\bint64_t revs_conv_report_scratch\s*\(", ops)
    for name in NAMES:
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_conv_report"][1]) == 18 and len(_lib.SIGNATURES["revs_conv_report_scratch"][1]) == 4
    assert "convergence_kernels.hip" in build.SOURCES


def test_record_layouts():
    from revs_admm_amd._lib import CONV_RES_DTYPE, CONV_RUN_DTYPE
    assert CONV_RES_DTYPE.itemsize == 24 and CONV_RUN_DTYPE.itemsize == 16
    assert {k: CONV_RES_DTYPE.fields[k][1] for k in CONV_RES_DTYPE.names} == dict(
        max=0, last=4, settle=8, n_above=12, worst_iteration=16, reserved=20)
    assert {k: CONV_RUN_DTYPE.fields[k][1] for k in CONV_RUN_DTYPE.names} == dict(
        converged_at=0, last_above=4, n_unsettled=8, n_never=12)
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    for name, dt in (("revs_conv_res_t", CONV_RES_DTYPE), ("revs_conv_run_t", CONV_RUN_DTYPE)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for part in re.findall(r"(?:float|int32_t)\s+([^;]+);", body) for f in part.split(",")]
        assert fields == list(dt.names)


def test_scratch_size(lib):
    f = lib.revs_conv_report_scratch
    base = f(3, 100, 40, 2)
    assert base > 0 and base % 16 == 0 and base >= 4 * 3 * 41 + 8 * 3
    # monotone (never smaller) in every size
    assert f(4, 100, 40, 2) >= base and f(3, 101, 40, 2) >= base and f(3, 100, 41, 2) >= base and f(3, 100, 40, 3) >= base
    assert f(4096, 1, 1, 0) > f(1, 1, 1, 0) > 0 and f(1, 1, 5000, 0) > f(1, 1, 1, 0)
    assert f(4096, 524287, 500, 4096) > 0
    for bad in ((0, 8, 4, 0), (4097, 8, 4, 0), (-1, 8, 4, 0), (1, 0, 4, 0), (1, -4, 4, 0), (1, 8, 0, 0), (1, 8, -2, 0),
                (1, 8, 4, -1), (1, 8, 4, 4097), (4096, 524288, 4, 0), (1, 2 ** 31, 4, 0), (2, 2 ** 62, 4, 0)):
        assert f(*bad) <= 0, bad


def _report(lib, S=2, n=8, K=5, hist=64, ld=None, keep=None, index=None, groups=(0, -1), G=1, eps=0.5, patience=8,
            iter_rec=256, pool_rec=512, res_rec=None, run_rec=None, settle_rec=None, scratch=1024):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    hg = None if groups is None else np.asarray(groups, np.int32)
    return lib.revs_conv_report(S, n, K, hist, n * S if ld is None else ld, keep, index,
                                None if hg is None else hg.ctypes.data, G, eps, patience, iter_rec, pool_rec, res_rec,
                                run_rec, settle_rec, scratch, None)


def test_conv_report_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for S in (0, -3, 4097):
        assert _report(lib, S=S, groups=None, G=0) == -1 and f"revs_conv_report: S={S}".encode() in err()
    for n in (0, -1):
        assert _report(lib, n=n) == -1 and f"n={n}".encode() in err()
    for K in (0, -1):
        assert _report(lib, K=K) == -1 and f"K={K}".encode() in err()
    assert _report(lib, n=2 ** 30) == -1 and b"2^31" in err()           # S n = 2^31 exactly
    assert _report(lib, S=1, n=2 ** 40, groups=(0,)) == -1 and b"2^31" in err()
    assert _report(lib, ld=15) == -1 and b"ld=15" in err()
    assert _report(lib, ld=0) == -1 and b"ld=0" in err()
    for p in (0, -8):
        assert _report(lib, patience=p) == -1 and f"patience={p}".encode() in err()
    assert _report(lib, eps=-1e-30) == -1 and b"eps=" in err()
    assert _report(lib, eps=float("nan")) == -1 and b"eps=" in err()
    assert _report(lib, hist=None) == -1 and b"argument hist" in err()
    assert _report(lib, iter_rec=None) == -1 and b"argument iter_rec" in err()
    assert _report(lib, scratch=None) == -1 and b"argument scratch" in err()
    assert _report(lib, scratch=1032) == -1 and b"16-byte aligned" in err()
    for G in (-1, 4097):
        assert _report(lib, G=G) == -1 and f"G={G}".encode() in err()
    assert _report(lib, groups=None) == -1 and b"groups is NULL" in err()
    assert _report(lib, pool_rec=None) == -1 and b"pool_rec is NULL" in err()
    assert _report(lib, groups=(0, 1)) == -1 and b"groups[1]=1" in err()
    assert _report(lib, groups=(-2, 0)) == -1 and b"groups[0]=-2" in err()
