"""revs_bill_rows / revs_bill_study / revs_bill_study_scratch (include/revs_admm_ops.h) are declared, exported and bound,
the record has the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("revs_bill_rows", "revs_bill_study", "revs_bill_study_scratch")


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_bill_rows\s*\(", ops) and re.search(r"\bint revs_bill_study\s*\(", ops)
    assert re.search(r"\bint64_t revs_bill_study_scratch\s*\(", ops)
    for name in NAMES:
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_bill_rows"][1]) == 10 and len(_lib.SIGNATURES["revs_bill_study"][1]) == 13
    from revs_admm_amd import build
    assert "bill_kernels.hip" in build.SOURCES


def test_record_layout():
    from revs_admm_amd._lib import BILL_DTYPE
    assert BILL_DTYPE.itemsize == 96
    want = dict(min=0, q1=8, median=16, q3=24, max=32, whisker_lo=40, whisker_hi=48, total=56, reserved0=64, count=72,
                n_nan=76, n_fliers=80, n_above=84, worst_index=88, worst_scenario=92)
    assert {k: BILL_DTYPE.fields[k][1] for k in BILL_DTYPE.names} == want
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} revs_bill_summary_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for part in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in part.split(",")]
    assert fields == list(BILL_DTYPE.names)


def test_scratch_size(lib):
    assert lib.revs_bill_study_scratch(5, 1126) == 8 * 5 * 1126
    assert lib.revs_bill_study_scratch(2, 70000) == 8 * 2 * 70000
    assert lib.revs_bill_study_scratch(4096, 524287) == 8 * 4096 * 524287
    for bad in ((0, 8), (4097, 8), (-1, 8), (1, 0), (1, -4), (4096, 524288), (1, 2 ** 31), (2, 2 ** 62)):
        assert lib.revs_bill_study_scratch(*bad) == 0, bad


def _rows(lib, S=2, n=8, T=24, g=64, f64=0, stride_s=None, stride_i=None, tariff=128, bill=256):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    stride_s = n * T if stride_s is None else stride_s
    stride_i = T if stride_i is None else stride_i
    return lib.revs_bill_rows(S, n, T, g, f64, stride_s, stride_i, tariff, bill, None)


def test_bill_rows_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for S in (0, -3, 4097):
        assert _rows(lib, S=S) == -1 and f"revs_bill_rows: S={S}".encode() in err()
    for T in (0, -1, 193):
        assert _rows(lib, T=T) == -1 and f"T={T}".encode() in err()
    for n in (0, -1):
        assert _rows(lib, n=n) == -1 and f"n={n}".encode() in err()
    assert _rows(lib, S=2, n=2 ** 30) == -1 and b"2^31" in err()       # 2^31 exactly
    assert _rows(lib, S=1, n=2 ** 40) == -1 and b"2^31" in err()
    assert _rows(lib, S=4096, n=2 ** 52) == -1 and b"2^31" in err()
    assert _rows(lib, g=None) == -1 and b"argument g" in err()
    assert _rows(lib, tariff=None) == -1 and b"tariff" in err()
    assert _rows(lib, bill=None) == -1 and b"argument bill" in err()
    for f in (2, -1):
        assert _rows(lib, f64=f) == -1 and f"g_f64={f}".encode() in err()
    # strides: (stride_s, stride_i) for S = 2, n = 8, T = 24
    for ss, si in ((191, 24), (192, 23), (24, 47), (23, 48), (0, 24), (24, 0), (-192, 24), (192, -24), (100, 30),
                   (2 ** 62, 2 ** 61)):
        assert _rows(lib, stride_s=ss, stride_i=si) == -1 and b"rows overlap" in err(), (ss, si)


def _study(lib, S=2, n=8, bill=64, base=(-1, 0), keep=None, ior=None, group=(0, 0), G=1, dev=128, summary=256, pooled=512,
           scratch=1024):
    hb = None if base is None else np.asarray(base, np.int32)
    hg = None if group is None else np.asarray(group, np.int32)
    return lib.revs_bill_study(S, n, bill, None if hb is None else hb.ctypes.data, keep, ior,
                               None if hg is None else hg.ctypes.data, G, dev, summary, pooled, scratch, None)


def test_bill_study_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for S in (0, -3, 4097):
        assert _study(lib, S=S) == -1 and f"revs_bill_study: S={S}".encode() in err()
    for n in (0, -1):
        assert _study(lib, n=n) == -1 and f"n={n}".encode() in err()
    assert _study(lib, n=2 ** 30) == -1 and b"2^31" in err()
    assert _study(lib, bill=None) == -1 and b"bill" in err()
    assert _study(lib, base=None) == -1 and b"base is NULL" in err()
    assert _study(lib, base=(-2, 0)) == -1 and b"base[0]=-2" in err()
    assert _study(lib, base=(0, 2)) == -1 and b"base[1]=2" in err()
    for G in (-1, 3):
        assert _study(lib, G=G) == -1 and f"G={G}".encode() in err()
    assert _study(lib, group=None) == -1 and b"group is NULL" in err()
    assert _study(lib, group=(0, 1)) == -1 and b"group[1]=1" in err()
    assert _study(lib, group=(-2, 0)) == -1 and b"group[0]=-2" in err()
    assert _study(lib, G=0, group=None) == -1 and b"pooled_out with G == 0" in err()
    assert _study(lib, scratch=None) == -1 and b"need scratch" in err()
    assert _study(lib, pooled=None, scratch=None) == -1 and b"need scratch" in err()
    assert _study(lib, summary=None, scratch=None) == -1 and b"need scratch" in err()
    assert _study(lib, scratch=1032) == -1 and b"16-byte aligned" in err()
    assert _study(lib, dev=None, summary=None, pooled=None) == -1 and b"every output is NULL" in err()
