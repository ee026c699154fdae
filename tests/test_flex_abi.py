"""revs_flex_report / revs_flex_report_scratch / revs_flex_report_chunk (include/revs_admm_ops.h) are declared, exported
and bound, the three records have the documented layouts, and bad arguments are rejected on the host, before any launch
(no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("revs_flex_report", "revs_flex_report_scratch", "revs_flex_report_chunk")


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    import revs_admm_amd
    from revs_admm_amd import _lib, build, flexibility
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_flex_report\s*\(", ops) and re.search(r"\bint64_t revs_flex_report_scratch\s*\(", ops)
    assert re.search(r"\bint32_t revs_flex_report_chunk\s*\(", ops)
    for name in NAMES:
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_flex_report"][1]) == 22 and len(_lib.SIGNATURES["revs_flex_report_scratch"][1]) == 3
    assert "flex_kernels.hip" in build.SOURCES
    assert 1 <= lib.revs_flex_report_chunk() <= _lib.MAX_T
    for name in ("FlexReport", "flexibility_report", "flexibility_report_device", "FlexMixin"):
        assert hasattr(flexibility, name)
    assert "flexibility" in revs_admm_amd.__doc__
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    assert callable(AdmmEngine.flexibility_report) and callable(AdmmEnsemble.flexibility_report)
    import inspect
    from revs_admm_amd.revs_fixture import REVS
    from revs_admm_amd.study import StudyReport
    assert inspect.signature(REVS.study).parameters["flexibility"].default is False
    assert "flexibility" in StudyReport.__dataclass_fields__


def _header_fields(name):
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, part in re.findall(r"(double|float|int32_t)\s+([^;]+);", body):
        for f in part.split(","):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", f.strip())
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("name,size", [("revs_flex_row_t", 64), ("revs_flex_slot_t", 32), ("revs_flex_day_t", 64)])
def test_record_layouts(name, size):
    from revs_admm_amd import _lib
    D = {"revs_flex_row_t": _lib.FLEX_ROW_DTYPE, "revs_flex_slot_t": _lib.FLEX_SLOT_DTYPE,
         "revs_flex_day_t": _lib.FLEX_DAY_DTYPE}[name]
    assert D.itemsize == size
    kinds = {"double": np.dtype("<f8"), "float": np.dtype("<f4"), "int32_t": np.dtype("<i4")}
    fields = _header_fields(name)
    assert [f[0] for f in fields] == list(D.names)
    off = 0
    for fname, ctype, count in fields:                       # packed in the header's order, every field aligned
        base = D.fields[fname][0].base
        assert base == kinds[ctype] and D.fields[fname][1] == off and off % base.itemsize == 0, fname
        assert D.fields[fname][0].itemsize == count * base.itemsize
        off += count * base.itemsize
    assert off == size
    want = {"revs_flex_row_t": ["up_energy", "down_energy", "laxity", "energy", "ready", "slack", "n_up", "n_down", "flags",
                                "reserved"],
            "revs_flex_slot_t": ["n_plugged", "n_up", "n_down", "reserved", "up", "down"],
            "revs_flex_day_t": ["up_energy", "down_energy", "peak_up", "peak_down", "peak_up_slot", "peak_down_slot", "n_ev",
                                "n_never_ready", "n_unservable", "n_late", "n_rigid", "reserved"]}[name]
    assert list(D.names) == want


def test_scratch_size(lib):
    f = lib.revs_flex_report_scratch
    base = f(3, 1000, 24)
    assert base > 0 and base % 16 == 0
    assert f(4, 1000, 24) >= base and f(3, 1001, 24) >= base and f(3, 1000, 25) >= base
    prev = 0
    for n in (1, 255, 256, 257, 600, 100000, 1000000):
        assert f(1, n, 96) >= prev and f(1, n, 96) % 16 == 0
        prev = f(1, n, 96)
    for T in range(1, 193):
        assert f(2, 300, T) >= f(2, 300, max(T - 1, 1)) > 0 and f(2, 300, T) % 16 == 0
    for S in (1, 2, 30, 4096):
        assert f(S, 300, 24) >= f(max(S - 1, 1), 300, 24) > 0
    assert f(1, 1, 1) > 0 and f(4096, 524287, 192) > 0
    for bad in ((0, 8, 4), (4097, 8, 4), (-1, 8, 4), (1, 0, 4), (1, -4, 4), (1, 8, 0), (1, 8, 193), (1, 8, -2),
                (4096, 524288, 4), (1, 2 ** 31, 4), (2, 2 ** 62, 4)):
        assert f(*bad) <= 0, bad


def _call(lib, S=2, n=8, T=5, p=64, stride_s=5, stride_i=10, homes=128, integral=0, on_frac=0.0, short_tol=1e-6,
          node_ptr=192, m=3, row=256, slot=512, day=768, hist=1024, node_up=2048, node_down=3072, val=1280, keep=1536,
          scratch=4096):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    return lib.revs_flex_report(S, n, T, p, stride_s, stride_i, homes, integral, on_frac, short_tol, node_ptr, m, row, slot,
                                day, hist, node_up, node_down, val, keep, scratch, None)


def test_flex_report_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    for S in (0, -3, 4097):
        assert _call(lib, S=S) == -1 and f"revs_flex_report: S={S}".encode() in err()
    for T in (0, -1, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    for n in (0, -1):
        assert _call(lib, n=n) == -1 and f"n={n}".encode() in err()
    assert _call(lib, n=2 ** 30, stride_s=5 * 2 ** 30, stride_i=5) == -1 and b"2^31" in err()      # S n = 2^31 exactly
    assert _call(lib, S=1, n=2 ** 40) == -1 and b"2^31" in err()
    # strides: revs_bill_rows' rule, as revs_charge_report has it
    for ss, si in ((4, 10), (5, 9), (5, 0), (0, 5), (40, 4), (39, 5), (-5, 10), (5, -10)):
        assert _call(lib, stride_s=ss, stride_i=si) == -1 and b"rows overlap" in err(), (ss, si)
        d = np.zeros(1)
        assert lib.revs_bill_rows(2, 8, 5, 64, 0, ss, si, 128, d.ctypes.data, None) == -1 and b"rows overlap" in err()
    assert _call(lib, p=None) == -1 and b"argument p" in err()
    assert _call(lib, homes=None) == -1 and b"argument homes" in err()
    for bad in (float("nan"), -0.5, -float("inf")):
        assert _call(lib, on_frac=bad) == -1 and b"on_frac" in err()
        assert _call(lib, short_tol=bad) == -1 and b"short_tol" in err()
    assert _call(lib, scratch=None) == -1 and b"argument scratch" in err()
    assert _call(lib, scratch=4104) == -1 and b"16-byte aligned" in err()
    none = dict(row=None, slot=None, day=None, hist=None, val=None, keep=None)
    assert _call(lib, node_up=None, node_down=None, **none) == -1 and b"every output is NULL" in err()
    # the node outputs: together, with node_ptr and m >= 1, m S T cells below 2^31
    assert _call(lib, node_up=None) == -1 and b"node_up and node_down" in err()
    assert _call(lib, node_down=None) == -1 and b"node_up and node_down" in err()
    assert _call(lib, node_down=None, **none) == -1 and b"node_up and node_down" in err()
    assert _call(lib, node_ptr=None) == -1 and b"argument node_ptr" in err()
    for m in (0, -2):
        assert _call(lib, m=m) == -1 and f"m={m}".encode() in err()
    assert _call(lib, m=2 ** 31 - 1) == -1 and b"m*S*T" in err()
    assert _call(lib, S=1, n=8, T=192, stride_s=1920, stride_i=192, m=(2 ** 31) // 192 + 1) == -1 and b"m*S*T" in err()
