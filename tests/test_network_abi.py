"""revs_net_node_sums / revs_net_report (include/revs_admm_ops.h) are declared, exported and bound, and reject bad
arguments on the host, before any launch (no GPU here)."""
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
    for name in ("revs_net_node_sums", "revs_net_report"):
        assert re.search(rf"\bint {name}\s*\(", ops), name
        assert name not in boundary                       # (the boundary header stays at its 45 functions)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "network_kernels.hip" in __import__("revs_admm_amd.build", fromlist=["SOURCES"]).SOURCES


def test_summary_record_layout():
    """revs_net_summary_t: eight doubles, five counts, three reserved words -- 96 bytes, as the header documents."""
    from revs_admm_amd.network import SUMMARY_DTYPE
    assert SUMMARY_DTYPE.itemsize == 96
    names = ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi", "worst_value")
    assert [SUMMARY_DTYPE.fields[k][1] for k in names] == list(range(0, 64, 8))
    assert [SUMMARY_DTYPE.fields[k][1] for k in ("count", "n_fliers", "n_violations", "n_nan", "worst_index")] == \
        list(range(64, 84, 4))
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} revs_net_summary_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for part in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in part.split(",")]
    assert fields == list(names[:5]) + list(names[5:7]) + ["worst_value", "count", "n_fliers", "n_violations", "n_nan",
                                                           "worst_index", "reserved[3]"]


def _report(lib, m=4, T=24, n=8, tree=True, pack=16, w=16, node_g=32, rating=48, mask=None, nop=None, n_out=8,
            vset=1.0, vmin=0.95, vmax=1.05, flow=64, loading=None, volt=None, summary=None):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    from revs_admm_amd import _lib
    tr = C.byref(_lib.Tree(n, pack, w)) if tree else None
    return lib.revs_net_report(m, T, tr, node_g, rating, mask, nop, n_out, vset, vmin, vmax, flow, loading, volt,
                               summary, None)


def test_net_report_rejects_bad_arguments(lib):
    for T in (0, -1, 193, 999):
        assert _report(lib, T=T) == -1 and f"T={T}".encode() in lib.revs_last_error()
    assert _report(lib, m=0) == -1 and b"m=0" in lib.revs_last_error()
    assert _report(lib, m=70000) == -1
    assert _report(lib, node_g=None) == -1 and b"null pointer" in lib.revs_last_error()
    assert _report(lib, tree=False) == -1 and b"null pointer" in lib.revs_last_error()
    assert _report(lib, pack=None) == -1 and _report(lib, w=None) == -1
    assert _report(lib, n=16392, n_out=8) == -1 and b"16384" in lib.revs_last_error()      # over REVS_TREE_MAX
    assert _report(lib, n=12) == -1 and b"multiple of 8" in lib.revs_last_error()          # not padded
    assert _report(lib, n=8200, n_out=8) == -1                                             # (of 16 beyond 8192)
    assert _report(lib, n=0) == -1
    assert _report(lib, n_out=0) == -1 and _report(lib, n_out=9) == -1 and b"n_out" in lib.revs_last_error()
    assert _report(lib, vmin=1.06, vmax=1.05) == -1 and b"vmin > vmax" in lib.revs_last_error()
    assert _report(lib, vmin=float("nan")) == -1
    assert _report(lib, vset=float("nan")) == -1 and b"vset" in lib.revs_last_error()
    assert _report(lib, vset=float("inf")) == -1 and _report(lib, vset=-1.0) == -1
    assert _report(lib, flow=None) == -1 and b"every output is NULL" in lib.revs_last_error()


def test_net_node_sums_rejects_bad_arguments(lib):
    call = lambda m=4, T=24, node_ptr=16, load=32, p=48, out=64: lib.revs_net_node_sums(m, T, node_ptr, load, p, out, None)
    for T in (0, 193):
        assert call(T=T) == -1 and f"T={T}".encode() in lib.revs_last_error()
    assert call(m=0) == -1
    for k in ("node_ptr", "p", "out"):
        assert call(**{k: None}) == -1 and b"null pointer" in lib.revs_last_error(), k
