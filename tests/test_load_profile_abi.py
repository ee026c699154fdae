"""revs_load_profile / revs_load_profile_scratch (include/revs_admm_ops.h) are declared, exported and bound, the day
record has the documented layout, and bad arguments are rejected on the host, before any launch (no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("revs_load_profile", "revs_load_profile_scratch", "revs_load_profile_chunk")


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from revs_admm_amd import _lib, build
    ops = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    boundary = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert re.search(r"\bint revs_load_profile\s*\(", ops) and re.search(r"\bint64_t revs_load_profile_scratch\s*\(", ops)
    assert re.search(r"\bint32_t revs_load_profile_chunk\s*\(", ops)
    for name in NAMES:
        assert name not in boundary
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["revs_load_profile"][1]) == 19 and len(_lib.SIGNATURES["revs_load_profile_scratch"][1]) == 5
    assert "load_profile_kernels.hip" in build.SOURCES
    assert re.search(r"#define REVS_PROFILE_MAX_CLASSES\s+4\b", ops) and _lib.PROFILE_MAX_CLASSES == 4
    assert 1 <= lib.revs_load_profile_chunk() <= 20000 // 3


def test_day_record_layout():
    from revs_admm_amd._lib import PROFILE_DAY_DTYPE as D
    assert D.itemsize == 64
    assert {k: D.fields[k][1] for k in D.names} == dict(peak=0, valley=8, energy=16, load_factor=24, sum_peaks=32,
                                                         diversity=40, peak_slot=48, valley_slot=52, slots=56, reserved=60)
    assert all(D.fields[k][0] == np.dtype("<f8") for k in D.names[:6]) and all(D.fields[k][0] == np.dtype("<i4") for k in D.names[6:])
    hdr = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} revs_profile_day_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for part in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in part.split(",")]
    assert fields == list(D.names)


def test_scratch_size(lib):
    f = lib.revs_load_profile_scratch
    base = f(3, 1000, 24, 2, 2)
    assert base > 0 and base % 16 == 0
    # never smaller in any size
    assert f(4, 1000, 24, 2, 2) >= base and f(3, 1001, 24, 2, 2) >= base and f(3, 1000, 25, 2, 2) >= base
    assert f(3, 1000, 24, 3, 2) >= base and f(3, 1000, 24, 2, 3) >= base
    assert f(1, 1, 1, 0, 0) > 0 and f(1, 1000000, 96, 2, 0) > f(1, 100000, 24, 2, 0) > 0
    assert f(4096, 524287, 192, 4, 4096) > 0
    for bad in ((0, 8, 4, 0, 0), (4097, 8, 4, 0, 0), (-1, 8, 4, 0, 0), (1, 0, 4, 0, 0), (1, -4, 4, 0, 0), (1, 8, 0, 0, 0),
                (1, 8, 193, 0, 0), (1, 8, -2, 0, 0), (1, 8, 4, -1, 0), (1, 8, 4, 5, 0), (1, 8, 4, 0, -1), (1, 8, 4, 0, 2),
                (3, 8, 4, 0, 4), (4096, 524288, 4, 0, 0), (1, 2 ** 31, 4, 0, 0), (2, 2 ** 62, 4, 0, 0)):
        assert f(*bad) <= 0, bad


def _call(lib, S=2, n=8, T=5, g=64, stride_s=5, stride_i=10, cls=128, C=2, index=None, groups=(0, -1), G=1, above=0.5,
          slot=256, peak=512, day=768, pslot=1024, ppeak=1280, scratch=4096):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    hg = None if groups is None else np.asarray(groups, np.int32)
    return lib.revs_load_profile(S, n, T, g, stride_s, stride_i, cls, C, index, None if hg is None else hg.ctypes.data, G,
                                 above, slot, peak, day, pslot, ppeak, scratch, None)


def test_load_profile_rejects_bad_arguments(lib):
    err = lambda: lib.revs_last_error()
    none = dict(groups=None, G=0, pslot=None, ppeak=None)
    for S in (0, -3, 4097):
        assert _call(lib, S=S, **none) == -1 and f"revs_load_profile: S={S}".encode() in err()
    for T in (0, -1, 193):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in err()
    for n in (0, -1):
        assert _call(lib, n=n) == -1 and f"n={n}".encode() in err()
    assert _call(lib, n=2 ** 30, stride_s=5 * 2 ** 30, stride_i=5) == -1 and b"2^31" in err()      # S n = 2^31 exactly
    assert _call(lib, S=1, n=2 ** 40, groups=(0,)) == -1 and b"2^31" in err()
    for C in (-1, 5):
        assert _call(lib, C=C) == -1 and f"C={C}".encode() in err()
    assert _call(lib, cls=None, C=2) == -1 and b"disagree" in err()
    assert _call(lib, cls=128, C=0) == -1 and b"disagree" in err()
    # strides: revs_bill_rows' rule
    for ss, si in ((4, 10), (5, 9), (5, 0), (0, 5), (40, 4), (39, 5), (-5, 10), (5, -10)):
        assert _call(lib, stride_s=ss, stride_i=si) == -1 and b"rows overlap" in err(), (ss, si)
    assert _call(lib, above=float("nan")) == -1 and b"above" in err()
    assert _call(lib, g=None) == -1 and b"argument g" in err()
    for G in (-1, 3):
        assert _call(lib, G=G) == -1 and f"G={G}".encode() in err()
    assert _call(lib, groups=None) == -1 and b"groups is NULL" in err()
    assert _call(lib, groups=(0, 1)) == -1 and b"groups[1]=1" in err()
    assert _call(lib, groups=(-2, 0)) == -1 and b"groups[0]=-2" in err()
    assert _call(lib, groups=None, G=0, ppeak=None) == -1 and b"pool output with G == 0" in err()
    assert _call(lib, groups=None, G=0, pslot=None) == -1 and b"pool output with G == 0" in err()
    assert _call(lib, scratch=None) == -1 and b"argument scratch" in err()
    assert _call(lib, scratch=4104) == -1 and b"16-byte aligned" in err()
    assert _call(lib, slot=None, peak=None, day=None, pslot=None, ppeak=None) == -1 and b"every output is NULL" in err()
    assert _call(lib, slot=None, peak=None, day=None, **none) == -1 and b"every output is NULL" in err()

