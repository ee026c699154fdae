"""revs_dual_bound_many (include/revs_admm_ops.h) rejects bad arguments on the host, before any launch, and sizes its
scratch as S single calls (no GPU here)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def _call(lib, n=10, S=3, T=24, cost=8, homes=16, node_of=24, m=4, d=None, y=None, load_node=None, scale=56,
          vlo=-0.1, vhi=0.1, scratch=32, out=40):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    return lib.revs_dual_bound_many(n, S, T, cost, homes, node_of, m, d, y, load_node, scale, vlo, vhi, 0, scratch,
                                    out, None)


def _rejected(lib, names, **kw):
    assert _call(lib, **kw) == -1, kw
    err = lib.revs_last_error()
    assert b"revs_dual_bound_many" in err and all(n.encode() in err for n in names), (kw, err)


def test_dual_bound_many_rejects_bad_arguments(lib):
    for T in (0, -1, 193, 999):
        _rejected(lib, [f"T={T}"], T=T)
    for S in (0, -2):
        _rejected(lib, [f"S={S}"], S=S)
    _rejected(lib, ["S*T=1032"], S=43, T=24)              # REVS_ENS_MAX_COLS = 1024 columns
    _rejected(lib, ["S*T=1152"], S=6, T=192)
    _rejected(lib, ["n_res"], n=-1)
    for m in (0, -3):
        _rejected(lib, ["m >"], m=m)
    for k in ("cost", "scale", "scratch", "out", "homes", "node_of"):
        _rejected(lib, ["null pointer", k], **{k: None})
    assert _call(lib, n=0, homes=None, node_of=None, S=0) == -1        # (n_res = 0 needs neither; S = 0 still refused)
    _rejected(lib, ["without y"], d=48)
    _rejected(lib, ["without d"], y=48)
    _rejected(lib, ["vlo > vhi"], vlo=0.2, vhi=0.1)
    # 8 lanes per residence at T = 24: 32 residences per workgroup -> 2^31 workgroups per scenario
    _rejected(lib, ["n_res", "too many"], n=32 * 2 ** 31, S=1)


def test_dual_bound_many_scratch_is_S_single_scratches(lib):
    one = lib.revs_dual_bound_scratch
    many = lib.revs_dual_bound_many_scratch
    assert many(100, 1, 24) == one(100, 24) == 2 * (24 + 4)
    assert many(100, 3, 24) == 3 * one(100, 24) == 3 * 2 * (24 + 4)
    assert many(0, 4, 96) == 4 * one(0, 96) == 4 * 2 * 96
    assert many(10, 5, 193) == 0
    assert many(10, 0, 24) == 0
    assert many(10, 43, 24) == 0          # 1032 columns
    assert many(-1, 2, 24) == 0
