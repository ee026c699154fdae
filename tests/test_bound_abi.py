"""revs_dual_bound (include/revs_admm.h) rejects bad arguments on the host, before any launch (no GPU here)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def _call(lib, n=10, T=24, cost=8, homes=16, node_of=24, m=4, d=None, y=None, load_node=None, scale=1.0,
          vlo=-0.1, vhi=0.1, scratch=32, p_node=None, out=40):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    return lib.revs_dual_bound(n, T, cost, homes, node_of, m, d, y, load_node, scale, vlo, vhi, 0, scratch, p_node,
                               out, None)


def test_dual_bound_rejects_bad_arguments(lib):
    for T in (0, -1, 193, 999):
        assert _call(lib, T=T) == -1 and f"T={T}".encode() in lib.revs_last_error()
    assert _call(lib, n=-1) == -1
    assert _call(lib, m=0) == -1
    for k in ("cost", "scratch", "out", "homes", "node_of"):
        assert _call(lib, **{k: None}) == -1 and b"null pointer" in lib.revs_last_error(), k
    assert _call(lib, scale=-1e-300) == -1 and b"scale" in lib.revs_last_error()
    assert _call(lib, scale=float("nan")) == -1
    assert _call(lib, d=48) == -1 and b"without y" in lib.revs_last_error()
    assert _call(lib, y=48) == -1 and b"without d" in lib.revs_last_error()
    assert _call(lib, vlo=0.2, vhi=0.1) == -1


def test_dual_bound_scratch_size(lib):
    # T = 24: 8 lanes per residence, 32 residences per workgroup -> {2 partials} x (T slot + 4 residence workgroups)
    assert lib.revs_dual_bound_scratch(100, 24) == 2 * (24 + 4)
    assert lib.revs_dual_bound_scratch(0, 96) == 2 * 96
    assert lib.revs_dual_bound_scratch(1_000_000, 96) == 2 * (96 + 62_500)     # 16 lanes at T = 96
    assert lib.revs_dual_bound_scratch(10, 0) == 0 and lib.revs_dual_bound_scratch(10, 193) == 0
