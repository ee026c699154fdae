"""revs_net_node_sums_many (include/revs_admm_ops.h) is exported and bound, and rejects bad arguments on the host, before
any launch (no GPU here)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def _call(lib, S=3, m=10, T=24, node_ptr=8, load=16, p=24, node_g=32):
    # (non-null "pointers" that are never dereferenced: the checks run before any launch)
    return lib.revs_net_node_sums_many(S, m, T, node_ptr, load, p, node_g, None)


def _rejected(lib, names, **kw):
    assert _call(lib, **kw) == -1, kw
    err = lib.revs_last_error()
    assert b"revs_net_node_sums_many" in err and all(n.encode() in err for n in names), (kw, err)


def test_the_symbol_is_declared_exported_and_bound(lib):
    from test_abi import header_functions
    from revs_admm_amd import _lib
    assert "revs_net_node_sums_many" in header_functions(("revs_admm_ops.h",))
    assert "revs_net_node_sums_many" in _lib.SIGNATURES and hasattr(lib, "revs_net_node_sums_many")
    assert len(_lib.SIGNATURES["revs_net_node_sums_many"][1]) == 8


def test_node_sums_many_rejects_bad_arguments(lib):
    for S in (0, -1, 4097):                               # REVS_STUDY_MAX_S = 4096
        _rejected(lib, [f"S={S}"], S=S)
    for T in (0, 193):                                    # REVS_MAX_T = 192
        _rejected(lib, [f"T={T}"], T=T)
    for m in (0, 65536):                                  # the report's limit
        _rejected(lib, [f"m={m}"], m=m)
    assert 32768 * 4096 * 16 == 2 ** 31
    _rejected(lib, [f"m*S*T={2 ** 31}"], m=32768, S=4096, T=16)
    for k in ("node_ptr", "p", "node_g"):
        _rejected(lib, ["null pointer", k], **{k: None})


def test_a_null_load_passes_the_checks(lib):
    """load = NULL means p alone: with it the only refusals left are the other arguments' -- the same call with a bad
    S names S, not load (a valid call would launch: that is tests/test_gpu_node_sums_many.py's)."""
    _rejected(lib, ["S=0"], S=0, load=None)
    _rejected(lib, ["null pointer", "node_g"], load=None, node_g=None)
    err = lib.revs_last_error()
    assert b"load" not in err
