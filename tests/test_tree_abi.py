"""Every entry point that takes the feeder as a tree (revs_tree_t) refuses a malformed one on the host, before any
launch, through the one predicate and with the one message of csrc/tree_body.h (no GPU here)."""
import ctypes as C

import pytest

P = 16          # a non-null "pointer" that is never dereferenced: the checks run before any launch


@pytest.fixture(scope="module")
def lib():
    from revs_admm_amd import _lib, build
    build.build()
    return _lib.load()


def _tree(n=8, pack=P, w=P, null=False):
    from revs_admm_amd import _lib
    return None if null else C.byref(_lib.Tree(n, pack, w))


# every argument but the tree is acceptable, so the tree is what each call is refused for
ENTRY_POINTS = {
    "revs_tree_voltage": lambda lib, tr: lib.revs_tree_voltage(4, 24, tr, P, 0.95, 1.05, P, P, None),
    "revs_op_dual_rows_tree": lambda lib, tr: lib.revs_op_dual_rows_tree(
        4, 24, tr, P, P, 0.95, 1.05, 4, P, P, P, None, P, P, P, P, 1.0, 1, None),
    "revs_op_dual_evaluate_tree": lambda lib, tr: lib.revs_op_dual_evaluate_tree(
        3, 4, 24, P, P, P, P, P, tr, P, 1, 1.0, 0.95, 1.05, 4, 1, P, P, P, P, P, P, P, P, P, P, 1.0, None),
    "revs_net_report": lambda lib, tr: lib.revs_net_report(4, 24, tr, P, P, None, None, 8, 1.0, 0.95, 1.05, P, None, None,
                                                           None, None),
    "revs_net_study": lambda lib, tr: lib.revs_net_study(2, 4, 24, tr, P, P, None, None, 8, 1.0, 0.95, 1.05, None, 0, None,
                                                         0, P, None, None, None, None, None, None, None),
}
# the smallest inputs that separate the branches of the predicate
BAD_TREES = {
    "n=0": dict(n=0),
    "n=12 (no multiple of 8)": dict(n=12),
    "n=8200 (beyond 8192: no multiple of 16)": dict(n=8200),
    "n=16392 (over REVS_TREE_MAX)": dict(n=16392),
    "pack=NULL": dict(pack=None),
    "w=NULL": dict(w=None),
    "a NULL tree": dict(null=True),
}


def _refused(lib, call, tree):
    return call(lib, tree) == -1 and b"multiple of 8" in lib.revs_last_error()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_every_shape_entry_points_refuse_a_malformed_tree(lib, name):
    for what, kw in BAD_TREES.items():
        assert _refused(lib, ENTRY_POINTS[name], _tree(**kw)), (name, what, lib.revs_last_error())
    # the message names the tree's size and the largest one
    assert ENTRY_POINTS[name](lib, _tree(n=16392)) == -1
    assert b"16392" in lib.revs_last_error() and b"16384" in lib.revs_last_error()


def _chain_kv(lib, tr):
    """revs_op_chain_kv with every argument but the tree acceptable (both sides, lists of the launch before given)"""
    from revs_admm_amd import _lib
    side = lambda base: _lib.ChainKvSide(P, P, base, P, P, P, P, P, P, 1.0, 4, 0)
    c = _lib.ChainKv(m=4, T=24, kadd=4, has_e2=1, vlo=0.95, vhi=1.05, kappa=1.0, delta=0.0, scale=1.0, eps=1e-8,
                     max_pivots=8, e1=side(P), e2=side(P + 16), R=P, k_full=P, yhat=P, info=P, y_trial=P + 16, lin_out=P,
                     sh_a=P, sh_b=P + 16, prev_cidx=P, prev_ccnt=P)
    if tr is not None:
        c.tree = C.pointer(tr._obj)         # (tr: what C.byref returned)
    return lib.revs_op_chain_kv(C.byref(c), None)


SWEEP_SHAPE = {
    "revs_op_dual_tree_select_model_step": lambda lib, tr: lib.revs_op_dual_tree_select_model_step(
        4, 24, tr, P, P, 0.95, 1.05, 4, P, P, P, P, P, P, P, 1.0, P, 1.0, 0.0, 8, P, P, P, 1.0, 1e-8, P + 16, P, None),
    "revs_op_chain_kv": _chain_kv,
}


def test_sweep_shape_entry_point_refuses_a_malformed_tree(lib):
    """revs_op_dual_tree_select_model_step and revs_op_chain_kv hold the 256 x 8 shape only: at most
    REVS_TREE_SWEEP_MAX = 2048 nodes."""
    for name, call in sorted(SWEEP_SHAPE.items()):
        for what, kw in dict(BAD_TREES, **{"n=2056 (over REVS_TREE_SWEEP_MAX)": dict(n=2056)}).items():
            assert _refused(lib, call, _tree(**kw)), (name, what, lib.revs_last_error())
        assert call(lib, _tree(n=2056)) == -1 and b"2056" in lib.revs_last_error() and b"2048" in lib.revs_last_error()


def test_chain_kv_refuses_a_null_descriptor(lib):
    assert lib.revs_op_chain_kv(None, None) == -1 and b"revs_op_chain_kv" in lib.revs_last_error()
