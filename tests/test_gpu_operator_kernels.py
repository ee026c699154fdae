"""The operator's ADMM kernels (csrc/operator_kernels.hip), entry by entry through the C ABI, against
their numpy restatements in tests/fake_kernels.py: inputs, the rounding bound and the comparison are
tests/operator_cases.py (checked on the CPU by tests/test_operator_cases_ref.py).  Every array an
entry writes is compared; every array it only reads must come back bit for bit."""
import numpy as np
import pytest

import operator_cases as oc

pytestmark = pytest.mark.gpu

T_EDGES = (1, 7, 32, 33, 64, 65, 128, 129, 256)          # both edges of every TL
NODE_SHAPES = ((1, 1), (37, 7), (50, 24), (24, 24), (300, 33), (11, 96), (5, 256))
WIDE = (3, 300)                                           # entries without a T limit


def _check(lib, entry, a, s):
    ref, got = oc.run_both(entry, a, s, lib=lib)
    used = oc.compare(entry, a, s, ref, got)
    return ref, got, used


# ---- residence-shaped kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("T", T_EDGES)
def test_home_pass(gpu_lib, T):
    for alpha in (1.6, 1.0):
        # xc = NULL: only rhat, s_b untouched (compare() holds every unwritten array to its bits)
        a, s = oc.make_home_pass(T, "rhs", alpha)
        ref, got, _ = _check(gpu_lib, "revs_op_home_pass", a, s)
        assert oc.same_bits(got["sb"], a["sb"])
        assert (got["rhat"][np.diff(a["node_ptr"]) == 0] == 0).all()          # empty nodes
        # update without residuals
        a, s = oc.make_home_pass(T, "upd", alpha)
        _check(gpu_lib, "revs_op_home_pass", a, s)
        # update with res and cty: rows 1, 2, 5, 6, 7 the maximum of old and new, rows 0, 3, 4 their bits
        a, s = oc.make_home_pass(T, "res", alpha)
        ref, got, _ = _check(gpu_lib, "revs_op_home_pass", a, s)
        new = oc.run_lib_seq(gpu_lib, [("revs_op_home_pass", s)], dict(a, res=np.zeros((8, T))))["res"]
        rows = [1, 2, 5, 6, 7]
        assert (got["res"][rows] == np.maximum(a["res"][rows], new[rows])).all()
        assert oc.same_bits(got["res"][[0, 3, 4]], a["res"][[0, 3, 4]]) and (new[[0, 3, 4]] == 0).all()


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("bscale_on", [True, False])
def test_home_pass_fused(gpu_lib, T, nslab, bscale_on):
    for alpha in (1.6, 1.0):
        a, s = oc.make_home_pass_fused(T, nslab, bscale_on, alpha)
        ref, got, _ = _check(gpu_lib, "revs_op_home_pass_fused", a, s)
        # ... and it is revs_op_node_update followed by revs_op_home_pass on the GPU itself
        two = oc.run_lib_seq(gpu_lib, [("revs_op_node_update", s), ("revs_op_home_pass", s)], a)
        for name in ("sb", "zv", "yv", "w", "xc"):
            assert oc.same_bits(got[name], two[name]), name
        S, chain = oc.bounds("revs_op_home_pass_fused", a, s)["rhat"]
        assert oc.close(got["rhat"], two["rhat"], S, chain)


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("preclamp", [0, 1])
def test_node_prep(gpu_lib, T, preclamp):
    for g0_out_on in (True, False):
        a, s = oc.make_node_prep(T, preclamp, g0_out_on)
        ref, got, _ = _check(gpu_lib, "revs_op_node_prep", a, s)
        empty = np.diff(a["node_ptr"]) == 0
        assert np.isposinf(got["gmin"][empty]).all() and (got["p0"][empty] == 0).all()
        assert np.isfinite(got["gmin"][~empty]).all()


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("preclamp", [0, 1])
def test_node_apply(gpu_lib, T, preclamp):
    for dzero in (False, True):
        a, s = oc.make_node_apply(T, preclamp, dzero)
        ref, got, used = _check(gpu_lib, "revs_op_node_apply", a, s)
        assert (got["pe_new"] >= 0).all() and (got["pe_new"] == 0).any() and (got["pe_new"] > 0).any()
        print(f"node_apply T={T} preclamp={preclamp} dzero={dzero}: float-ulp allowance used on "
              f"{used['ulp32']} of {got['pe_new'].size} elements")


# ---- node-shaped kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,T", NODE_SHAPES + (WIDE,))
def test_init_node_row_scale_node_w(gpu_lib, M, T):
    for bscale_on in (True, False):
        _check(gpu_lib, "revs_op_init_node", *oc.make_init_node(M, T, bscale_on))
    _check(gpu_lib, "revs_op_row_scale", *oc.make_row_scale(M, T))
    _check(gpu_lib, "revs_op_node_w", *oc.make_node_w(M, T))


@pytest.mark.parametrize("M,T", NODE_SHAPES + (WIDE,))
@pytest.mark.parametrize("nslab", [1, 3])
def test_node_scale_and_nodefast_scale(gpu_lib, M, T, nslab):
    _check(gpu_lib, "revs_op_node_scale", *oc.make_node_scale(M, T, nslab))
    _check(gpu_lib, "revs_op_nodefast_scale", *oc.make_nodefast_scale(M, T, nslab))


def _res_rows_merge(lib, entry, a, s, got, rows):
    """rows: the maximum of what was there and of what the call produces (taken from a second call on
    a zeroed res); every other row keeps its bits."""
    T = s["T"]
    new = oc.run_lib_seq(lib, [(entry, s)], dict(a, res=np.zeros((8, T))))["res"]
    other = [r for r in range(8) if r not in rows]
    assert (got["res"][rows] == np.maximum(a["res"][rows], new[rows])).all()
    assert oc.same_bits(got["res"][other], a["res"][other]) and (new[other] == 0).all()


@pytest.mark.parametrize("M,T", NODE_SHAPES)
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("bscale_on", [True, False])
def test_node_update_and_nodefast_update(gpu_lib, M, T, nslab, bscale_on):
    for make, entry in ((oc.make_node_update, "revs_op_node_update"),
                        (oc.make_nodefast_update, "revs_op_nodefast_update")):
        for alpha in (1.6, 1.0):
            _check(gpu_lib, entry, *make(M, T, nslab, bscale_on, None, alpha))
            a, s = make(M, T, nslab, bscale_on, "fill", alpha)
            ref, got, _ = _check(gpu_lib, entry, a, s)
            _res_rows_merge(gpu_lib, entry, a, s, got, [0, 3, 4])


@pytest.mark.parametrize("M,T", NODE_SHAPES)
@pytest.mark.parametrize("nslab", [1, 3])
def test_nodefast_dualres(gpu_lib, M, T, nslab):
    _check(gpu_lib, "revs_op_nodefast_dualres", *oc.make_nodefast_dualres(M, T, nslab, "zero"))
    a, s = oc.make_nodefast_dualres(M, T, nslab, "fill")
    ref, got, _ = _check(gpu_lib, "revs_op_nodefast_dualres", a, s)
    _res_rows_merge(gpu_lib, "revs_op_nodefast_dualres", a, s, got, [2, 5, 6, 7])


@pytest.mark.parametrize("M,T", NODE_SHAPES + (WIDE,))
@pytest.mark.parametrize("nslab", [1, 3])
def test_nodefast_feas_and_finish(gpu_lib, M, T, nslab):
    for fill in ("zero", "above"):
        for violate in (False, True):
            for bscale_on in (True, False):
                a, s = oc.make_nodefast_feas(M, T, nslab, bscale_on, violate, fill)
                ref, got, _ = _check(gpu_lib, "revs_op_nodefast_feas", a, s)
                if fill == "above" or not violate:
                    assert oc.same_bits(got["stats"], a["stats"])               # stays as given
            a, s = oc.make_nodefast_finish(M, T, nslab, violate, fill)
            ref, got, _ = _check(gpu_lib, "revs_op_nodefast_finish", a, s)
            assert np.isposinf(got["slack"][np.isposinf(a["gmin"])]).all()
            if fill == "above":
                assert oc.same_bits(got["stats"], a["stats"])
            elif not violate:
                assert got["stats"][0] == 0 and got["stats"][1] == np.abs(a["p0"]).max()


# ---- residence-count kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(255, 1), (256, 1), (257, 1), (3001, 7)])
def test_g0_init_home_export(gpu_lib, n, T):
    _check(gpu_lib, "revs_op_g0", *oc.make_g0(n, T))                   # bit-equal: one fmaf
    _check(gpu_lib, "revs_op_init_home", *oc.make_init_home(n, T))
    a, s = oc.make_export(n, T)
    ref, got, _ = _check(gpu_lib, "revs_op_export", a, s)              # bit-equal
    assert (got["pe"] == 0).any() and (got["pe"] > 0).any()


@pytest.mark.parametrize("T", T_EDGES)
def test_aggregate_f32(gpu_lib, T):
    a, s = oc.make_aggregate(T, integer=True)
    ref, got, _ = _check(gpu_lib, "revs_aggregate_f32", a, s)
    assert oc.same_bits(got["out"], ref["out"])                         # integer-valued floats: exact
    x = np.zeros((s["m"], T))
    np.add.at(x, np.repeat(np.arange(s["m"]), np.diff(a["node_ptr"])), a["inp"].astype(np.float64))
    assert (got["out"] == x).all()
    _check(gpu_lib, "revs_aggregate_f32", *oc.make_aggregate(T, integer=False))   # chain 2^-24 sum|x|

