"""The tree-form kernels (csrc/tree_body.h) on feeders that are not stars, bit for bit: chains, hubs, balanced trees, combs
and caterpillars under a random renumbering, with zero-weight edges, junction nodes, unchecked rows and rows off the
tree, at position counts on and just past every shape boundary (256 x 8 up to 2048, 512 x 8 to 4096, 1024 x 8 to 8192,
1024 x 16 beyond).  The inputs are on the forward grid of tests/tree_cases.py -- every sum the three scans form is an
integer below 2^41 in units of 2^-10, exact in double in any order (tests/test_tree_cases.py) -- and the reference is
an integer recursion over the tree itself, so every comparison is ==.
  (a) revs_tree_voltage: voltages and the slots' largest violation, every kind at every size;
  (b) the shifts of an evaluation, revs_op_dual_evaluate_tree phase 1 (op_tree_shift_kernel);
  (c) the rows of an evaluation, revs_op_dual_rows_tree without and with the selection: staged through LDS, handed
      over through global memory (m too large for LDS), and the launches of more than 2048 positions.
Outputs start as junk so that anything left unwritten -- or written where it must not be -- shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import select_ref as sr
import tree_cases as tc

pytestmark = pytest.mark.gpu

A, T = 128, 3
JUNK, SEQ, KADD = -5, 11.0, 16
NODES = (8, 2048, 2056, 4096, 4104, 8192, 8193, 16384)          # 8193 nodes: 8208 positions, the first count padded to 16
POSITIONS = {n: {8193: 8208}.get(n, n) for n in NODES}
# (b), (c): one kind per size, and every kind at 2048 and at 8208 positions
SOME = sorted({(tc.KINDS[i % len(tc.KINDS)], n) for i, n in enumerate(NODES)} | {(k, n) for k in tc.KINDS for n in (2048, 8193)},
              key=lambda kn: (kn[1], kn[0]))


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _junk(shape, dtype=None, value=JUNK):
    import torch
    return torch.full(shape, value, dtype=dtype or torch.float64, device="cuda:0")


def _device_tree(c):
    from revs_admm_amd import _lib
    from revs_admm_amd.feeder import feeder_tree
    tr = feeder_tree(*c["forest"], c["checked"])
    keep = (_up(tr["pack"].view(np.int64)), _up(tr["w"]))
    return _lib.Tree(tr["n"], keep[0].data_ptr(), keep[1].data_ptr()), keep, tr


# ---- (a) revs_tree_voltage -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("n", NODES)
def test_tree_voltage(gpu_lib, kind, n):
    import torch
    from revs_admm_amd._lib import check, ptr
    c = tc.weighted_case(kind, n, 0, T)
    tree, keep, tr = _device_tree(c)
    assert tr["n"] == POSITIONS[n]
    m, chk, v = c["m"], c["checked"], c["v"]
    vlo, vhi = tc.bounds(v, chk)
    over, under = (v[chk] > vhi).any(axis=0), (v[chk] < vlo).any(axis=0)
    assert over.any() and under.any() and (v[chk] == vhi).any() and (v[chk] == vlo).any()
    v_out, rmax, dp = _junk((m, T), value=np.nan), _junk((T,)), _up(c["p"])
    check(gpu_lib.revs_tree_voltage(m, T, C.byref(tree), ptr(dp), vlo, vhi, ptr(v_out), ptr(rmax), None),
          "revs_tree_voltage")
    torch.cuda.synchronize()
    got = v_out.cpu().numpy()
    assert np.isnan(got[~chk]).all(), "written at a row that is unchecked or off the tree"
    bad = np.flatnonzero((got[chk] != v[chk]).any(axis=1))
    assert len(bad) == 0, (kind, n, len(bad), np.flatnonzero(chk)[bad][:8])
    want = np.maximum(np.maximum(v - vhi, vlo - v), 0.0)[chk].max(axis=0)
    assert np.array_equal(rmax.cpu().numpy(), want)


# ---- (b) the shifts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", SOME)
def test_shifts(gpu_lib, kind, n):
    """d = R^T y by the tree form into slab 0, at the rows with residences only (one residence per checked row); the home
    pass behind it against tests/fake_kernels.py's, fed the exact d, at the bars of
    test_shifts_by_the_tree_form_equal_the_dense_product.  kappa is the power of two that brings |d| / kappa to 1 at
    most (the division stays exact), gamma is scaled by it: free and clamped residences both occur."""
    import torch
    from fake_kernels import FakeKernels
    from revs_admm_amd._lib import check, ptr
    c = tc.weighted_case(kind, n, 0, T)
    tree, keep, tr = _device_tree(c)
    m, chk, d = c["m"], c["checked"], c["d"]
    assert np.abs(d).max() > 0
    kappa, ks = float(2.0 ** np.ceil(np.log2(np.abs(d).max()))), 4
    rng = np.random.default_rng(n)
    nres = int(chk.sum())
    node_ptr = np.concatenate([[0], np.cumsum(chk)]).astype(np.int64)
    pe, ps = (rng.uniform(0.0, 3.0, (nres, T)).astype(np.float32) for _ in range(2))
    gm = (rng.uniform(0.0, 3.0, (nres, T)) * kappa).astype(np.float32)
    d_sl, pnq, pen = _junk((ks, m, T)), _junk((3, m, T)), _junk((nres, T), torch.float32)
    dptr, dpe, dps, dgm, dy = (_up(a) for a in (node_ptr, pe, ps, gm, c["y"]))       # (named: alive until the launch is done)
    check(gpu_lib.revs_op_dual_evaluate_tree(
        1, m, T, ptr(dptr), ptr(dpe), ptr(dps), ptr(dgm), None, C.byref(tree), ptr(dy), 1, kappa,
        -1.0, 1.0, 2, ks, ptr(d_sl), ptr(pnq), ptr(pen), None, None, None, None, None, None, None, 0.0, None),
        "revs_op_dual_evaluate_tree")
    torch.cuda.synchronize()
    got = d_sl.cpu().numpy()
    assert (got[1:] == JUNK).all() and (got[0][~chk] == JUNK).all(), "written where no residence is"
    bad = np.flatnonzero((got[0][chk] != d[chk]).any(axis=1))
    assert len(bad) == 0, (kind, n, len(bad), np.flatnonzero(chk)[bad][:8])
    # the home pass on the exact shifts
    r_pnq, r_pen = np.zeros((3, m, T)), np.zeros((nres, T), np.float32)
    hold = [np.ascontiguousarray(x) for x in (node_ptr, pe, ps, gm, d.reshape(1, m, T))]
    q = lambda i: hold[i].ctypes.data
    FakeKernels().revs_op_dual_eval(m, T, q(0), q(1), q(2), q(3), 1, q(4), kappa, r_pnq.ctypes.data, r_pen.ctypes.data, None)
    g_pnq, g_pen = pnq.cpu().numpy(), pen.cpu().numpy()
    np.testing.assert_allclose(g_pen, r_pen, rtol=0, atol=5e-7)
    np.testing.assert_allclose(g_pnq[0], r_pnq[0], rtol=0, atol=1e-8)
    np.testing.assert_array_equal(g_pnq[1], r_pnq[1])
    assert (r_pen > 0).any() and (r_pen == 0).any()


# ---- (c) the rows ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_expected(kind, n, m_spread=0):
    c = tc.weighted_case(kind, n, 0, T)
    if m_spread:
        c = tc.spread(c, m_spread)
    chk = c["checked"]
    vlo, vhi = tc.bounds(c["v"], chk)
    pnq = np.ascontiguousarray(np.stack([c["p"], np.ones_like(c["p"]), c["q"]]))
    # a row without a checked position is not judged: no dual term, and the restatement sees it AT a bound (the voltages
    # here are all positive, so that the 0 the row keeps would lie below vlo) -- its v and violation stay zero
    eff = pnq.copy()
    eff[2] = np.where(chk[:, None], c["q"], 0.0)
    exp = sr.restate(np.where(chk[:, None], c["v"], vlo), c["y"], eff, vlo, vhi, KADD, A)
    exp["vfull"] = c["v"]
    assert (exp["viol"][~chk] == 0).all() and (c["v"][~chk] == 0).all()
    return c, pnq, vlo, vhi, exp


def _run_rows(lib, c, pnq, vlo, vhi, with_select):
    import torch
    from revs_admm_amd._lib import check, ptr
    tree, keep, tr = _device_tree(c)
    m = c["m"]
    z = lambda: torch.zeros(m, T, dtype=torch.float64, device="cuda:0")     # (rows without a position stay zero: the contract)
    b = dict(vfull=z(), viol=z(), partial=_junk((1, T, 4)), cidx=_junk((T, A), torch.int64), ccnt=_junk((T,), torch.int32),
             cval=_junk((T, 3, A)), stats=_junk((T, 8)))
    dpnq, dy = _up(pnq), _up(c["y"])
    check(lib.revs_op_dual_rows_tree(m, T, C.byref(tree), ptr(dpnq), ptr(dy), vlo, vhi, KADD, ptr(b["vfull"]),
                                     ptr(b["viol"]), ptr(b["partial"]), None, ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]),
                                     ptr(b["stats"]), SEQ, with_select, None), "revs_op_dual_rows_tree")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in b.items()}, tr


def _assert_rows(g, exp, with_select, rows_written, what):
    assert np.array_equal(g["partial"][0], exp["sums"]), (what, g["partial"][0], exp["sums"])
    if with_select:
        for k in ("ccnt", "cidx", "cval"):
            assert np.array_equal(g[k], exp[k]), (what, k)
        assert np.array_equal(g["stats"][:, 0:4], exp["sums"]) and (g["stats"][:, 5] == SEQ).all(), what
        assert (g["stats"][:, [4, 6, 7]] == JUNK).all(), what
    else:
        for k in ("ccnt", "cidx", "cval", "stats"):
            assert (g[k] == JUNK).all(), (what, k)
    if rows_written:
        assert np.array_equal(g["vfull"], exp["vfull"]) and np.array_equal(g["viol"], exp["viol"]), what
    else:                                       # (staged in LDS: vfull / viol are not written)
        assert (g["vfull"] == 0).all() and (g["viol"] == 0).all(), what


@pytest.mark.parametrize("with_select", [0, 1])
@pytest.mark.parametrize("kind,n", SOME)
def test_rows(gpu_lib, kind, n, with_select):
    c, pnq, vlo, vhi, exp = _rows_expected(kind, n)
    assert (exp["sums"][:, 2] > 0).all()
    if n >= 2048:                               # (more violated rows than are admitted, behind the rows with a multiplier)
        assert (exp["sums"][:, 3] > 0).all() and (exp["sums"][:, 3] > KADD).any()
        assert (exp["ccnt"] == exp["sums"][:, 2] + np.minimum(exp["sums"][:, 3], KADD)).all()
    g, tr = _run_rows(gpu_lib, c, pnq, vlo, vhi, with_select)
    assert tr["n"] == POSITIONS[n]
    _assert_rows(g, exp, with_select, tr["n"] > 2048 or not with_select, (kind, n, with_select))


@pytest.mark.parametrize("with_select", [0, 1])
def test_rows_hand_over_through_global_memory_on_a_comb(gpu_lib, with_select):
    """A comb of 2048 nodes whose rows are scattered over m = 4500: 3 m + 4 doubles do not fit in LDS beside the scan
    buffer (more than 120 KB), so rows and selection share a workgroup and meet in vfull / viol."""
    m = 4500
    c, pnq, vlo, vhi, exp = _rows_expected("comb", 2048, m)
    assert (2 + 2048 + 8 + 3 * m + 4) * 8 > 120 * 1024 and c["m"] == m
    assert (exp["sums"][:, 3] > KADD).all() and (exp["ccnt"] == exp["sums"][:, 2] + KADD).all()
    g, tr = _run_rows(gpu_lib, c, pnq, vlo, vhi, with_select)
    assert tr["n"] == 2048
    _assert_rows(g, exp, with_select, True, ("comb", m, with_select))
    for t in range(T):
        assert c["checked"][exp["cidx"][t, :exp["ccnt"][t]]].all()
