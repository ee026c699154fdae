"""tests/chain_cases.py on the CPU: every column is what its name claims (from the restatement's own counts), the
preconditions of revs_op_chain_kv hold in every column, the Gram sums are exact, every branch of op_chain_kv_kernel is taken at
two sizes at least (2048 among them), and restate_chain agrees with tests/fake_kernels.py (no GPU here)."""
import numpy as np
import pytest

import chain_cases as cc
import select_ref as sr

GEOS = list(cc.GEOMETRY)
NAMES = list(cc.NAMES)


def _col(name):
    return NAMES.index(name)


@pytest.mark.parametrize("geo", GEOS)
def test_preconditions_hold_in_every_column(geo):
    c = cc.case(geo)
    m, on, y, pci, pcc = c["m"], c["on"], c["y"], c["prev_cidx"], c["prev_ccnt"]
    assert y.shape == (m, sr.T) and c["pnq"].shape == (3, m, sr.T) and c["R"].shape == (m, m)
    assert (y[~on] == 0).all() and (c["v"][~on] == 0).all()
    assert np.abs(c["v"] / sr.G).max() <= sr.KMAX and (c["v"] / sr.G == np.round(c["v"] / sr.G)).all()
    for t in range(sr.T):
        pc = int(pcc[t])
        assert pc == -1 or 0 <= pc <= 2 * cc.KADD_PREV
        assert (pci[t, max(pc, 0):] == 0).all(), "list padding"           # (flagged -1: all of it)
        assert ((0 <= pci[t]) & (pci[t] < m)).all() and on[pci[t, :max(pc, 0)]].all()
        if pc >= 0:
            assert len(set(pci[t, :pc])) == pc
            assert set(np.flatnonzero(y[:, t])) <= set(pci[t, :pc]), (NAMES[t], "support on the list")
    # the dense R and N of the exactness claim
    R16, N = c["R"] * 16, c["pnq"][1]
    assert (R16 == np.round(R16)).all() and np.abs(R16).max() < 32 and (R16 == 0).any() == (m > 1)
    assert (N == np.round(N)).all() and (N == 0).any() == (m > 1) and 0 <= N.min() and N.max() <= 16


@pytest.mark.parametrize("geo", GEOS)
def test_the_tree_form_of_the_node_sums_is_v(geo):
    """feeder.py's restatement of the three prefix sums turns pnq[0] into v bit for bit on every geometry's forest -- p
    itself on the forests of roots, the injections of tests/tree_cases.py on the real trees, which are not degenerate:
    on those a gather in preorder where end-order is due does not return v (the chains aside: there the two agree)."""
    from revs_admm_amd.feeder import feeder_tree, tree_voltage_host
    import tree_cases as tc
    c = cc.case(geo)
    M, m, njun = cc.GEOMETRY[geo]
    tr = feeder_tree(*c["forest"], np.ones(m, bool))
    assert tr["n"] <= 2048 and (tr["src"] >= 0).sum() == M and len(c["forest"][0]) == M + njun
    assert np.array_equal(tree_voltage_host(tr, np.array(c["pnq"][0])), c["v"])
    if geo in cc.TREES:
        assert not np.array_equal(c["pnq"][0][c["on"]], c["v"][c["on"]])
        assert (c["forest"][0] > np.arange(M + njun)).any() and (tr["cle"] != np.arange(tr["n"])).any()
        assert (tr["end"] - np.arange(tr["n"]) > 64).any()
        o = cc.build(geo, seed=1)               # (test_gpu_chain_kv.py's verdict half: another draw on the same rows)
        p2, v2 = np.array(c["pnq"][0]), np.zeros_like(c["v"])
        p2[c["on"]], v2[c["on"]] = o["pnq"][0][o["on"]], o["v"][o["on"]]
        assert np.array_equal(tree_voltage_host(tr, p2), v2)
        wrong = tc.tree_voltage_preorder_gather(tr, np.array(c["pnq"][0]))
        assert np.array_equal(wrong, c["v"]) == (cc.TREES[geo][0] == "chain"), geo
    else:
        assert np.array_equal(tc.tree_voltage_preorder_gather(tr, np.array(c["pnq"][0])), c["v"])


@pytest.mark.parametrize("geo", GEOS)
def test_gram_sums_are_exact(geo):
    """K of the restatement == the same sums in integers (R 2^4 and N are integers, kappa = 4), and every partial sum of
    |r n r'| stays below 2^17: exact in double at resolution 2^-8 in any order."""
    c, e = cc.case(geo), cc.expected(geo)
    R16, N = np.round(c["R"] * 16).astype(np.int64), np.round(c["pnq"][1]).astype(np.int64)
    for t in range(sr.T):
        a = int(e["cnt"][t])
        if not 1 <= a <= 8:
            assert (e["K"][t] == 0).all()
            continue
        RF = R16[e["cidx"][t, :a]]
        Kint = (RF * N[:, t][None, :]) @ RF.T
        assert ((np.abs(RF) * N[:, t][None, :]) @ np.abs(RF).T).max() < 2 ** 17 * 256
        assert np.array_equal(e["K"][t, :a, :a] * (256 * cc.KAPPA), Kint.astype(np.float64)), NAMES[t]
        assert e["tr"][t] > 0, (NAMES[t], "a model without curvature")


@pytest.mark.parametrize("geo", GEOS)
def test_columns_are_what_their_names_claim(geo):
    c, e = cc.case(geo), cc.expected(geo)
    M = cc.GEOMETRY[geo][0]
    y, v, pci, pcc = c["y"], c["v"], c["prev_cidx"], c["prev_ccnt"]
    P = lambda name, **kw: cc.path(c, e, _col(name), **kw)
    lst = lambda name: e["cidx"][_col(name), :e["cnt"][_col(name)]]
    t = _col("empty")
    assert (e["ns"][t], e["nv"][t], e["cnt"][t], pcc[t]) == (0, 0, 0, 0) and "empty" in P("empty")
    if M == 1:                      # what fits in one row: a multiplier, or a violation, or nothing
        assert (e["cnt"] <= 1).all()
        return
    for k in range(1, 9):
        t = _col(f"a{k}")
        assert e["cnt"][t] == k and f"fast<{k}>" in P(f"a{k}") and "ranked" in P(f"a{k}"), (geo, k)
        assert "general" in P(f"a{k}", es=1) and "general" in P(f"a{k}", prev=False) and "npre=0" in P(f"a{k}", es=1)
    t = _col("unsorted_support")
    head = [r for r in pci[t, :pcc[t]] if y[r, t] != 0]
    assert len(head) == 4 and head != sorted(head) and "ranked" in P("unsorted_support")
    assert list(lst("unsorted_support")[:4]) == sorted(head)
    t = _col("not_same")
    assert not e["same"][t] and "not_same" in P("not_same") and e["ns"][t] == 2
    t = _col("leaving")
    a = e["cnt"][t]
    left = (e["cval"][t, 2, :a] != 0) & (e["yhat"][t, :a] == 0)
    assert left.any() and not left.all() and e["alpha"][t] == 1.0
    assert (e["y_trial"][lst("leaving")[left], t] == 0).all() and (y[lst("leaving")[left], t] != 0).all()
    t = _col("neg_zero")
    nz = np.flatnonzero((y[:, t] == 0) & np.signbit(y[:, t]))
    assert len(nz) == 1 and nz[0] in pci[t, :pcc[t]] and nz[0] in lst("neg_zero")[e["ns"][t]:] and e["viol"][nz[0], t] > 0
    t = _col("mult_on_violated")
    assert (np.abs(v[y[:, t] != 0, t]) > sr.VHI).all() and e["ns"][t] == 3 and e["nv"][t] == 3
    t = _col("at_bound")
    at = (y[:, t] == 0) & (np.abs(v[:, t]) == sr.VHI)
    assert at.sum() >= 4 and not set(np.flatnonzero(at)) & set(lst("at_bound")) and e["nv"][t] == 2
    assert (e["cval"][t, 1, :e["ns"][t]] == 0).all()
    t = _col("no_step")
    assert e["alpha"][t] == 0.0 and e["ns"][t] == 3 and e["sums"][t, 0] == 0 and "no_step" in P("no_step")
    assert np.array_equal(e["y_trial"][:, t], y[:, t])
    for name in ("nine", "many"):
        t = _col(name)
        assert e["ns"][t] <= 8 < e["cnt"][t] and e["info"][t] == -999 and "over8" in P(name) and "ranked" in P(name)
        assert np.array_equal(e["y_trial"][:, t], y[:, t])
    assert e["cnt"][_col("nine")] == 9 and e["ns"][_col("many")] == 8
    assert pcc[_col("prev9")] == 9 and "general" in P("prev9") and 1 <= e["cnt"][_col("prev9")] <= 8
    assert pcc[_col("prev_overflow")] == -1 and "general" in P("prev_overflow") and 1 <= e["cnt"][_col("prev_overflow")] <= 8
    assert (pci[_col("prev_overflow")] == 0).all()
    if M >= 257:
        assert e["nv"][_col("nv256")] == 256 and "ranked" in P("nv256")
        assert e["nv"][_col("nv257")] == 257 and "general" in P("nv257")
        for name in ("nv256", "nv257"):             # tied violations at the cut
            t = _col(name)
            cut = e["viol"][lst(name)[-1], t]
            assert (e["viol"][:, t] == cut).sum() > 1 and e["cnt"][t] == e["ns"][t] + cc.KADD
    t = _col("ties_one_thread")
    rows = np.flatnonzero(c["on"])                  # (the columns are built in the numbering of the rows ON the tree)
    own = {int(rows[r]) for r in set(range(8, 16)) | set(range(5, M, 256)) if r < M}
    top = e["viol"][:, t].max()
    assert set(np.flatnonzero(e["viol"][:, t] == top)) == own
    if M >= 255:
        assert set(lst("ties_one_thread")[:8]) <= own and e["cnt"][t] == cc.KADD
    t = _col("ends")
    assert {rows[0], rows[M - 1]} <= set(lst("ends")[e["ns"][t]:]) and 1 <= e["cnt"][t] <= 8


def test_no_column_is_skipped_and_every_branch_is_taken_at_two_sizes():
    """Over the size list: every branch of the launch at two sizes at least, 2048 among them."""
    where = {}
    for M in cc.SIZES:
        c, e = cc.case(str(M)), cc.expected(str(M))
        assert len(e["cnt"]) == len(NAMES) == sr.T
        for t, name in enumerate(NAMES):
            p = cc.path(c, e, t)
            marks = set(p)
            if "general" in p:              # which refusal of chain_rows_select_body
                marks.add("refused:prev>8" if c["prev_ccnt"][t] > 8 else "refused:prev<0" if c["prev_ccnt"][t] < 0
                          else "refused:nv>256")
            if e["nv"][t] == 256 and "ranked" in p:
                marks.add("ranked:nv=256")
            a = e["cnt"][t]
            if 1 <= a <= 8 and ((e["cval"][t, 2, :a] != 0) & (e["y_trial"][e["cidx"][t, :a], t] == 0)).any():
                marks.add("leaving")
            head = [r for r in c["prev_cidx"][t, :max(c["prev_ccnt"][t], 0)] if c["y"][r, t] != 0]
            if "ranked" in p and head != sorted(head):
                marks.add("rank reorders")
            if "ranked" in p and len(head) >= 5:
                marks.add("rank of 5..8")
            if (c["y"][:, t] == 0).all() and e["nv"][t] > 0:
                marks.add("ns=0 with violations")
            for k in marks:
                where.setdefault(k, set()).add(M)
    want = ({f"fast<{k}>" for k in range(1, 9)} |
            {"ranked", "general", "empty", "over8", "npre=0", "npre=A", "npre<A", "ns>=5", "same", "not_same", "no_step",
             "refused:prev>8", "refused:prev<0", "refused:nv>256", "ranked:nv=256", "leaving", "rank reorders",
             "rank of 5..8", "ns=0 with violations"})
    assert want <= set(where), want - set(where)
    for k in want:
        assert len(where[k]) >= 2 and 2048 in where[k], (k, where[k])
    for k in range(1, 9):
        assert where[f"fast<{k}>"] >= {M for M in cc.SIZES if M >= 9}


@pytest.mark.parametrize("geo", GEOS)
def test_restatement_equals_the_test_double(geo):
    """restate_chain against FakeKernels: revs_op_dual_select + revs_op_dual_model_small + revs_op_dual_step_pending on the
    same inputs (columns of more than 8 candidates aside: the double solves those, the small model flags them)."""
    from fake_kernels import FakeKernels
    c, e = cc.case(geo), cc.expected(geo)
    m, nt, A = c["m"], sr.T, cc.A
    fk = FakeKernels()
    v, y = np.ascontiguousarray(c["v"]), np.ascontiguousarray(c["y"])
    pnq = c["pnq"].copy()
    pnq[2] = np.where(c["on"][:, None], pnq[2], 0.0)
    nblk = fk.revs_op_dual_blocks(m)
    vfull, viol, part = np.zeros((m, nt)), np.zeros((m, nt)), np.zeros((nblk, nt, 4))
    cidx, ccnt, cval = np.zeros((nt, A), np.int64), np.zeros(nt, np.int32), np.zeros((nt, 3, A))
    stats, R = np.zeros((nt, 8)), np.ascontiguousarray(c["R"])
    d = lambda a: a.ctypes.data
    fk.revs_op_dual_select(m, nt, 1, d(v), d(pnq), d(y), sr.VLO, sr.VHI, cc.KADD, d(vfull), d(viol), d(part), d(cidx),
                           d(ccnt), d(cval), d(stats), 3.0, None)
    for k, got in (("cidx", cidx), ("ccnt", ccnt), ("cval", cval)):
        assert np.array_equal(got, e[k]), k
    assert np.array_equal(stats[:, :4], e["sums"])
    small = ccnt <= 8
    cc8 = np.where(small, ccnt, 0).astype(np.int32)
    yhat, info, ytr, lin = np.zeros((nt, A)), np.zeros(nt, np.int32), np.full((m, nt), 9.0), np.zeros((nt, 8))
    N = np.ascontiguousarray(pnq[1])
    fk.revs_op_dual_model_small(m, nt, d(R), d(N), d(cidx), d(cc8), d(cval), cc.KAPPA, cc.DELTA, cc.MAX_PIVOTS, None,
                                d(yhat), d(info), None)
    fk.revs_op_dual_step_pending(nt, d(cidx), d(cc8), d(cval), d(yhat), d(stats), cc.SCALE, cc.EPS, d(y), m, d(ytr), d(lin),
                                 None)
    assert np.array_equal(yhat, e["yhat"]) and np.array_equal(info[small], e["info"][small])
    assert (e["info"][~small] == -999).all()
    assert np.array_equal(ytr, e["y_trial"])
    np.testing.assert_allclose(lin[:, 0], e["lin"], rtol=1e-13, atol=0)
    # the model's answer is a solution of the LCP it states (tests/test_gpu_newton.py: test_model_problem_sizes)
    for t in np.flatnonzero(small & (ccnt > 0)):
        assert cc.lcp_ok(e, t, e["yhat"][t]), cc.NAMES[t]


@pytest.mark.parametrize("geo", ["9", "257"])
def test_shifts_in_both_orders(geo):
    """sh_a / sh_b of the restatement are R_F^T y_trial / kappa (any order agrees to rounding), and differ in the summation
    order only where the column is not `same`."""
    c, e = cc.case(geo), cc.expected(geo)
    ref = (c["R"].T @ e["y_trial"]).T / cc.KAPPA
    for sh in (e["sh_a"], e["sh_b"]):
        np.testing.assert_allclose(sh, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    assert np.array_equal(e["sh_a"][e["same"]], e["sh_b"][e["same"]])
    assert (e["sh_a"][_col("empty")] == 0).all()
