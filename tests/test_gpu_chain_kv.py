"""The folded chain's operator launch, branch by branch (revs_op_chain_kv = chain_kv_launch: op_chain_kv_kernel), and the
three-pass chain's (revs_op_dual_tree_select_model_step), on the columns of tests/chain_cases.py: tests/test_chain_cases.py
holds on the CPU that every column is what its name claims and that every branch is taken at two sizes at least.

  (a) the step half against the numpy restatement, bit for bit where the inputs make the arithmetic exact (lists, stats,
      partial sums, the Gram block, the pivot count), in the four forms es = 1 | 4, with | without the previous lists;
  (b) against its parts: revs_op_dual_rows_tree(with_select) + revs_op_dual_model_small + revs_op_dual_step_pending;
  (c) the shifts against a long-double product of the launch's own trial multipliers, to the rounding of an fma chain;
  (d) both halves in one launch: the verdict half against select_ref.restate(), stats forwarding, the clears;
  (e) the golden 121144 feeder -- its tree with junction nodes and its own R -- against the parts.
The geometries of chain_cases.TREES put (a)-(d) and the three-pass launch on a chain, a comb and a comb with split edges
under random node numbers (the others are forests of roots, on which the three scans are the identity).
Outputs start as junk so that anything left unwritten shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import chain_cases as cc
import select_ref as sr

pytestmark = pytest.mark.gpu

A, T = cc.A, sr.T
JUNK, SENT, SEQ, SEQ2 = -5, -7.0, 11.0, 12.0
PAR = dict(vlo=sr.VLO, vhi=sr.VHI, kadd=cc.KADD, kappa=cc.KAPPA, delta=cc.DELTA, scale=cc.SCALE, eps=cc.EPS,
           max_pivots=cc.MAX_PIVOTS)
GEOS = list(cc.GEOMETRY)
FORMS = [(4, True), (4, False), (1, True), (1, False)]         # (es, previous lists given)


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _junk(shape, dtype=None, value=JUNK):
    import torch
    return torch.full(shape, value, dtype=dtype or torch.float64, device="cuda:0")


def _sums4(pnq):
    """double[3][m][T] -> the folded sweep's double[T][m][4] = {p, N, q, 0}"""
    out = np.zeros((pnq.shape[2], pnq.shape[1], 4))
    out[:, :, :3] = pnq.transpose(2, 1, 0)
    return out


def _device(m, forest, y, pnq, R, pci, pcc, par):
    from revs_admm_amd import _lib
    from revs_admm_amd.feeder import feeder_tree
    tr = feeder_tree(*forest, np.ones(m, bool))
    keep = (_up(tr["pack"].view(np.int64)), _up(tr["w"]))
    return dict(m=m, tree=_lib.Tree(tr["n"], keep[0].data_ptr(), keep[1].data_ptr()), keep=keep, y=_up(y), pnq1=_up(pnq),
                pnq4=_up(_sums4(pnq)), R=_up(R), pci=_up(pci), pcc=_up(pcc), par=par, y_host=np.asarray(y))


@functools.lru_cache(maxsize=None)
def _dev(geo):
    c = cc.case(geo)
    return _device(c["m"], c["forest"], c["y"], c["pnq"], c["R"], c["prev_cidx"], c["prev_ccnt"], PAR)


def _side_buffers(m):
    import torch
    return dict(vfull=_junk((m, T)), viol=_junk((m, T)), partial=_junk((T, 4)), cidx=_junk((T, A), torch.int64),
                ccnt=_junk((T,), torch.int32), cval=_junk((T, 3, A)), stats=_junk((T, 8)))


def _side(b, pnq, y, seq, es):
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import ptr
    return _lib.ChainKvSide(ptr(pnq), ptr(y), ptr(b["vfull"]), ptr(b["viol"]), ptr(b["partial"]), ptr(b["cidx"]),
                            ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]), seq, es, 0)


def _model_buffers(m):
    import torch
    return dict(k_full=_junk((T, A, A)), yhat=_junk((T, A)), info=_junk((T,), torch.int32), y_trial=_junk((m, T), value=SENT),
                lin=_junk((T, 8)))


def _host(b):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items()}


def _launch(lib, d, es, prev, e2=None, clears=True, forward=True):
    """One launch; e2 = (y, pnq4) of the verdict half, or None.  Returns the step half's outputs and, with e2, the verdict
    half's (keys e2_*), fwd_src / fwd_dst and the two cleared arrays, all on the host."""
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import check, ptr
    m, par = d["m"], d["par"]
    b1, mo = _side_buffers(m), _model_buffers(m)
    sh = dict(sh_a=_junk((T * m,)), sh_b=_junk((T * m + 32 * T,)))
    c = _lib.ChainKv(m=m, T=T, kadd=par["kadd"], has_e2=0, tree=C.pointer(d["tree"]), vlo=par["vlo"], vhi=par["vhi"],
                     kappa=par["kappa"], delta=par["delta"], scale=par["scale"], eps=par["eps"], max_pivots=par["max_pivots"],
                     e1=_side(b1, d["pnq4"] if es == 4 else d["pnq1"], d["y"], SEQ, es), R=ptr(d["R"]), k_full=ptr(mo["k_full"]),
                     yhat=ptr(mo["yhat"]), info=ptr(mo["info"]), y_trial=ptr(mo["y_trial"]), lin_out=ptr(mo["lin"]),
                     sh_a=ptr(sh["sh_a"]), sh_b=ptr(sh["sh_b"]))
    if prev:
        c.prev_cidx, c.prev_ccnt = ptr(d["pci"]), ptr(d["pcc"])
    extra = {}
    if e2 is not None:
        b2 = _side_buffers(m)
        c.has_e2, c.e2 = 1, _side(b2, e2[1], e2[0], SEQ2, 4)
        extra.update({"e2_" + k: v for k, v in b2.items()})
        if clears:
            extra["clr0"], extra["clr1"] = _junk((4 * m * T + 8,)), _junk((4 * m * T + 8,))
            c.clr0, c.clr1 = ptr(extra["clr0"]), ptr(extra["clr1"])
        if forward:
            extra["fwd_src"] = torch.arange(T * 8, dtype=torch.float64, device="cuda:0").reshape(T, 8) + 0.5
            extra["fwd_dst"] = _junk((T, 8))
            c.fwd_src, c.fwd_dst = ptr(extra["fwd_src"]), ptr(extra["fwd_dst"])
    check(lib.revs_op_chain_kv(C.byref(c), None), "revs_op_chain_kv")
    out = _host({**b1, **mo, **sh, **extra})
    out["sh_tail"], out["sh_a"], out["sh_b"] = out["sh_b"][T * m:], out["sh_a"].reshape(T, m), out["sh_b"][:T * m].reshape(T, m)
    return out


def _parts(lib, d):
    """The same evaluation by the general loop's launches, on the planar sums."""
    from revs_admm_amd._lib import check, ptr
    m, par = d["m"], d["par"]
    b, mo = _side_buffers(m), _model_buffers(m)
    check(lib.revs_op_dual_rows_tree(m, T, C.byref(d["tree"]), ptr(d["pnq1"]), ptr(d["y"]), par["vlo"], par["vhi"], par["kadd"],
                                     ptr(b["vfull"]), ptr(b["viol"]), ptr(b["partial"]), None, ptr(b["cidx"]), ptr(b["ccnt"]),
                                     ptr(b["cval"]), ptr(b["stats"]), SEQ, 1, None), "revs_op_dual_rows_tree")
    check(lib.revs_op_dual_model_small(m, T, ptr(d["R"]), ptr(d["pnq1"][1]), ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]),
                                       par["kappa"], par["delta"], par["max_pivots"], ptr(mo["k_full"]), ptr(mo["yhat"]),
                                       ptr(mo["info"]), None), "revs_op_dual_model_small")
    check(lib.revs_op_dual_step_pending(T, ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(mo["yhat"]), ptr(b["stats"]),
                                        par["scale"], par["eps"], ptr(d["y"]), m, ptr(mo["y_trial"]), ptr(mo["lin"]), None),
          "revs_op_dual_step_pending")
    return _host({**b, **mo})


def _three_pass(lib, d, zero_rows=False):
    """revs_op_dual_tree_select_model_step: the three-pass chain's operator launch (zero_rows: vfull / viol start as
    zeros -- what a row without a position in the tree keeps, and the selection reads every row)"""
    import torch
    from revs_admm_amd._lib import check, ptr
    m, par = d["m"], d["par"]
    b, mo = _side_buffers(m), _model_buffers(m)
    if zero_rows:
        b["vfull"], b["viol"] = (torch.zeros(m, T, dtype=torch.float64, device="cuda:0") for _ in range(2))
    check(lib.revs_op_dual_tree_select_model_step(
        m, T, C.byref(d["tree"]), ptr(d["pnq1"]), ptr(d["y"]), par["vlo"], par["vhi"], par["kadd"], ptr(b["vfull"]),
        ptr(b["viol"]), ptr(b["partial"]), ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]), SEQ, ptr(d["R"]),
        par["kappa"], par["delta"], par["max_pivots"], ptr(mo["k_full"]), ptr(mo["yhat"]), ptr(mo["info"]), par["scale"],
        par["eps"], ptr(mo["y_trial"]), ptr(mo["lin"]), None), "revs_op_dual_tree_select_model_step")
    return _host({**b, **mo})


@functools.lru_cache(maxsize=None)
def _run(geo, es, prev):
    from revs_admm_amd import _lib
    return _launch(_lib.load(), _dev(geo), es, prev)


@functools.lru_cache(maxsize=None)
def _run_parts(geo):
    from revs_admm_amd import _lib
    return _parts(_lib.load(), _dev(geo))


def _off(got, want, names=cc.NAMES):
    """names of the columns (slots) in which two [T][...] arrays differ"""
    bad = (np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1)
    return [names[t] for t in np.flatnonzero(bad)]


SHARED = ("cidx", "ccnt", "cval", "partial", "k_full", "yhat", "info")


def _assert_same_outputs(g, p, on, y, what):
    """Two launches of the same evaluation: every output both write, bit for bit (y_trial: where the rows have a position
    in the tree -- the chain leaves the others alone, the parts copy all of y)."""
    for k in SHARED:
        assert np.array_equal(g[k], p[k]), (what, k, _off(g[k], p[k]))
    assert np.array_equal(g["stats"][:, [0, 1, 2, 3, 5]], p["stats"][:, [0, 1, 2, 3, 5]]), what
    assert np.array_equal(g["lin"][:, 0], p["lin"][:, 0]), (what, "lin", _off(g["lin"][:, 0], p["lin"][:, 0]))
    assert np.array_equal(g["y_trial"][on], p["y_trial"][on]), (what, "y_trial", _off(g["y_trial"][on].T, p["y_trial"][on].T))
    over8 = g["ccnt"] > 8
    assert (g["info"][over8] == -999).all() and np.array_equal(g["y_trial"][on][:, over8], y[on][:, over8]), what


# ---- (a) the step half against numpy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_step_half_against_the_restatement(gpu_lib, geo):
    c, e = cc.case(geo), cc.expected(geo)
    on, y = c["on"], c["y"]
    runs = {f: _run(geo, *f) for f in FORMS}
    for f, g in runs.items():
        for k in ("cidx", "ccnt", "cval"):
            assert np.array_equal(g[k], e[k]), (f, k, _off(g[k], e[k]))
        assert np.array_equal(g["partial"], e["sums"]), (f, _off(g["partial"], e["sums"]))
        assert np.array_equal(g["stats"][:, 0:4], e["sums"]), (f, _off(g["stats"][:, 0:4], e["sums"]))
        assert (g["stats"][:, 5] == SEQ).all() and (g["stats"][:, [4, 6, 7]] == JUNK).all(), f
        assert np.array_equal(g["info"], e["info"]), (f, _off(g["info"], e["info"]))
        for t in range(T):
            a = int(e["cnt"][t]) if e["cnt"][t] <= 8 else 0
            blk = np.full((A, A), float(JUNK))                   # (the top-left block, nothing else)
            blk[:a, :a] = e["K"][t, :a, :a]
            assert np.array_equal(g["k_full"][t], blk), (f, "k_full", cc.NAMES[t])
            # the model's answer: a solution of the LCP, and the restatement's to the tolerance the model's own test uses
            if 1 <= e["cnt"][t] <= 8:
                assert cc.lcp_ok(e, t, g["yhat"][t]), (f, "LCP", cc.NAMES[t])
                np.testing.assert_allclose(g["yhat"][t], e["yhat"][t], rtol=1e-5, atol=1e-6 * np.abs(e["yhat"][t]).max(),
                                           err_msg=cc.NAMES[t])
            else:
                assert np.array_equal(g["yhat"][t], e["cval"][t, 2]), (f, "yhat", cc.NAMES[t])
        # the trial: the sentinel survives where a row has no position; off the list it is y; on it, the step
        assert (g["y_trial"][~on] == SENT).all(), f
        listed = np.zeros(y.shape, bool)
        for t in range(T):
            listed[e["cidx"][t, :e["cnt"][t]], t] = True
        keep = on[:, None] & ~listed
        assert np.array_equal(g["y_trial"][keep], y[keep]), f
        for t in range(T):
            rows = e["cidx"][t, :e["cnt"][t]]
            want = g["yhat"][t, :e["cnt"][t]] if (e["alpha"][t] == 1.0 and e["cnt"][t] <= 8) else e["cval"][t, 2, :e["cnt"][t]]
            assert np.array_equal(g["y_trial"][rows, t], want), (f, "step", cc.NAMES[t])
        # the linear term of the launch's own step: the same products, summed in another order (gamma_cnt sum |terms|)
        for t in range(T):
            a, rows = int(e["cnt"][t]), e["cidx"][t, :e["cnt"][t]]
            terms = e["cval"][t, 1, :a] * (g["y_trial"][rows, t] - e["cval"][t, 2, :a])
            gam = a * 2.0 ** -53 / (1 - a * 2.0 ** -53)
            assert abs(g["lin"][t, 0] - terms.sum()) <= gam * np.abs(terms).sum(), (f, "lin", cc.NAMES[t])
        assert (g["lin"][:, 1:] == JUNK).all() and (g["sh_tail"] == JUNK).all(), f
    first = runs[FORMS[0]]
    for f, g in runs.items():
        for k in SHARED + ("y_trial", "lin", "sh_a", "sh_b"):
            a, b = (g[k].T, first[k].T) if k == "y_trial" else (g[k], first[k])
            assert np.array_equal(a, b), (f, k, _off(a, b))


# ---- (b) the step half against its parts -----------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_step_half_against_its_parts(gpu_lib, geo):
    c, p = cc.case(geo), _run_parts(geo)
    assert (p["stats"][:, 5] == SEQ).all()
    for f in FORMS:
        _assert_same_outputs(_run(geo, *f), p, c["on"], c["y"], f)


# ---- (c) the shifts --------------------------------------------------------------------------------------------------
def _fma_chain(R, rows, yv, nodes, kappa):
    """d = fma(R[row][node], y, d) over the rows in the order given, then d * (1 / kappa): the kernel's chain, every fma
    rounded once (exact rationals, rounded to nearest even by float())"""
    from fractions import Fraction
    out = np.zeros(len(nodes))
    for i, n in enumerate(nodes):
        d = 0.0
        for r, v in zip(rows, yv):
            d = float(Fraction(float(R[r, n])) * Fraction(float(v)) + Fraction(d))
        out[i] = d * (1.0 / kappa)
    return out


@pytest.mark.parametrize("geo", GEOS)
def test_shifts(gpu_lib, geo):
    """|err| <= gamma_(cnt + 1) sum |R y| / kappa with gamma_k = k u / (1 - k u), u = 2^-53: an fma chain of cnt terms and
    one multiply by 1 / kappa (exact here: kappa = 4; the bound does not use that).  The reference is a long-double
    product (2^-64), so its own error is 2^-11 of the bound's unit.  Beyond the bound, the ORDER of the two sums -- the
    next evaluation's home pass reproduces sh_b term for term -- by the same fma chains in exact rationals."""
    c, e = cc.case(geo), cc.expected(geo)
    g = _run(geo, 4, True)
    R, yt = c["R"].astype(np.longdouble), np.where(c["on"][:, None], g["y_trial"], 0.0).astype(np.longdouble)
    u = np.longdouble(2.0) ** -53
    for t in range(T):
        cnt = int(e["cnt"][t])
        rows = e["cidx"][t, :cnt]
        terms = R[rows] * yt[rows, t][:, None]
        ref, mag = terms.sum(axis=0) / cc.KAPPA, np.abs(terms).sum(axis=0) / cc.KAPPA
        gam = (cnt + 1) * u / (1 - (cnt + 1) * u)
        for k in ("sh_a", "sh_b"):
            err = np.abs(g[k][t].astype(np.longdouble) - ref)
            assert (err <= gam * mag).all(), (k, cc.NAMES[t], float(err.max()), float((gam * mag).max()))
        if e["same"][t]:
            assert np.array_equal(g["sh_a"][t], g["sh_b"][t]), cc.NAMES[t]
        if 1 <= cnt <= 8:       # the two summation orders themselves, on a spread of nodes (all of them up to 300)
            m = c["m"]
            nodes = np.arange(m) if m <= 300 else np.unique(np.r_[0:8, 248:264, m - 8:m, 0:m:19])
            yn = g["y_trial"][rows, t]
            carry = np.flatnonzero(yn != 0)
            asc = carry[np.argsort(rows[carry])]
            assert np.array_equal(g["sh_a"][t, nodes], _fma_chain(c["R"], rows, yn, nodes, cc.KAPPA)), ("list order", cc.NAMES[t])
            assert np.array_equal(g["sh_b"][t, nodes], _fma_chain(c["R"], rows[asc], yn[asc], nodes, cc.KAPPA)), \
                ("row order", cc.NAMES[t])
            assert bool(e["same"][t]) == bool((np.diff(rows[carry]) > 0).all()), cc.NAMES[t]
        if e["alpha"][t] == 0.0 or e["info"][t] == -999:          # integer trial multipliers: the shifts are exact
            assert (g["y_trial"][rows, t] == np.round(g["y_trial"][rows, t])).all()
            assert np.array_equal(g["sh_a"][t], e["sh_a"][t]) and np.array_equal(g["sh_b"][t], e["sh_b"][t]), cc.NAMES[t]
            assert np.array_equal(g["sh_a"][t].astype(np.longdouble), ref), cc.NAMES[t]
    t = cc.NAMES.index("empty")
    assert (g["sh_a"][t] == 0).all() and (g["sh_b"][t] == 0).all()


# ---- (d) both halves in one launch -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _verdict_case(geo):
    """The verdict half's evaluation: the SAME multipliers (they are on the same previous lists) on other node sums --
    the voltages and dual terms of another draw of the columns.  Returns its pnq and what restate() makes of it."""
    c, o = cc.case(geo), cc.build(geo, seed=1)
    on = c["on"]
    pnq = c["pnq"].copy()
    pnq[0][on] = o["pnq"][0][o["on"]]
    pnq[2] = o["pnq"][2]
    eff = pnq.copy()                            # (off the tree: no voltage, no dual term)
    eff[0], eff[2] = 0.0, np.where(on[:, None], pnq[2], 0.0)
    eff[0][on] = o["v"][o["on"]]                # (the tree form of the node sums: themselves on a forest of roots)
    return pnq, sr.restate(eff[0], c["y"], eff, sr.VLO, sr.VHI, cc.KADD, A)


@pytest.mark.parametrize("geo", GEOS)
def test_both_halves_in_one_launch(gpu_lib, geo):
    c, d = cc.case(geo), _dev(geo)
    pnq2, exp2 = _verdict_case(geo)
    assert c["m"] == 1 or not np.array_equal(exp2["cidx"], cc.expected(geo)["cidx"])
    alone = _run(geo, 4, True)
    m = c["m"]
    for clears, forward in ((True, True), (False, False)):
        g = _launch(gpu_lib, d, 4, True, e2=(d["y"], _up(_sums4(pnq2))), clears=clears, forward=forward)
        # the verdict half: lists, stats, partial sums of the other evaluation, its own tag
        for k in ("cidx", "ccnt", "cval"):
            assert np.array_equal(g["e2_" + k], exp2[k]), (k, _off(g["e2_" + k], exp2[k]))
        assert np.array_equal(g["e2_partial"], exp2["sums"]) and np.array_equal(g["e2_stats"][:, 0:4], exp2["sums"])
        assert (g["e2_stats"][:, 5] == SEQ2).all() and (g["e2_stats"][:, [4, 6, 7]] == JUNK).all()
        # the step half: what it leaves when launched alone (its tag by a plain store)
        for k in SHARED + ("stats", "y_trial", "lin", "sh_a", "sh_b", "sh_tail"):
            assert np.array_equal(g[k], alone[k]), (k, clears)
        if forward:
            assert np.array_equal(g["fwd_dst"][:, 0:4], g["fwd_src"][:, 0:4]) and (g["fwd_dst"][:, 4:] == JUNK).all()
        if clears:
            for k in ("clr0", "clr1"):
                assert (g[k][:4 * m * T] == 0).all() and (g[k][4 * m * T:] == JUNK).all(), k


# ---- (e) a real feeder -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feeder_dev(golden, feeder_R):
    """The 121144 feeder: feeder_tree on its 1126 residence rows with the junction nodes in between, and its own R
    (consistent with the tree); a synthetic state in which rows bind: node sums whose voltages cross bounds set at
    their own quantiles, three multipliers per slot (on the previous lists), integer counts of free residences."""
    import networkx as nx
    from revs_admm_amd.lpsolver import feeder_arrays
    z, fd = golden
    g = nx.Graph()
    for nid, lab in zip(z["node_id"], fd.label):
        g.add_node(int(nid), label=lab.decode())
    for u, v, r in zip(fd.edge_u, fd.edge_v, fd.edge_r):
        g.add_edge(int(z["node_id"][u]), int(z["node_id"][v]), r=float(r))
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    forest = feeder_arrays(g, res)
    Rn = np.ascontiguousarray(feeder_R)
    m = len(res)
    rng = np.random.default_rng(12)
    pnq = np.stack([rng.uniform(0.0, 4.0, (m, T)), rng.integers(0, 5, (m, T)).astype(np.float64), -rng.uniform(0.0, 30.0, (m, T))])
    ref = Rn @ pnq[0]
    par = dict(PAR, vhi=float(np.quantile(ref, 0.998)), vlo=float(np.quantile(ref, 0.001)), kadd=4, kappa=5.0)
    par["scale"] = par["vhi"]
    y, pci, pcc = np.zeros((m, T)), np.zeros((T, A), np.int64), np.zeros(T, np.int32)
    for t in range(T):
        n = t % 5
        rows = rng.choice(m, n + 1, replace=False)
        pci[t, :n + 1], pcc[t] = rows, n + 1                    # (one row of the list has lost its multiplier)
        y[rows[:n], t] = rng.normal(0, 200.0, n)
    d = _device(m, forest, y, pnq, Rn, pci, pcc, par)
    assert m == 1126 and m < d["tree"].n <= 2048
    return d


def test_the_golden_feeder_against_its_parts(gpu_lib, feeder_dev):
    d = feeder_dev
    p = _parts(gpu_lib, d)
    on = np.ones(d["m"], bool)
    assert (p["ccnt"] <= 8).all() and (p["ccnt"] >= 1).sum() >= 20 and len(set(p["ccnt"])) >= 4 and (p["info"] != -999).all()
    for f in FORMS:
        _assert_same_outputs(_launch(gpu_lib, d, *f), p, on, d["y_host"], f)


# ---- the three-pass chain's operator launch --------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["9", "257", "2048"] + list(cc.TREES))
def test_tree_select_model_step_against_its_parts(gpu_lib, geo):
    """revs_op_dual_tree_select_model_step == revs_op_dual_rows_tree(with_select) + revs_op_dual_model_small +
    revs_op_dual_step_pending, bit for bit; it does not stage the rows through LDS: vfull / viol are the restatement's.
    (cc.TREES: the same on a chain, a comb and a comb with split edges; split_edges2048 has rows off the tree.)"""
    c, e = cc.case(geo), cc.expected(geo)
    g, p = _three_pass(gpu_lib, _dev(geo), zero_rows=not c["on"].all()), _run_parts(geo)
    _assert_same_outputs(g, p, c["on"], c["y"], geo)
    assert np.array_equal(g["y_trial"], p["y_trial"])
    assert np.array_equal(g["vfull"], e["vfull"]) and np.array_equal(g["viol"], e["viol"])
    for k in ("cidx", "ccnt", "cval"):
        assert np.array_equal(g[k], e[k]), (k, _off(g[k], e[k]))
    assert np.array_equal(g["stats"][:, 0:4], e["sums"]) and (g["stats"][:, 5] == SEQ).all()


def test_tree_select_model_step_on_the_golden_feeder(gpu_lib, feeder_dev):
    g, p = _three_pass(gpu_lib, feeder_dev), _parts(gpu_lib, feeder_dev)
    _assert_same_outputs(g, p, np.ones(feeder_dev["m"], bool), feeder_dev["y_host"], "feeder")
    assert np.array_equal(g["y_trial"], p["y_trial"])
