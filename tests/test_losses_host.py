"""The loss report's contract on the host (no GPU): tests/losses_ref.py's contract() on the scans as feeder.tree_report_host
restates them agrees with its definition() from the dense F and R P within the bounds that 1e-12 x the largest entry
(test_gpu_network.py's BOUND on the scans) propagates -- random forests with zero-weight edges and exporting rows, the
121144 feeder under a stored schedule; the fixed-tree sum against math.fsum; the marginal loss factor as the derivative of
the total; a hand case with its numbers written out; the bad-slot rule."""
import math

import numpy as np
import pytest

import headroom_ref as hr
import losses_ref as lr
from test_gpu_network import BOUND, dense_of_forest, golden_net, synthetic_forest  # noqa: F401  (golden_net: a fixture)

from revs_admm_amd._lib import LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE
from revs_admm_amd.feeder import feeder_tree, tree_report_host


def setup(parent, edge_r, cons_of, p):
    """-> (tree, flow, drop, inj by preorder position: the scans restated by tree_report_host, n)."""
    n = len(parent)
    tree = feeder_tree(parent, edge_r, cons_of, np.ones(p.shape[0], bool))
    flow, drop = tree_report_host(tree, p, n)
    src = tree["src"]
    inj = np.where((src >= 0)[:, None], p[np.maximum(src, 0)], 0.0)
    return tree, hr.to_pos(tree, flow), hr.to_pos(tree, drop), inj, n


def random_forest(n, seed):
    rng = np.random.default_rng(1000 * n + seed)
    parent = np.full(n, -1, np.int64)
    for i in range(1, n):
        parent[i] = rng.integers(-1, i) if rng.random() < 0.85 else -1
    er = rng.uniform(0.5, 1.5, n)
    er[rng.random(n) < 0.15] = 0.0                              # zero-resistance edges
    rows = np.flatnonzero(rng.random(n) < 0.7)
    cons = np.full(n, -1, np.int64)
    cons[rows] = np.arange(len(rows))
    p = rng.uniform(-0.5, 1.0, (max(len(rows), 1), 3))          # (exporting rows: negative injections)
    return parent, er, cons, p, rng


def against_definition(tree, n, flow, drop, inj, F, RP, vset2):
    paths = lr.root_paths(lr.parent_positions(tree))
    d = lr.definition(tree["w"], F, RP, vset2, paths)
    b = lr.contract(tree, n, flow, drop, inj, vset2)
    b_loss, _, b_mlf = lr.propagated_bounds(tree["w"], F, RP, vset2, paths, BOUND)
    assert not b["bad"].any()
    print(f"loss err/bound {np.max(np.abs(b['loss'] - d['loss']) / np.maximum(b_loss, 1e-300)):.3e}, "
          f"mlf err/bound {np.max(np.abs(b['mlf'] - d['mlf']) / np.maximum(b_mlf, 1e-300)):.3e}")
    assert (np.abs(b["loss"] - d["loss"]) <= b_loss).all() and (np.abs(b["mlf"] - d["mlf"]) <= b_mlf).all()
    return b, d


@pytest.mark.parametrize("n", [1, 2, 13, 300])
def test_contract_agrees_with_definition_on_random_forests(n):
    for seed in range(3):
        parent, er, cons, p, rng = random_forest(n, seed)
        P = np.zeros((n, p.shape[1]))
        P[cons >= 0] = p[cons[cons >= 0]]
        F, RP = dense_of_forest(parent, er, P)
        s = 0.15 / np.abs(RP).max() if np.abs(RP).max() > 0 else 1.0     # (the deepest drop is 0.15 in size)
        tree, flow, drop, inj, _ = setup(parent, er, cons, p * s)
        b, d = against_definition(tree, n, flow, drop, inj, hr.to_pos(tree, F * s), hr.to_pos(tree, RP * s), 1.0)
        assert (b["loss"][tree["w"] == 0.0] == 0.0).all()        # a zero-resistance line loses exactly 0
        assert (b["loss"] >= 0.0).all()


def test_contract_agrees_with_definition_on_the_stored_feeder(golden, golden_net):
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    p = np.asarray(z["dis_a90_r4800_P_res"], np.float64)
    tree, flow, drop, inj, n = setup(par, er, cons, p)
    P = np.zeros((gn["n"], 24))
    P[gn["rows"]] = p
    F, RP = gn["to_node"](gn["A_inv"] @ P), gn["R"] @ P
    b, d = against_definition(tree, n, flow, drop, inj, hr.to_pos(tree, F), hr.to_pos(tree, RP), 1.0)
    assert b["slot"]["n_bad"].sum() == 0 and np.isfinite(b["day"]["energy"]) and b["day"]["energy"] > 0
    assert (b["day"]["top_index"] >= 0).all() and (np.diff(b["day"]["top_energy"]) <= 0).all()


def test_fixed_tree_sum_against_fsum():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 8, 13, 100, 1000, 4099):
        x = rng.uniform(-1.0, 1.0, (n, 2)) * 10.0 ** rng.integers(-6, 6, (n, 2))
        got = lr.tree_sum(x)
        for t in range(2):
            assert abs(got[t] - math.fsum(x[:, t])) <= n * 2.0 ** -53 * np.abs(x[:, t]).sum()
    e = 2.0 ** -53                                              # the tree's order, not the running sum's (which stays at 1)
    assert lr.tree_sum(np.array([[1.0], [e], [e], [e], [e]]))[0] == ((1.0 + e) + (e + e)) + ((e + 0.0) + (0.0 + 0.0)) == 1.0 + 2.0 ** -51


def test_mlf_is_the_derivative_of_the_total_with_den_frozen():
    """total(p + h e_i) - total(p) = h mlf_i + h^2 sum over i's root path of r / den, the flows of the path moved by h and
    every den kept: both sides from exact sums (math.fsum), compared to the roundings of their terms."""
    parent, er, cons = synthetic_forest(200, 9)
    rng = np.random.default_rng(9)
    p = rng.uniform(-0.2, 1.0, (200, 1))
    F, RP = dense_of_forest(parent, er, p)
    p *= 0.15 / np.abs(RP).max()
    tree, flow, drop, inj, n = setup(parent, er, cons, p)
    b = lr.contract(tree, n, flow, drop, inj, 1.0)
    paths = lr.root_paths(lr.parent_positions(tree))
    w, den, f0 = tree["w"], b["den"][:, 0], flow[:, 0]
    total = lambda f: math.fsum(0.5 * w * f * f / den)
    h = 2.0 ** -10
    for i in (0, 17, 101, 199):
        f1 = f0.copy()
        f1[paths[i]] += h
        lhs = total(f1) - total(f0)
        rhs = h * math.fsum(b["c"][paths[i], 0]) + h * h * math.fsum(0.5 * w[paths[i]] / den[paths[i]])
        tol = 8 * 2.0 ** -52 * (total(f1) + total(f0))
        assert abs(lhs - rhs) <= tol, (i, lhs, rhs, tol)
        assert abs(b["mlf"][i, 0] - math.fsum(b["c"][paths[i], 0])) <= 2 * tree["n"] * 2.0 ** -53 * np.abs(b["c"][:, 0]).sum()


def test_hand_case_chain_of_three_lines():
    """r = 0.5, 1, 2 (w = 1, 2, 4), injections 0.5, 0.25, 0.25, vset = 2: flows 1, 0.5, 0.25; w flow = 1, 1, 1; drops
    1, 2, 3; den 3, 2, 1; losses 1/6, 1/8, 1/8; c = 1/3, 1/2, 1; mlf = 1/3, 5/6, 11/6."""
    parent, er, cons = np.array([-1, 0, 1]), np.array([0.5, 1.0, 2.0]), np.arange(3)
    p = np.array([[0.5], [0.25], [0.25]])
    tree, flow, drop, inj, n = setup(parent, er, cons, p)
    assert flow[:3, 0].tolist() == [1.0, 0.5, 0.25] and drop[:3, 0].tolist() == [1.0, 2.0, 3.0]
    b = lr.contract(tree, n, flow, drop, inj, 4.0, line_class=np.array([0, 1, 1, 2, 2, 2, 2, 2]), C=2, loss_max=0.15,
                    cost=[3.0], slot_hours=0.5)
    assert b["loss"][:, 0].tolist() == [0.16666666666666666, 0.125, 0.125, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert b["c"][:3, 0].tolist() == [0.3333333333333333, 0.5, 1.0]
    assert b["mlf"][:3, 0].tolist() == [0.3333333333333333, 0.8333333333333333, 1.8333333333333333]
    s = b["slot"]
    assert s["total"][0] == (0.16666666666666666 + 0.125) + 0.125 == 0.41666666666666663
    assert s["delivered"][0] == 1.0 and s["class_total"][0].tolist() == [0.16666666666666666, 0.25, 0.0, 0.0]
    assert s["mlf_max"][0] == 1.8333333333333333 and s["mlf_max_index"][0] == 2 and s["n_bad"][0] == 0
    r = b["summary"][0]
    assert (r["count"], r["n_nan"], r["n_violations"], r["worst_index"], r["worst_value"]) == (3, 0, 1, 0, 0.16666666666666666)
    assert b["line_day"]["energy"].tolist() == [0.08333333333333333, 0.0625, 0.0625]
    assert b["line_day"]["peak_slot"].tolist() == [0, 0, 0]
    d = b["day"]
    assert d["energy"] == 0.41666666666666663 * 0.5 and d["delivered"] == 0.5 and d["cost"] == (0.41666666666666663 * 3.0) * 0.5
    assert d["top_index"].tolist() == [0, 1, 2, -1, -1, -1, -1, -1]          # (the tie of lines 1 and 2: the lower index)
    assert d["top_energy"][:3].tolist() == [0.08333333333333333, 0.0625, 0.0625] and np.isnan(d["top_energy"][3:]).all()
    assert (d["peak"], d["peak_slot"], d["n_bad_slots"]) == (0.41666666666666663, 0, 0)


def test_restatement_records_mirror_the_library_records():
    """contract()'s slot, line-day and day records carry the fields of revs_loss_slot_t, revs_loss_line_day_t and
    revs_loss_day_t (their numpy mirrors in _lib.py), the reserved tails aside."""
    tree, flow, drop, inj, n = setup(np.array([-1, 0]), np.array([0.5, 0.5]), np.arange(2), np.array([[0.1], [0.1]]))
    b = lr.contract(tree, n, flow, drop, inj, 1.0)
    assert tuple(b["slot"]) == LOSS_SLOT_DTYPE.names
    assert set(b["line_day"]) == set(LOSS_LINE_DAY_DTYPE.names) - {"reserved"}
    assert set(b["day"]) == set(LOSS_DAY_DTYPE.names) - {"reserved"}
    assert b["slot"]["class_total"].shape == (1,) + LOSS_SLOT_DTYPE["class_total"].shape
    assert b["day"]["top_index"].shape == LOSS_DAY_DTYPE["top_index"].shape


def test_bad_slot_rule():
    """A non-finite injection, or den > 0 failing at a node: every loss, mlf and double of the slot record a NaN, the
    summary empty with every line in n_nan, n_bad 1 -- and the day's energy and peak with it."""
    parent, er, cons = np.array([-1, 0, 1, -1]), np.array([0.5, 1.0, 2.0, 1.0]), np.arange(4)
    p = np.array([[0.5, 0.5, np.nan, 0.5], [0.25, 0.25, 0.25, 0.25], [0.25, 0.5, 0.25, 0.25], [0.1, 0.1, 0.1, 0.1]])
    tree, flow, drop, inj, n = setup(parent, er, cons, p)       # (slot 1: the drop at node 2 is 1.25 + 1.5 + 2.0 > vset2 = 4)
    b = lr.contract(tree, n, flow, drop, inj, 4.0, cost=np.ones(4))
    assert drop[2, 1] == 4.75 and b["bad"].tolist() == [False, True, True, False]
    for t in (1, 2):
        assert np.isnan(b["loss"][:, t]).all() and np.isnan(b["mlf"][:, t]).all()
        s = b["slot"]
        assert np.isnan([s["total"][t], s["delivered"][t], s["mlf_max"][t]]).all() and np.isnan(s["class_total"][t]).all()
        assert s["mlf_max_index"][t] == -1 and s["n_bad"][t] == 1
        assert (b["summary"][t]["count"], b["summary"][t]["n_nan"], b["summary"][t]["box"]) == (0, 4, None)
    assert not np.isnan(b["loss"][:, [0, 3]]).any() and b["summary"][0]["count"] == 4
    d = b["day"]
    assert np.isnan([d["energy"], d["peak"], d["cost"]]).all() and d["peak_slot"] == -1 and d["n_bad_slots"] == 2
    assert np.isnan(b["line_day"]["energy"]).all() and (b["line_day"]["peak_slot"] == -1).all()
    assert (d["top_index"] == -1).all()
    # den == 0 exactly is bad as well: den > 0 must hold
    tree, flow, drop, inj, n = setup(np.array([-1]), np.array([2.0]), np.arange(1), np.array([[1.0]]))
    assert drop[0, 0] == 4.0 and lr.contract(tree, n, flow, drop, inj, 4.0)["bad"].tolist() == [True]
