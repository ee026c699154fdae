"""The price report's contract on the host (no GPU): the scans of the multipliers against the dense R y, the split of the
congestion payment into a rent per line, and the three statements against an LP solved by HiGHS -- the multipliers price
the nodes (reduced-cost signs), and s Y_e P_e is the derivative of the optimum in the weight of line e.

These tests check the mathematics on tests/price_ref.py, the restatement the GPU tests hold the kernel to; apart from
the last one, which reads PriceReport.reinforcement_value(), they need nothing of the feature and pass without it.  What
fails without the feature is tests/test_prices_abi.py and tests/test_gpu_prices.py."""
import numpy as np
import pytest

import headroom_ref as hr
import price_ref as pr
from test_attribution_host import random_forest

from revs_admm_amd.feeder import feeder_tree, headroom_aux

U = 2.0 ** -53


def forest(n, seed, zero_edges=True):
    """A random forest of n nodes (15 % zero-weight edges), 70 % of the nodes a row -> (tree, dense R by position, rng,
    rows)."""
    rng = np.random.default_rng(seed)
    parent, er = random_forest(n, rng)
    if not zero_edges:
        er = np.where(er == 0.0, 0.01, er)
    rows = np.flatnonzero(rng.random(n) < 0.7)
    cons = np.full(n, -1, np.int64)
    cons[rows] = np.arange(len(rows))
    tree = feeder_tree(parent, er, cons, np.ones(len(rows), bool))
    aux = headroom_aux(tree)
    return tree, hr.lca_matrix(aux["parent_pos"], aux["depth"], aux["wc"]), rng, len(rows)


def sparse_multipliers(rng, m, T, frac=0.05):
    """Signed multipliers on about `frac` of the rows (at least one)."""
    y = np.where(rng.random((m, T)) < frac, rng.normal(0.0, 1.0, (m, T)), 0.0)
    y[rng.integers(m), :] = 0.5
    return y


@pytest.mark.parametrize("n", [13, 300, 2056])
def test_scans_of_the_multipliers_are_the_dense_product(n):
    """d = the drop scan of w Y, Y the flow scan of y, is R y: within 4 n 2^-53 (R |y|), which covers any order of the at
    most n additions behind each entry (R >= 0)."""
    tree, R, rng, m = forest(n, n)
    mu = pr.gathered(tree, sparse_multipliers(rng, m, 3))
    Y, d = pr.walk(tree, mu)
    want, bound = R @ mu, 4.0 * tree["n"] * U * (R @ np.abs(mu))
    err = np.abs(d - want)
    print(f"forest of {n}: |d - R y| at most {err.max():.3e}, {np.max(err / np.maximum(bound, 1e-300)):.3e} of the bound")
    assert (err <= bound).all()
    # (Y is the sum of y over the subtree: 1_sub(e)^T y)
    end = np.asarray(tree["end"])
    sub = np.array([mu[j:end[j]].sum(axis=0) for j in range(tree["n"])])
    assert (np.abs(Y - sub) <= 4.0 * tree["n"] * U * np.array([np.abs(mu[j:end[j]]).sum(axis=0) for j in range(tree["n"])])).all()


@pytest.mark.parametrize("n", [13, 300, 2056])
def test_congestion_payment_splits_into_rents(n):
    """sum_e rent_e = sum_i inj_i cong_i = s sum_i y_i (R g)_i, each pair within 4 n 2^-53 sum |terms|; the contract's
    slot record carries the first two."""
    tree, R, rng, m = forest(n, n + 1)
    T, s = 3, 0.75
    inj = pr.gathered(tree, rng.uniform(-0.5, 4.0, (m, T)))
    mu = pr.gathered(tree, sparse_multipliers(rng, m, T))
    flow, drop = pr.walk(tree, inj)
    Y, d = pr.walk(tree, mu)
    b = pr.contract(tree, tree["n"], flow, drop, Y, d, np.zeros_like(d), inj, mu, s, np.full(T, 0.2), with_loss=False)
    w = np.asarray(tree["w"])[:, None]
    terms = [b["rent"], inj * b["cong"], s * mu * (R @ inj)]
    sums = [t.sum(axis=0) for t in terms]
    tol = 4.0 * tree["n"] * U * sum(np.abs(t).sum(axis=0) for t in terms)
    for a in range(3):
        for c in range(a + 1, 3):
            assert (np.abs(sums[a] - sums[c]) <= tol).all(), (a, c, sums[a], sums[c], tol)
    assert (np.abs(b["slot"]["rent_total"] - sums[0]) <= tol).all() and (np.abs(b["slot"]["cong_pay"] - sums[1]) <= tol).all()
    assert b["rent"].tobytes() == (((w * Y) * flow) * s + 0.0).tobytes()
    assert (b["slot"]["n_rows"] == (mu != 0).sum(axis=0)).all() and b["slot"]["n_bad"].sum() == 0
    assert (b["price"] == 0.2 + b["cong"]).all()


def solve_lp(w, tree, c, ub, hi):
    """min c x over 0 <= x <= ub, R(w) x <= hi with HiGHS -> (optimum, x, y >= 0: the rows' multipliers)."""
    from scipy.optimize import linprog
    n = tree["n"]
    end = np.asarray(tree["end"])
    sub = np.zeros((n, n))
    for j in range(n):
        sub[j, j:end[j]] = 1.0
    R = sub.T @ (w[:, None] * sub)                # sum_e w_e 1_sub(e) 1_sub(e)^T
    res = linprog(c, A_ub=R, b_ub=np.full(n, hi), bounds=list(zip(np.zeros(n), ub)), method="highs")
    assert res.status == 0, res.message
    return res.fun, res.x, -res.ineqlin.marginals, R


def test_lp_duals_are_prices_and_line_values():
    """A 16-node random tree, one slot, box-constrained draws that are paid for (c < 0 at most nodes) under R x <= hi.
    At least one row binds; the reduced costs c + d = c + R y have the sign of the bound x sits at; a forward difference
    of the optimum in every w_e (h = 1e-6) is Y_e P_e."""
    rng = np.random.default_rng(16)
    n = 16
    parent, er = random_forest(n, rng)
    er = np.where(er == 0.0, 0.02, er)
    tree = feeder_tree(parent, er, np.arange(n), np.ones(n, bool))
    assert tree["n"] == n
    w = np.asarray(tree["w"], np.float64)
    c = np.where(rng.random(n) < 0.8, -rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 0.5, n))
    ub = rng.uniform(1.0, 3.0, n)
    _, _, _, R = solve_lp(w, tree, c, ub, 1.0)
    hi = 0.6 * (R @ ub).max()
    opt, x, y, R = solve_lp(w, tree, c, ub, hi)
    binding = np.flatnonzero(y > 1e-9)
    assert len(binding) >= 1 and np.allclose((R @ x)[binding], hi, rtol=1e-9)
    # ---- the restatement on the LP's y and x
    flow, drop = pr.walk(tree, x[:, None])
    Y, d = pr.walk(tree, y[:, None])
    assert np.abs(d[:, 0] - R @ y).max() <= 4.0 * n * U * (R @ y).max()
    b = pr.contract(tree, n, flow, drop, Y, d, np.zeros_like(d), x[:, None], y[:, None], 1.0, np.zeros(1), with_loss=False)
    rc = c + b["cong"][:, 0]                       # the price a draw at node i faces, its own value included
    tol = 1e-7 * np.abs(c).max()
    at_lo, at_hi = x <= 1e-9, x >= ub - 1e-9
    assert (rc[at_lo] >= -tol).all() and (rc[at_hi] <= tol).all() and (np.abs(rc[~at_lo & ~at_hi]) <= tol).all()
    assert at_hi.any() and (~at_lo & ~at_hi).any()
    # (strong duality: the optimum is the Lagrangian at (x, y))
    assert abs(opt - (c @ x + y @ (R @ x - hi))) <= 1e-8 * abs(opt)
    assert abs(b["slot"]["rent_total"][0] - hi * y.sum()) <= 1e-8 * hi * y.sum()
    # ---- d optimum / d w_e = Y_e P_e
    value = b["rent"][:, 0] / w                    # s = 1
    assert np.allclose(value, Y[:, 0] * flow[:, 0], rtol=1e-14)
    h, worst = 1e-6, 0.0
    for e in range(n):
        wh = w.copy()
        wh[e] += h
        fd = (solve_lp(wh, tree, c, ub, hi)[0] - opt) / h
        if value[e] == 0.0:                        # (a line that carries no multiplier: the optimum does not move)
            assert abs(fd) <= 1e-4 * np.abs(value).max(), (e, fd)
            continue
        dev = abs(fd - value[e]) / abs(value[e])
        worst = max(worst, dev)
        assert dev <= 1e-4, (e, fd, value[e])
    print(f"{len(binding)} rows bind; forward differences against Y P: largest relative deviation {worst:.3e}")
    assert (value != 0.0).sum() >= 3


def test_reinforcement_value_is_the_lp_derivative_per_ohm():
    """PriceReport.reinforcement_value() on the restatement's Y and flow is 2 s Y P: d optimum / d r_e with w = 2 r."""
    from revs_admm_amd._lib import LOSS_LINE_DAY_DTYPE, PRICE_DAY_DTYPE, PRICE_NODE_DAY_DTYPE, PRICE_SLOT_DTYPE
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.prices import PriceReport
    tree, R, rng, m = forest(300, 5)
    flow, _ = pr.walk(tree, pr.gathered(tree, rng.uniform(-0.5, 4.0, (m, 2))))
    Y, _ = pr.walk(tree, pr.gathered(tree, sparse_multipliers(rng, m, 2)))
    z = lambda dt, k: np.zeros(k, dt)
    rep = PriceReport(None, None, None, Y, None, None, flow, z(SUMMARY_DTYPE, 2), z(PRICE_SLOT_DTYPE, 2),
                      z(PRICE_NODE_DAY_DTYPE, 1), z(LOSS_LINE_DAY_DTYPE, 1), np.zeros((), PRICE_DAY_DTYPE), 0.75, 1.0, 12.0)
    b = pr.contract(tree, tree["n"], flow, flow, Y, Y, Y, flow, Y, 0.75, np.ones(2), with_loss=False)
    w = np.asarray(tree["w"])[:, None]
    live = (w > 0) & np.ones_like(Y, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_ohm = 2.0 * b["rent"] / w
    assert np.allclose(rep.reinforcement_value()[live], per_ohm[live], rtol=1e-14, atol=0.0)
