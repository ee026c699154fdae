"""The transformer report's host side (no GPU): the owners read off the golden graph's labels, the sizing ladder, the
numpy restatement tests/xf_ref.py against closed forms, and the CSR the Python layer builds."""
import numpy as np
import pytest

import xf_ref as xr
from test_network_host import golden_graph


def test_rows_by_transformer_on_the_golden_graph(golden):
    """The 121144 feeder: 462 'T' nodes, every one of the 1126 homes owned, 215 transformers with a single home, the
    largest with 14 -- and the owner is the NEAREST 'T' node towards the substation, checked by walking up."""
    from revs_admm_amd.lpsolver import feeder_arrays
    from revs_admm_amd.transformers import rows_by_transformer
    g = golden_graph(golden)
    xf_nodes, xf_of = rows_by_transformer(g)
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    assert len(xf_nodes) == 462 and xf_of.shape == (1126,) == (len(res),) and (xf_of >= 0).all()
    homes = np.bincount(xf_of, minlength=462)
    assert (homes == 1).sum() == 215 and homes.max() == 14 and homes.sum() == 1126
    nonsub = [n for n in g.nodes if g.nodes[n]["label"] != "S"]
    parent, _, _ = feeder_arrays(g, res)
    pos = {n: i for i, n in enumerate(nonsub)}
    for h, k in list(zip(res, xf_of))[::37]:
        i = pos[h]
        while g.nodes[nonsub[i]]["label"] != "T":
            i = int(parent[i])
        assert nonsub[i] == xf_nodes[k]
    # another order of the residences gives the same owners, row by row
    again = rows_by_transformer(g, res[::-1])[1]
    assert (again == xf_of[::-1]).all()


def test_size_ratings_on_the_ladders_edges():
    from revs_admm_amd.transformers import STANDARD_KVA, size_ratings
    assert STANDARD_KVA == (5.0, 10.0, 15.0, 25.0, 37.5, 50.0, 75.0, 100.0, 167.0)
    pf = 0.95
    peak = np.array([0.0, 4.75, 4.7500001, 5.0 * pf, 10.0 * pf, 9.6, 167.0 * pf, 200.0, -9.6, 35.0])
    want = np.array([5.0, 5.0, 10.0, 5.0, 10.0, 15.0, 167.0, 167.0, 15.0, 37.5])
    assert (size_ratings(peak, pf) == want).all()
    assert (size_ratings([4.0], pf=1.0) == [5.0]).all() and (size_ratings([4.0], pf=1.0, margin=1.3) == [10.0]).all()
    assert (size_ratings([12.0, 80.0], pf=1.0, ladder=(10.0, 20.0)) == [20.0, 20.0]).all()
    # no transformer sized this way is above its rating under the load it was sized for, unless beyond the ladder
    load = np.random.default_rng(0).uniform(0.0, 150.0, 500)
    assert (load / (size_ratings(load, pf) * pf) <= 1.0).all()
    with pytest.raises(ValueError, match="ascending"):
        size_ratings([1.0], ladder=(10.0, 5.0))


def _constant(ratio, K=3, T=24, q=1, **kw):
    rated = np.full(K, 10.0)
    g = np.full((K, T), 10.0 * ratio)
    ptr, rows = xr.csr([[k] for k in range(K)])
    return xr.restate(g, ptr, rows, rated, np.full(T, 30.0), q=q, **kw)


def test_constant_load_sits_at_its_ultimate_rise():
    """Under the cyclic start a constant load gives top_oil = u_to in every slot (to the recursion's roundings), and at
    rated load the defaults give 30 + 55 + 25 = 110 degrees: faa = 1 exactly where the hot-spot is theta_ref."""
    for q in (1, 4):
        r = _constant(1.0, q=q)
        assert (r["ratio"] == 1.0).all() and (r["u_to"] == 55.0).all() and (r["u_w"] == 25.0).all()
        assert np.abs(r["top_oil"] - 55.0).max() <= 1e-12 and np.abs(r["hot"] - 110.0).max() <= 1e-12
    r = _constant(0.6)
    assert np.abs(r["top_oil"] - r["u_to"]).max() <= 1e-12 and (r["day"]["n_over_slots"] == 0).all()
    # faa = exp(0) = 1 where hot == theta_ref: decay 0 puts the state on the ultimate values without a rounding
    r = _constant(1.0, decay_to=0.0, decay_w=0.0)
    assert (r["hot"] == 110.0).all() and (r["faa"] == 1.0).all()
    assert (r["day"]["age_hours"] == 24.0).all() and (r["day"]["feqa"] == 1.0).all()
    assert r["fleet"]["n_aging"] == 0 and r["fleet"]["feqa_mean"] == 1.0
    assert r["fleet"]["lol_sum"] == 3 * 100.0 * 24.0 / 180000.0


def _varied(T=24, q=1, K=7, seed=5, **kw):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 6.0, (3 * K, T))
    ptr, rows = xr.csr([[3 * k, 3 * k + 1, 3 * k + 2] for k in range(K)])
    rated = rng.choice([5.0, 10.0], K) * 0.95
    return xr.restate(g, ptr, rows, rated, 25.0 + 5.0 * np.sin(np.arange(T)), q=q, **kw), g, ptr, rows, rated


def test_the_cyclic_day_closes_on_itself():
    """The state after the last sub-step is the state the day started from: each of the T q sub-steps adds at most
    6 U X to the error (xf_ref.propagated_bounds) and the start's division 1 / (1 - aN) scales what the first pass
    gathered -- 2e-14 K in the prototype at T = 24."""
    for T, q in ((24, 1), (24, 4), (96, 1)):
        r, *_ = _varied(T, q)
        d_to, _ = xr.decays(1.0, q)                        # (restate's default: slots of one hour)
        X = np.abs(r["u_to"]).max()
        bound = 2 * 6 * xr.U * X * T * q / (1.0 - d_to ** (T * q))
        assert np.abs(r["x_end"] - r["x0"]).max() <= bound and np.abs(r["y_end"] - r["y0"]).max() <= bound
        print(f"T={T} q={q}: closure {np.abs(r['x_end'] - r['x0']).max():.2e} K (bound {bound:.2e})")
    # a given start does not close
    r, *_ = _varied(24, 1, cyclic=0, to0=0.0, w0=0.0)
    assert np.abs(r["x_end"] - r["x0"]).min() > 1.0


def test_substeps_agree_with_a_finer_slot_grid():
    """q sub-steps per slot are the recursion on a grid of q T slots with every load repeated q times: top_oil and
    hot_spot at the slots' ends are the same bits, faa the mean of the finer grid's q values."""
    q, T = 4, 12
    r, g, ptr, rows, rated = _varied(T, q)
    d = xr.decays(1.0, q)
    amb = 25.0 + 5.0 * np.sin(np.arange(T))
    fine = xr.restate(np.repeat(g, q, axis=1), ptr, rows, rated, np.repeat(amb, q), slot_hours=1.0 / q, q=1,
                      decay_to=d[0], decay_w=d[1])
    assert np.array_equal(fine["top_oil"][:, q - 1::q], r["top_oil"]) and np.array_equal(fine["hot"][:, q - 1::q], r["hot"])
    mean = fine["faa"].reshape(-1, T, q)
    acc = mean[:, :, 0] * 0.0
    for s in range(q):
        acc = acc + mean[:, :, s]
    assert np.array_equal(acc / float(q), r["faa"])
    assert np.allclose(fine["day"]["age_hours"], r["day"]["age_hours"], rtol=1e-13, atol=0.0)


def test_bad_transformers_and_ties_in_the_restatement():
    g = np.ones((6, 3))
    g[1, 2] = np.nan
    ptr, rows = xr.csr([[0], [1, 2], [], [3], [6], [4, 5]])
    r = xr.restate(g, ptr, rows, np.array([1.0, 1.0, 1.0, 0.0, 1.0, 4.0]), np.full(3, 30.0))
    assert r["bad"].tolist() == [False, True, False, True, True, False]
    assert (r["load"][2] == 0).all() and (r["load"][4] == 0).all() and np.isnan(r["load"][1, 2]) and r["load"][1, 0] == 2.0
    assert np.isinf(r["ratio"][3]).all() and np.isnan(r["hot"][[1, 3, 4]]).all() and not np.isnan(r["hot"][[0, 2, 5]]).any()
    assert r["fleet"]["n_nan"] == 3 and np.isnan(r["fleet"]["lol_sum"]) and r["fleet"]["top_index"].tolist() == [0, 5, 2, -1, -1, -1, -1, -1]
    assert r["day"]["peak_ratio_slot"].tolist() == [0, -1, 0, -1, -1, 0] and r["summary_hot"][0]["n_nan"] == 3
    assert r["summary_ratio"][2]["n_nan"] == 1 and r["summary_ratio"][0]["worst_index"] == 3


def test_build_csr_orders_rows_by_transformer():
    from revs_admm_amd.transformers import build_csr
    ptr, rows = build_csr(np.array([2, -1, 0, 2, 0, 0]), 6, 4)
    assert ptr.tolist() == [0, 3, 3, 5, 5] and rows.tolist() == [2, 4, 5, 0, 3]
    assert ptr.dtype == rows.dtype == np.int32
