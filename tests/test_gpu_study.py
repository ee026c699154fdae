"""The study report on the GPU (revs_net_study; study.study_report, REVS.study) against tests/study_ref.py: scenario s of
a batch is, bit for bit, revs_net_report of that schedule alone; a pool of one is the schedule; pooled records are
network_ref.summary over the concatenation of the group's kernel-produced arrays (counts, extremes, whiskers, worst
entry exact; quartiles within 2 ulps, check_summary's bar for the same np_lerp); band counts are numpy's `<=` on the
kernel's own voltages -- and, where no dense float64 voltage lies within 1e-9 of a threshold (asserted, never
skipped), on the dense form's too."""
import types

import numpy as np
import pytest

import study_ref as sr
from test_gpu_network import (_golden_dense, _lines, check_arrays, check_summary, dense_of_forest,  # noqa: F401
                              golden_net, synthetic_forest)

pytestmark = pytest.mark.gpu

TAGS = ("dis_a90_r4800", "ind_a90_r4800", "ind_a70_r4800", "ind_a90_r3600", "cen_a90_r4800")
BANDS = (0.92, 0.95, 0.98)


def scenario(rep, s):
    """Scenario s of a study as a NetworkReport-like object (check_arrays / check_summary read these fields)."""
    return types.SimpleNamespace(flow=rep.flow[s], loading=rep.loading[s], volt=rep.volt[s], vmin=rep.vmin, vmax=rep.vmax,
                                 summary_loading=rep.summary_loading[s], summary_volt=rep.summary_volt[s])


def check_batch_is_the_single_report(rep, par, er, cons, p, rating, nodes, vset, vmin=0.95, vmax=1.05):
    """Scenario s of the batch == report_for_tree of schedule s alone: arrays and summaries, every bit."""
    from revs_admm_amd.network import report_for_tree
    for s in range(len(p)):
        one = report_for_tree(par, er, cons, p[s], rating=rating, nodes=nodes, vset=vset, vmin=vmin, vmax=vmax)
        for k in ("flow", "loading", "volt"):
            assert getattr(one, k).tobytes() == getattr(rep, k)[s].tobytes(), (s, k)
        assert one.summary_loading.tobytes() == rep.summary_loading[s].tobytes(), s
        assert one.summary_volt.tobytes() == rep.summary_volt[s].tobytes(), s


def check_pools_of_one(rep):
    for g in range(rep.n_groups):
        members = np.flatnonzero(rep.groups == g)
        if len(members) == 1:
            s = members[0]
            for t in range(rep.summary_volt.shape[1]):
                assert sr.same_shared_fields(rep.pooled_volt[g, t], rep.summary_volt[s, t]), (g, t)
                assert sr.same_shared_fields(rep.pooled_loading[g, t], rep.summary_loading[s, t]), (g, t)
            ok = rep.pooled_volt[g]["count"] > 0
            assert (rep.pooled_volt[g]["worst_scenario"][ok] == s).all()


def same_study(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes()
               for k in ("summary_loading", "summary_volt", "pooled_loading", "pooled_volt", "band_counts"))


def test_golden_study(gpu_lib, golden, golden_net):
    """The reference's five stored results as five scenarios over community 2."""
    from revs_admm_amd.study import study_report
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    nodes = np.array([gn["nonsub"].index(h) for h in com])
    p = np.stack([z[t + "_P_res"] for t in TAGS])
    rep = study_report(par, er, cons, p, groups=[1, 0, 0, 0, 2], rating=gn["rating"], nodes=nodes, bands=BANDS,
                       vset=1.0, arrays=True)
    assert rep.volt.shape == (5, gn["n"], 24) and rep.band_counts.shape == (5, 24, 3) and rep.n_groups == 3
    dense_v = []
    for s in range(5):
        F, RP = _golden_dense(gn, p[s])
        check_arrays(scenario(rep, s), F, RP, gn["rating"], 1.0)
        check_summary(scenario(rep, s), gn["rating"], nodes, gn["n"])
        dense_v.append(np.sqrt(1.0 - RP))
    dense_v = np.stack(dense_v)
    check_batch_is_the_single_report(rep, par, er, cons, p, gn["rating"], nodes, 1.0)
    sr.check_pooled(rep, gn["rating"], nodes)
    sr.check_bands(rep, nodes)
    check_pools_of_one(rep)
    near = min(np.abs(dense_v[:, nodes] - b).min() for b in BANDS)
    print(f"nearest dense voltage to a threshold: {near:.3e}")
    assert near > 1e-9
    assert np.array_equal(rep.band_counts, sr.band_counts(dense_v, nodes, BANDS))
    c = {t: rep.band_counts[i, 20:23].tolist() for i, t in enumerate(TAGS)}
    print(c)
    assert c["ind_a90_r4800"][0][0] > 0 and c["dis_a90_r4800"][0][2] > 0 and np.sum(c["cen_a90_r4800"]) == 0
    # ind_a90_r4800 as a pool of its own (a scenario is in one pool per call)
    alone = study_report(par, er, cons, p, groups=[-1, 0, -1, -1, -1], rating=gn["rating"], nodes=nodes, bands=BANDS,
                         vset=1.0, arrays=True)
    check_pools_of_one(alone)
    assert alone.summary_volt.tobytes() == rep.summary_volt.tobytes() and np.array_equal(alone.band_counts, rep.band_counts)
    # the input is non-trivial: the pooled quartiles are none of the per-scenario ones
    for k in ("q1", "median", "q3"):
        assert (rep.summary_volt[k][1:4, 20] != rep.pooled_volt[k][0, 20]).all(), k
    assert rep.pooled_volt["count"][0, 20] == 3 * 297 and rep.pooled_loading["count"][0, 20] == 3 * 1691
    # the same bits from call to call; the summaries alone (no arrays)
    again = study_report(par, er, cons, p, groups=[1, 0, 0, 0, 2], rating=gn["rating"], nodes=nodes, bands=BANDS, vset=1.0)
    assert again.volt is None and same_study(rep, again)


def _midpoint_bands(dense_v, nodes, fractions=(0.05, 0.25, 0.60)):
    """Thresholds at midpoints between adjacent sorted dense voltages near the given ranks, none within 1e-9 of a value."""
    v = np.sort(dense_v[:, nodes].ravel())
    v = v[~np.isnan(v)]
    out = []
    for f in fractions:
        k = int(f * len(v))
        while v[k + 1] - v[k] < 1e-8:
            k += 1
        out.append(0.5 * (v[k] + v[k + 1]))
    return tuple(out)


@pytest.mark.parametrize("M", [2048, 4096, 8192, 16384])
def test_every_tree_shape(gpu_lib, M):
    """synthetic_forest at the four tree shapes, S = 5 with random load scalings, two pools and one scenario in none,
    unrated lines and a node mask as in test_kernel_matches_dense_form."""
    from revs_admm_amd.study import study_report
    rng = np.random.default_rng(21 + M)
    S, T = 5, {2048: 24, 4096: 12, 8192: 6}.get(M, 3)
    par, er, cons = synthetic_forest(M, seed=M)
    p = rng.uniform(0.0, 4.0, (S, M, T)) * rng.uniform(0.5, 1.0, (S, 1, 1))
    F, RP = dense_of_forest(par, er, np.concatenate(list(p), axis=1))
    scale = 0.15 / np.abs(RP).max()                 # (the deepest node of the heaviest scenario drops by 0.15)
    p, F, RP = p * scale, F * scale, RP * scale
    F, RP = F.reshape(M, S, T).transpose(1, 0, 2), RP.reshape(M, S, T).transpose(1, 0, 2)
    rating = rng.uniform(0.5, 2.0, M) * np.abs(F).max() / 3
    rating[rng.random(M) < 0.15] = np.nan           # unrated lines
    nodes = np.flatnonzero(rng.random(M) < 0.6)
    dense_v = np.sqrt(1.0 - RP)
    bands = _midpoint_bands(dense_v, nodes)
    near = min(np.abs(dense_v[:, nodes] - b).min() for b in bands)
    print(f"M={M}: bands {bands}, nearest dense voltage {near:.3e}")
    assert near > 1e-9
    groups = [0, 1, 0, -1, 1]
    rep = study_report(par, er, cons, p, groups=groups, rating=rating, nodes=nodes, bands=bands, vset=1.0, arrays=True)
    for s in range(S):
        check_arrays(scenario(rep, s), F[s], RP[s], rating, 1.0)
    check_batch_is_the_single_report(rep, par, er, cons, p, rating, nodes, 1.0)
    sr.check_pooled(rep, rating, nodes)
    sr.check_bands(rep, nodes)
    assert np.array_equal(rep.band_counts, sr.band_counts(dense_v, nodes, bands))
    frac = rep.band_counts.sum(axis=(0, 1)) / (S * T * len(nodes))
    assert np.abs(frac - (0.05, 0.25, 0.60)).max() < 0.01        # (the thresholds sit where they were put)
    assert (rep.pooled_volt["count"] == 2 * len(nodes)).all() and (rep.pooled_volt["n_nan"] == 0).all()
    only = study_report(par, er, cons, p, groups=groups, rating=rating, nodes=nodes, bands=bands, vset=1.0)
    assert only.flow is None and same_study(rep, only)


@pytest.mark.parametrize("case", ["ties", "nan", "few", "unrated", "no_groups", "unordered_bands"])
def test_edge_cases(gpu_lib, case):
    from revs_admm_amd.network import report_for_tree
    from revs_admm_amd.study import study_report
    rng = np.random.default_rng(5)
    M, T, S = 3000, 6, 3
    par, er, cons = synthetic_forest(M, seed=9)
    er = er * 4e-7                                  # (the deepest node then drops by ~0.1 under these loads)
    p = rng.uniform(0.0, 4.0, (S, M, T))
    rating = np.full(M, 3000.0)
    nodes, groups, bands = None, [0, 0, 1], (0.946, 0.97, 0.99)       # (the voltages span 0.944 .. 1)
    if case == "ties":
        p = np.round(p)
        p[1] = p[0]                                 # two identical schedules in pool 0
        p[:, :, 3] = 0.0                            # every value equal
    elif case == "nan":
        p[1, :, 1] *= 400.0                         # LinDistFlow collapses at the deep nodes of scenario 1, slots 1 and 4
        p[1, :, 4] *= 1e6
        rating[rng.random(M) < 0.2] = 0.0
    elif case == "few":
        nodes = np.array([2500])                    # pool 0: two voltages per slot, pool 1: one
        rating[:] = np.nan
        rating[17] = 25.0                           # pool 0: two loadings per slot
    elif case == "unrated":
        rating = None
    elif case == "no_groups":
        groups = None
    elif case == "unordered_bands":
        bands = (0.99, 0.90, 0.97, 0.946, 2.0, 0.0, 0.97, 0.95)       # eight, any order, a repeat, all / none
    rep = study_report(par, er, cons, p, groups=groups, rating=rating, nodes=nodes, bands=bands, arrays=True)
    check_batch_is_the_single_report(rep, par, er, cons, p, rating, nodes, 1.0)
    sr.check_pooled(rep, rating, nodes)
    sr.check_bands(rep, nodes)
    check_pools_of_one(rep)
    if case == "ties":
        one = report_for_tree(par, er, cons, p[0], rating=rating)
        for pool, single in ((rep.pooled_loading[0], one.summary_loading), (rep.pooled_volt[0], one.summary_volt)):
            for k in ("count", "n_fliers", "n_violations"):
                assert np.array_equal(pool[k], 2 * single[k]), k
            for k in ("min", "max", "whisker_lo", "whisker_hi", "worst_value"):
                assert pool[k].tobytes() == single[k].tobytes(), k
            assert (pool["worst_scenario"] == 0).all() and np.array_equal(pool["worst_index"], single["worst_index"])
        assert np.array_equal(rep.band_counts[0], rep.band_counts[1]) and rep.band_counts.max() > 0
        assert (rep.pooled_loading["max"][:, 3] == 0).all() and (rep.pooled_loading["n_fliers"][:, 3] == 0).all()
    if case == "nan":
        nn = rep.pooled_volt["n_nan"][0]
        assert nn[1] > 0 and nn[4] > 0 and nn[0] == 0
        assert np.array_equal(nn, rep.summary_volt["n_nan"][0] + rep.summary_volt["n_nan"][1])
        assert (rep.pooled_volt["count"][0] + nn == 2 * M).all()
        assert rep.pooled_volt["count"][0, 4] == M + (~np.isnan(rep.volt[1, :, 4])).sum()
        assert (rep.band_counts[1, 4] <= M - rep.summary_volt["n_nan"][1, 4]).all()
        assert (rep.pooled_volt["n_nan"][1] == 0).all()
    if case == "few":
        assert (rep.pooled_volt["count"][0] == 2).all() and (rep.pooled_volt["count"][1] == 1).all()
        assert (rep.pooled_loading["count"][0] == 2).all()
        three = study_report(par, er, cons, p, groups=[0, 0, 0], rating=rating, nodes=nodes, bands=bands, arrays=True)
        assert (three.pooled_volt["count"][0] == 3).all()
        sr.check_pooled(three, rating, nodes)
    if case == "unrated":
        pl = rep.pooled_loading
        assert (pl["count"] == 0).all() and np.isnan(pl["min"]).all() and np.isnan(pl["worst_value"]).all()
        assert (pl["worst_index"] == -1).all() and (pl["worst_scenario"] == -1).all() and (pl["n_nan"] == 0).all()
    if case == "no_groups":
        assert rep.n_groups == 0 and rep.pooled_volt.shape == (0, T) and rep.pooled_loading.shape == (0, T)
    if case == "unordered_bands":
        assert rep.band_counts.shape == (S, T, 8)
        assert (rep.band_counts[..., 4] == M).all() and (rep.band_counts[..., 5] == 0).all()
        assert np.array_equal(rep.band_counts[..., 2], rep.band_counts[..., 6])
        assert 0 < rep.band_counts[..., 3].sum() < rep.band_counts[..., 2].sum() < rep.band_counts[..., 0].sum()


def test_many_scenarios_and_groups(gpu_lib):
    """70 scenarios (more than one mask word) in 36 pools, among them pools of one and an id no scenario has."""
    from revs_admm_amd.study import study_report
    rng = np.random.default_rng(3)
    M, T, S = 600, 4, 70
    par, er, cons = synthetic_forest(M, seed=4)
    p = rng.uniform(0.0, 4.0, (S, M, T))
    groups = rng.integers(-1, 34, S)
    groups[groups == 7] = 8                          # pool 7 is empty
    groups[-1] = 35
    rep = study_report(par, er * 2e-6, cons, p, groups=groups, rating=np.full(M, 400.0), bands=(0.97,), arrays=True)
    assert rep.n_groups == 36 and (rep.pooled_volt["count"][7] == 0).all() and (rep.pooled_volt["worst_scenario"][7] == -1).all()
    sr.check_pooled(rep, np.full(M, 400.0), None)
    sr.check_bands(rep, None)
    check_pools_of_one(rep)


def _oracle_grid(z, com, feeder_R, grid):
    """The CPU oracle's schedules of the grid -> {(adoption, seed, method): P_res (n, T)}, on the inputs
    test_config0_15_iterations gives it (load and tariff as the float32 values the GPU holds)."""
    from helpers import f32
    from oracle import revs_oracle as ro
    idx = {int(h): i for i, h in enumerate(z["res_id"])}
    cost = f32(z["tariff_shift6"])
    out = {}
    for adoption, seed in grid:
        np.random.seed(seed)
        ev_homes = np.random.choice(com, int(adoption * 1e-2 * len(com)), replace=False)
        ev = np.zeros(len(idx), bool)
        ev[[idx[int(h)] for h in ev_homes]] = True
        oh = ro.Homes.uniform(f32(z["LOAD"]), ev, 4.8, 20.0, 0.2, 11, 23)
        out[adoption, seed, "distributed"] = ro.solve_ADMM(oh, feeder_R, np.arange(len(idx)), cost, 5.0, 15, 1.03, 0.95, 1.05,
                                                           mode="binary", util_method="dual")[1]
        out[adoption, seed, "individual"] = ro.solve_residence(cost, oh)[2]
    return out


def _direction(counts, pooled_volt):
    """The reference's result, as conditions on {(adoption, seed, method): counts (T, 3)} and {(method, adoption):
    pooled volt records (T,)}: the margins' left and right sides, for printing and asserting."""
    rows = []
    for seed in (1234, 56):
        d, i = counts[90, seed, "distributed"], counts[90, seed, "individual"]
        rows.append((f"seed {seed}: largest count at 0.95 over slots 20..22", d[20:23, 1].max(), i[20:23, 1].max()))
        rows.append((f"seed {seed}: count at 0.92 in slot 20", d[20, 0], i[20, 0]))
    pd, pi = pooled_volt["distributed", 90][20], pooled_volt["individual", 90][20]
    for k in ("whisker_lo", "q1", "min"):
        rows.append((f"pooled {k} at slot 20", pd[k], pi[k]))
    return rows


def _assert_direction(rows, who):
    for what, d, i in rows:
        print(f"{who}: {what}: distributed {d}, individual {i}")
    for seed_rows in (rows[0:2], rows[2:4]):
        assert seed_rows[0][1] < seed_rows[0][2], (who, seed_rows[0])
        assert seed_rows[1][1] == 0 and seed_rows[1][2] >= 8, (who, seed_rows[1])
    for what, d, i in rows[4:]:
        assert d > i, (who, what, d, i)


def test_the_grid_on_the_gpu(gpu_lib, golden, golden_net, feeder_R):
    """REVS.study on the golden feeder, community 2: adoptions (30, 90) x seeds (1234, 56) x both methods at 4800 W, 15
    iterations, pools by (method, adoption): 8 scenarios in 4 pools of two seeds.  Every record against the yard-stick
    on the run's own schedules; the direction of the reference's result (the distributed optimum keeps the community
    above the bands the individual one falls below) on the oracle's figures first, then on the GPU's.  The GPU's on/off
    closed loop parts from the oracle at exactly tied optima, and the stored individual result
    spreads its charging over slots 20..22 where the project's tie rule is the earlier slot: no run is compared with
    stored counts or with the oracle's number by number."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.extract import get_homes_ev_param
    from revs_admm_amd.revs_fixture import REVS
    z, gn = golden[0], golden_net
    ln = _lines()
    table = {s.decode(): float(r) for s, r in zip(ln["type_name"], ln["type_rating"])}
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    nodes = np.array([gn["nonsub"].index(h) for h in com])
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    labels, rep = fx.study(tariff, all_homes, dist, com, adoptions=(30, 90), ratings=(4800,), seeds=(1234, 56),
                           group_by=("method", "adoption"), max_iterations=15, v0=1.03, line_rating=table, arrays=True)
    assert labels == [dict(method=m, adoption=a, rating=4800, seed=s) for a in (30, 90) for s in (1234, 56)
                      for m in ("distributed", "individual")]
    assert rep.groups.tolist() == [0, 1, 0, 1, 2, 3, 2, 3] and rep.n_groups == 4
    key = {(l["adoption"], l["seed"], l["method"]): s for s, l in enumerate(labels)}
    pool = {("distributed", 30): 0, ("individual", 30): 1, ("distributed", 90): 2, ("individual", 90): 3}
    # the individual scenarios are get_individual_optimal's schedules: the same call
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    for (adoption, seed, method), s in key.items():
        if method == "individual":
            np.random.seed(seed)
            ev_homes = np.random.choice(com, int(adoption * 1e-2 * len(com)), replace=False)
            homes = get_homes_ev_param(all_homes, dist, ev_homes, 4.8, 20, 0.2, 11, 23)
            P_res = fx.get_individual_optimal(tariff, homes)[0]
            assert np.array([P_res[h] for h in res], np.float64).tobytes() == rep.node_p[s].tobytes(), (adoption, seed)
    # every record against the yard-stick on the run's own schedules
    dense_v = np.stack([np.sqrt(1.0 - _golden_dense(gn, rep.node_p[s])[1]) for s in range(8)])
    near = min(np.abs(dense_v[:, nodes] - b).min() for b in BANDS)
    print(f"nearest dense voltage to a threshold: {near:.3e}")
    assert near > 1e-9
    assert np.array_equal(rep.band_counts, sr.band_counts(dense_v, nodes, BANDS))
    sr.check_bands(rep, nodes)
    sr.check_pooled(rep, gn["rating"], nodes)
    assert (rep.pooled_volt["count"] == 2 * 297).all() and (rep.pooled_loading["count"] == 2 * 1691).all()
    for s in range(8):
        check_summary(scenario(rep, s), gn["rating"], nodes, gn["n"])
    # the direction of the reference's result: the oracle's figures first, with their margins
    orc = _oracle_grid(z, com, feeder_R, [(90, 1234), (90, 56)])
    o_keys = sorted(orc)
    o_volt = np.stack([np.sqrt(1.0 - _golden_dense(gn, orc[k])[1]) for k in o_keys])
    assert min(np.abs(o_volt[:, nodes] - b).min() for b in BANDS) > 1e-9
    o_counts = dict(zip(o_keys, sr.band_counts(o_volt, nodes, BANDS)))
    keep = sr.keep_masks(gn["n"], None, nodes)[1]
    o_pool = {}
    for m in ("distributed", "individual"):
        members = [i for i, k in enumerate(o_keys) if k[2] == m]
        recs = sr.pooled(o_volt, keep, members, "volt", 0.95, 1.05)
        o_pool[m, 90] = [r["box"] for r in recs]
    _assert_direction(_direction(o_counts, o_pool), "oracle")
    g_counts = {k: rep.band_counts[s] for k, s in key.items()}
    g_pool = {k: rep.pooled_volt[g] for k, g in pool.items()}
    for k, s in key.items():
        print(f"GPU {k}: counts at slots 20..22 {rep.band_counts[s, 20:23].tolist()}, lower whisker at 20 "
              f"{rep.summary_volt['whisker_lo'][s, 20]:.5f}")
    _assert_direction(_direction(g_counts, g_pool), "GPU")


def test_a_study_leaves_engines_alone(gpu_lib):
    """run_steps / network_report of engines created before a study give the same bits after it."""
    from helpers import f32
    from network_worker import line_ratings
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.study import study_report
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(4000, 24, seed=2, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    make = lambda: AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow,
                              vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    rating, nodes = line_ratings(w)
    a, b = make(), make()
    for e in (a, b):
        e.run(3)
        e.run_steps(10)
    state = lambda e: [x.copy() for x in e.get_state()] + [np.asarray(e.iteration)]
    assert all(np.array_equal(x, y) for x, y in zip(state(a), state(b)))
    before = b.network_report(rating=rating, nodes=nodes)
    a.run_steps(10)                                  # a: never sees a study between its steps
    ref = a.network_report(rating=rating, nodes=nodes)
    par, er, cons = w.feeder
    g = before.node_sums
    study_report(par, er, cons, np.stack([g, 0.5 * g, 2.0 * g]), groups=[0, 0, 1], rating=rating, nodes=nodes, arrays=True)
    again = b.network_report(rating=rating, nodes=nodes)
    for k in ("flow", "loading", "volt", "node_sums"):
        assert getattr(before, k).tobytes() == getattr(again, k).tobytes(), k
    assert before.summary_volt.tobytes() == again.summary_volt.tobytes()
    b.run_steps(10)
    assert all(np.array_equal(x, y) for x, y in zip(state(a), state(b)))
    after = b.network_report(rating=rating, nodes=nodes)
    assert after.volt.tobytes() == ref.volt.tobytes() and after.summary_loading.tobytes() == ref.summary_loading.tobytes()


def test_pool_with_a_datum_on_the_whisker_limit(gpu_lib):
    """test_gpu_network.test_datum_on_the_whisker_limit's feeder as a pool of two equal scenarios: every value twice,
    the same quartiles, the same limit -- the two largest loadings are the upper whisker, not fliers."""
    from revs_admm_amd.study import study_report
    from whisker_case import datum_on_the_upper_limit
    par, er, cons, p, rating, hival = datum_on_the_upper_limit()
    rep = study_report(par, er, cons, np.stack([p, p]), groups=[0, 0], rating=rating, bands=(), arrays=True)
    assert (rep.loading[:, 8, 0] == hival).all() and rep.loading[:, :8, 0].max() < hival
    g = rep.pooled_loading[0, 0]
    print(f"upper limit {hival!r}: pooled whisker_hi {g['whisker_hi']!r}, fliers {g['n_fliers']}")
    assert g["count"] == 18 and g["whisker_hi"] == hival
    assert g["n_fliers"] == int((rep.loading[:, :, 0] < g["whisker_lo"]).sum())
    sr.check_pooled(rep, rating, None)
    for s in range(2):
        check_summary(scenario(rep, s), rating, None, 9)


@pytest.mark.parametrize("M", [1, 2, 1025])
@pytest.mark.parametrize("case", ["all_equal", "first_digit"])
def test_pool_ranks_share_or_part(gpu_lib, M, case):
    """The pooled selection where the three ranks share a prefix through all eight digits (every value equal) and
    where they part at the first (loadings 2^120 apart; voltages of 0, 2^-18 and 1/2): star feeders of 1, 2 and 1025
    lines -- below, at and above one pass of the workgroup over a row -- three scenarios in pools of two and of one."""
    from revs_admm_amd.study import study_report
    rng = np.random.default_rng(40 + M)
    par, cons = np.full(M, -1, np.int64), np.arange(M)
    if case == "all_equal":
        p = np.full((3, M, 2), 1.25)
        er, rating = np.full(M, 2.0 ** -7), np.full(M, 2.0)      # (powers of two: every sum of the scans is exact)
    else:
        p = np.round(rng.uniform(0.5, 2.0, (3, M, 2)) * 1024.0) / 1024.0
        rating = 2.0 ** (120.0 * rng.integers(-1, 2, M))
        x = np.array([0.0, 2.0 ** -36, 0.25])[rng.integers(0, 3, M)]      # vset^2 - drop at scenario 0, slot 0
        er = (1.0 - x) / (2.0 * p[0, :, 0])
        p[1:] = p[0]                                 # (the same drops in every scenario)
        p[:, :, 1] = p[:, :, 0]
    rep = study_report(par, er, cons, p, groups=[0, 0, 1], rating=rating, bands=(), arrays=True)
    sr.check_pooled(rep, rating, None)
    check_pools_of_one(rep)
    assert (rep.pooled_loading["count"] == np.array([[2 * M] * 2, [M] * 2])).all()
    if case == "all_equal":
        for rec, val in ((rep.pooled_loading, rep.loading), (rep.pooled_volt, rep.volt)):
            for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi"):
                assert (rec[k] == val[0, 0, 0]).all(), k
            assert (rec["n_fliers"] == 0).all()
    elif M == 1025:
        top = lambda a: a.view(np.uint64) >> np.uint64(56)
        pl = rep.pooled_loading[0, 0]
        assert top(pl["q1"]) < top(pl["median"]) < top(pl["q3"])             # (they did part at the first digit)
