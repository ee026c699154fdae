"""The network report on the GPU (revs_net_node_sums, revs_net_report; AdmmEngine.network_report) against the dense
float64 restatement of the reference's formulas (tests/network_ref.py): flows, loading and voltages at every line
and node, the per-slot summaries against numpy.percentile / matplotlib's whisker rule applied to the kernel's own
arrays, the reference's stored results, the engine (state untouched), sharding (bit-identical), config 4.

Bounds.  flow and the drop vset^2 - volt^2 are sums of at most `nodes` terms of one sign pattern, compared with a dense
evaluation of the same sums in another order: 1e-12 x the largest entry, the bound test_tree_voltage_matches_dense_product
holds these sums to (BOUND).  loading = |flow| / rating carries that through one correctly rounded division:
BOUND max|F| / rating + 2^-52 |ref|.  volt = sqrt(x) with x within e = BOUND max|R P| of the dense x: |sqrt(x + e) - sqrt(x)| <=
e / (2 sqrt(x - e)), plus 2^-52 for the root's own rounding; entries with x <= 4 e are not compared (there the root magnifies
without bound), entries with x < -e must be NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import network_ref as nr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-12
U = 2.0 ** -52


def _lines():
    return np.load(os.path.join(HERE, "golden", "revs_121144_lines.npz"))


def synthetic_forest(M, seed):
    """A forest like synthetic.make_workload's (a few long laterals with short branches), every node a row -- without
    the dense M x M matrix that workload carries."""
    rng = np.random.default_rng(seed)
    parent = np.full(M, -1, np.int64)
    for i in range(1, M):
        parent[i] = rng.integers(max(0, i - 12), i) if rng.random() < 0.9 else rng.integers(0, i)
    parent[:max(1, M // 64)] = -1
    return parent, rng.uniform(0.5, 1.5, M), np.arange(M)


def dense_of_forest(parent, edge_r, P):
    """The dense formulas on the forest's graph: node M is the substation, edge k runs from k's parent to k."""
    M = len(parent)
    eu = np.where(parent < 0, M, parent)
    return nr.dense_solve(M + 1, eu, np.arange(M), edge_r, np.arange(M), P)


def check_arrays(rep, F, RP, rating, vset):
    """rep's flow / loading / volt (tree-node order; F signed towards the child) against the dense F and R P."""
    eF, eV = BOUND * np.abs(F).max(), BOUND * np.abs(RP).max()
    print(f"flow: max err {np.abs(rep.flow - F).max():.3e} (bound {eF:.3e})")
    assert np.abs(rep.flow - F).max() <= eF
    rated = np.isfinite(rating) & (rating > 0)
    assert np.isnan(rep.loading[~rated]).all()
    ref_ld = np.abs(F[rated]) / rating[rated, None]
    tol = eF / rating[rated, None] + U * ref_ld
    print(f"loading: max err/tol {(np.abs(rep.loading[rated] - ref_ld) / tol).max():.3e}")
    assert (np.abs(rep.loading[rated] - ref_ld) <= tol).all()
    x = vset * vset - RP
    assert np.isnan(rep.volt[x < -eV]).all() and not np.isnan(rep.volt[x > eV]).any()
    ok = ~np.isnan(rep.volt)
    drop = vset * vset - rep.volt[ok] ** 2
    print(f"drop: max err {np.abs(drop - RP[ok]).max():.3e} (bound {eV + 4 * U * vset * vset:.3e})")
    assert np.abs(drop - RP[ok]).max() <= eV + 4 * U * vset * vset      # (the root and the square: two roundings of <= vset^2)
    far = x > 4 * eV
    tolv = eV / (2.0 * np.sqrt(x[far] - eV)) + U * np.sqrt(x[far])
    assert (np.abs(rep.volt[far] - np.sqrt(x[far])) <= tolv).all()


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_summary(rep, rating, nodes, n_nodes):
    """The records == numpy.percentile / the whisker rule / the counts / the arg-extremes of the kernel's OWN arrays."""
    rated = np.zeros(n_nodes, bool) if rating is None else (np.isfinite(rating) & (rating > 0))
    keep = np.ones(n_nodes, bool)
    if nodes is not None:
        keep[:] = False
        keep[nodes] = True
    for rec, ref in ((rep.summary_loading, nr.summary(rep.loading, rated, "loading")),
                     (rep.summary_volt, nr.summary(rep.volt, keep, "volt", rep.vmin, rep.vmax))):
        for t, r in enumerate(ref):
            g = rec[t]
            assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"]) == \
                (r["count"], r["n_nan"], r["n_violations"], r["worst_index"]), (t, g, r)
            if r["count"] == 0:
                assert np.isnan(g["min"]) and np.isnan(g["median"]) and g["n_fliers"] == 0
                continue
            b = r["box"]
            for k in ("min", "max", "whisker_lo", "whisker_hi"):
                assert g[k] == b[k], (t, k, g[k], b[k])
            assert g["worst_value"] == r["worst_value"], (t, g, r)
            for k in ("q1", "median", "q3"):
                assert ulps(g[k], b[k]) <= 2, (t, k, g[k], b[k])
            assert g["n_fliers"] == b["n_fliers"], (t, g, b)


@pytest.fixture(scope="module")
def golden_net(golden):
    from test_network_host import golden_tree
    z, fd = golden
    g, res, nonsub, feeder, child, sign = golden_tree(golden)
    A_inv, R = nr.dense(fd.n_nodes, fd.edge_u, fd.edge_v, fd.edge_r, fd.nonsub())
    node_rating = np.zeros(len(nonsub))
    node_rating[child] = _lines()["edge_rating"]
    # the dense flows re-indexed by the tree node below each edge, signed towards it
    to_node = lambda F: (sign[:, None] * F)[np.argsort(child)]
    rows = np.flatnonzero(feeder[2] >= 0)[np.argsort(feeder[2][feeder[2] >= 0])]     # tree node of residence row r
    return dict(feeder=feeder, A_inv=A_inv, R=R, rating=node_rating, to_node=to_node, rows=rows, n=len(nonsub),
                res=res, nonsub=nonsub)


def _golden_dense(gn, p):
    P = np.zeros((gn["n"], p.shape[1]))
    P[gn["rows"]] = p
    return gn["to_node"](nr.flows(gn["A_inv"], P)), gn["R"] @ P


@pytest.mark.parametrize("case", ["golden24", "golden96", "synthetic2048", "synthetic4096", "synthetic8192",
                                  "synthetic12001", "synthetic16384"])
def test_kernel_matches_dense_form(gpu_lib, golden, golden_net, case):
    """flow, loading and volt at every line and node, all four tree shapes, with a node mask and unrated lines; and the
    summaries of the same call against numpy on the kernel's arrays."""
    from revs_admm_amd.network import report_for_tree
    rng = np.random.default_rng(21)
    if case.startswith("golden"):
        z, gn = golden[0], golden_net
        par, er, cons = gn["feeder"]
        p = z["dis_a90_r4800_P_res"] if case == "golden24" else rng.uniform(0.0, 2.5, (1126, 96))
        F, RP = _golden_dense(gn, p)
        rating = gn["rating"].copy()
        vset = 1.0
    else:
        M = int(case[len("synthetic"):])
        par, er, cons = synthetic_forest(M, seed=M)
        p = rng.uniform(0.0, 4.0, (M, {2048: 24, 4096: 12, 8192: 6}.get(M, 3)))
        F, RP = dense_of_forest(par, er, p)
        s = 0.15 / np.abs(RP).max()                 # (loads scaled so that the deepest node drops by 0.15: both are linear in p)
        p, F, RP = p * s, F * s, RP * s
        rating = rng.uniform(0.5, 2.0, M) * np.abs(F).max() / 3
        vset = 1.0
    n = len(par)
    rating[rng.random(n) < 0.15] = np.nan          # unrated lines
    nodes = np.flatnonzero(rng.random(n) < 0.6)
    rep = report_for_tree(par, er, cons, p, rating=rating, nodes=nodes, vset=vset, vmin=0.95, vmax=1.05)
    assert rep.flow.shape == rep.loading.shape == rep.volt.shape == (n, p.shape[1])
    check_arrays(rep, F, RP, rating, vset)
    check_summary(rep, rating, nodes, n)
    assert (rep.summary_volt["count"] == len(nodes)).all() and (rep.summary_volt["n_nan"] == 0).all()
    only = report_for_tree(par, er, cons, p, rating=rating, nodes=nodes, vset=vset, arrays=False)     # the summary alone
    assert only.flow is None and only.volt is None
    assert only.summary_loading.tobytes() == rep.summary_loading.tobytes()
    assert only.summary_volt.tobytes() == rep.summary_volt.tobytes()


@pytest.mark.parametrize("case", ["ties", "nan", "few", "unrated", "one"])
def test_summary_is_exact(gpu_lib, case):
    """Ties (leaves with equal loads and equal ratings), NaN voltages from a large input profile, a slot summary over
    fewer than four values, no rated line at all, a single value."""
    from revs_admm_amd.network import report_for_tree
    rng = np.random.default_rng(5)
    M, T = 3000, 6
    par, er, cons = synthetic_forest(M, seed=9)
    er = er * 4e-7                                  # (the deepest node then drops by ~0.1 under these loads)
    p = rng.uniform(0.0, 4.0, (M, T))
    rating = np.full(M, 3000.0)                     # (the largest flow is ~4650)
    nodes, vmin, vmax = None, 0.95, 1.05
    if case == "ties":
        p = np.round(p)                             # loads 0..4: many equal leaves, equal sums, zeros
        p[:, 2] = 1.0
        p[:, 3] = 0.0                               # every value equal (zero flow everywhere)
    elif case == "nan":
        p[:, 1] *= 400.0                            # LinDistFlow collapses at the deep nodes of slots 1 and 4
        p[:, 4] *= 1e6
        rating[rng.random(M) < 0.2] = 0.0
    elif case == "few":
        nodes = np.array([17, 2500, 4])             # three voltages per slot
        rating[:] = np.nan
        rating[[5, 77]] = 25.0                      # two loadings per slot
    elif case == "unrated":
        rating = None
    elif case == "one":
        nodes = np.array([1234])
        rating[:] = 0.0
        rating[99] = 10.0
    rep = report_for_tree(par, er, cons, p, rating=rating, nodes=nodes, vset=1.0, vmin=vmin, vmax=vmax)
    check_summary(rep, rating, nodes, M)
    if case == "nan":
        assert rep.summary_volt["n_nan"][1] > 0 and rep.summary_volt["n_nan"][4] > 0 and rep.summary_volt["n_nan"][0] == 0
        assert rep.summary_volt["count"][4] + rep.summary_volt["n_nan"][4] == M
        assert np.isnan(rep.volt[:, 4]).sum() == rep.summary_volt["n_nan"][4]
    if case == "ties":
        assert (rep.summary_loading["min"][3] == 0) and (rep.summary_loading["max"][3] == 0)
        assert rep.summary_loading["worst_index"][3] == 0 and rep.summary_loading["n_fliers"][3] == 0
    if case == "few":
        assert (rep.summary_volt["count"] == 3).all() and (rep.summary_loading["count"] == 2).all()
    if case == "unrated":
        assert np.isnan(rep.loading).all() and (rep.summary_loading["count"] == 0).all()
        assert (rep.summary_loading["worst_index"] == -1).all() and rep.worst_line is None
    if case == "one":
        assert (rep.summary_volt["worst_index"] == 1234).all() and (rep.summary_loading["worst_index"] == 99).all()
        assert np.array_equal(rep.summary_volt["median"], rep.volt[1234])


def test_datum_on_the_whisker_limit(gpu_lib):
    """numpy rounds 1.5 (q3 - q1) and then the sum: a loading equal to that limit is the upper whisker, not a flier."""
    from revs_admm_amd.network import report_for_tree
    from whisker_case import datum_on_the_upper_limit
    par, er, cons, p, rating, hival = datum_on_the_upper_limit()
    rep = report_for_tree(par, er, cons, p, rating=rating, vset=1.0)
    assert rep.loading[8, 0] == hival and rep.loading[:8, 0].max() < hival       # (the input is what it was made to be)
    b = nr.box_stats(rep.loading[:, 0])
    assert b["whisker_hi"] == hival and b["n_fliers"] == int((rep.loading[:, 0] < b["whisker_lo"]).sum())
    g = rep.summary_loading[0]
    print(f"upper limit {hival!r}: whisker_hi {g['whisker_hi']!r}, fliers {g['n_fliers']} (numpy {b['n_fliers']})")
    assert g["whisker_hi"] == hival and g["n_fliers"] == b["n_fliers"]
    check_summary(rep, rating, None, 9)


@pytest.mark.parametrize("tag", ["dis_a90_r4800", "cen_a90_r4800", "ind_a90_r4800"])
def test_stored_results_of_the_reference(gpu_lib, golden, golden_net, tag):
    """The report of the reference's own stored schedules: the dense restatement's figures (recomputed here, not
    hard-coded: largest loading 0.660 / 0.595 / 0.729, lowest voltage 0.8829, 171 / 136 / 196 node-slots below 0.95)."""
    from revs_admm_amd.network import report_for_tree
    z, gn = golden[0], golden_net
    p = z[tag + "_P_res"]
    F, RP = _golden_dense(gn, p)
    V = nr.volt(gn["R"], _rows(gn, p), 1.0)
    ld = np.abs(F) / gn["rating"][:, None]
    rep = report_for_tree(*gn["feeder"], p, rating=gn["rating"], vset=1.0, vmin=0.95, vmax=1.05)
    check_arrays(rep, F, RP, gn["rating"], 1.0)
    check_summary(rep, gn["rating"], None, gn["n"])
    print(f"{tag}: largest loading {ld.max():.4f}, lowest voltage {V.min():.4f}, below 0.95: {(V < 0.95).sum()}")
    assert not np.isnan(V).any() and 0.5 < ld.max() < 1.0 and (V < 0.95).sum() > 100     # (the inputs are non-trivial)
    assert abs(rep.summary_loading["max"].max() - ld.max()) <= BOUND * np.abs(F).max() / gn["rating"].min() + U
    assert rep.n_overloaded.sum() == (ld > 1).sum() == 0
    assert abs(rep.summary_volt["min"].min() - V.min()) <= 1e-12
    # (a voltage within rounding of the limit could be counted either way: none is)
    assert np.abs(V - 0.95).min() > 1e-9 and np.abs(V - 1.05).min() > 1e-9
    assert rep.n_voltage_violations.sum() == ((V < 0.95) | (V > 1.05)).sum()
    assert (rep.summary_volt["n_nan"] == 0).all()
    line, slot, val = rep.worst_line
    assert ld[line, slot] == ld.max() or abs(val - ld.max()) <= 1e-12
    node, slot, v = rep.worst_node
    assert abs(v - V.min()) <= 1e-12 and abs(V[node, slot] - V.min()) <= 1e-12


def _rows(gn, p):
    P = np.zeros((gn["n"], p.shape[1]))
    P[gn["rows"]] = p
    return P


def _state(e):
    return [x.copy() for x in e.get_state()] + [np.asarray(e.iteration)]


def _same_report(a, b):
    return (all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in ("flow", "loading", "volt", "node_sums"))
            and a.summary_loading.tobytes() == b.summary_loading.tobytes()
            and a.summary_volt.tobytes() == b.summary_volt.tobytes())


def test_engine_report_golden_feeder(gpu_lib, golden, golden_net, feeder_R):
    """After 15 iterations on the 121144 feeder: network_report() == the dense form of result()'s schedule + LOAD
    (float32 state widened to double); the run's state and iteration count keep their bits; a second call returns the
    same bits; at the residence rows the report's drop agrees with voltage() within float32 rounding of the latter."""
    from conftest import golden_homes
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine, pack_homes
    z, gn = golden[0], golden_net
    oh, evi = golden_homes(z, "dis_a90_r4800", 4.8)
    n, T = oh.LOAD.shape
    e = AdmmEngine(f32(z["tariff_shift6"]), pack_homes(oh.ev, 4.8, 20.0, 0.2, 11, 23), f32(oh.LOAD), np.arange(n),
                   feeder_R, kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="binary", feeder=gn["feeder"])
    e.run(15)
    P_sch = e.result()[0]
    before = _state(e)
    rep = e.network_report(rating=gn["rating"])
    again = e.network_report(rating=gn["rating"])
    after = _state(e)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert _same_report(rep, again)
    g = f32(oh.LOAD) + P_sch.astype(np.float64)
    assert np.array_equal(rep.node_sums, g)                         # (one residence per row: the sums are exact)
    F, RP = _golden_dense(gn, g)
    check_arrays(rep, F, RP, gn["rating"], 1.03)
    check_summary(rep, gn["rating"], None, gn["n"])
    assert (rep.vset, rep.vmin, rep.vmax) == (1.03, 0.95, 1.05)
    # voltage(): R32 @ (the f32 node sums of P_sch alone) on the matrix cores -- a dot product of K = 1126 non-negative
    # terms in float32: (K + 2) 2^-24 relative to the row's value, per the standard bound
    only = e.network_report(profile=e.P_sch)
    v32 = e.voltage().cpu().numpy().astype(np.float64)
    drop = (1.03 * 1.03 - only.volt ** 2)[gn["rows"]]
    assert np.abs(drop - v32).max() <= (n + 2) * 2.0 ** -24 * np.abs(v32).max()
    assert np.isnan(only.loading).all() and (only.summary_loading["count"] == 0).all()
    # a profile in the caller's order is the same profile
    assert _same_report(only, e.network_report(profile=P_sch))
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(e)))


def _sequential_node_sums(e, w, P_sch):
    """sum over every node's residences of (double) load + (double) p, in the engine's residence order, one at a time."""
    term = (w.load.astype(np.float32).astype(np.float64) + P_sch.astype(np.float64))[e.perm]
    node = np.asarray(w.node_of)[e.perm]
    first = np.concatenate([[0], np.flatnonzero(np.diff(node)) + 1])
    rank = np.arange(len(node)) - np.repeat(first, np.diff(np.concatenate([first, [len(node)]])))
    out = np.zeros((w.M, term.shape[1]))
    for k in range(int(rank.max()) + 1):
        out[node[rank == k]] += term[rank == k]
    return out


def test_engine_report_after_streaming_run(gpu_lib):
    """A synthetic 20 000 x 24 workload (2048 nodes, ~10 residences each) after a streaming run: node sums in the
    documented order bit for bit, the report against the dense form, the state untouched."""
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    from network_worker import line_ratings
    w = make_workload(20000, 24, seed=2, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run(3)
    e.run_steps(40)
    assert e.spec_hist[0] > 0, "the streaming steady state did not run"
    P_sch = e.result()[0]
    before = _state(e)
    rating, nodes = line_ratings(w)
    rep = e.network_report(rating=rating, nodes=nodes)
    assert _same_report(rep, e.network_report(rating=rating, nodes=nodes))
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(e)))
    g = _sequential_node_sums(e, w, P_sch)
    assert np.array_equal(rep.node_sums, g)
    F, RP = dense_of_forest(w.parent, w.edge_r, g)
    check_arrays(rep, F, RP, rating, w.vset)
    check_summary(rep, rating, nodes, w.M)
    e.run_steps(5)                                              # the loop goes on from the state the report left alone
    assert e.iteration == int(before[-1]) + 5


SHARD_CASE = dict(name="net", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=12)


def _one_rank(case):
    sys.path.insert(0, HERE)
    from network_worker import engine, reports
    from sharded_worker import make_case
    w = make_case(case)
    e = engine(w, 0, len(w.load), None, None)
    return reports(e, w, 0, len(w.load), case["steps"])


def _run_workers(tmp, specs):
    procs = []
    for i, spec in enumerate(specs):
        path = tmp / f"spec{i}.json"
        path.write_text(json.dumps(spec))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp / f"w{i}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "network_worker.py"), str(path)], stdout=log,
                                       stderr=subprocess.STDOUT, env=env), log))
    rcs = []
    for p, log in procs:
        try:
            rcs.append(p.wait(timeout=600))
        except subprocess.TimeoutExpired:
            p.kill()
            rcs.append(-9)
        log.close()
    logs = "\n".join((tmp / f"w{i}.log").read_text()[-3000:] for i in range(len(specs)))
    assert rcs == [0] * len(specs), logs


@pytest.mark.parametrize("layout", ["two_processes", "eight_logical_ranks"])
def test_sharded_report_is_bit_identical(gpu_lib, tmp_path, layout):
    """Residences sharded node-aligned over two processes (gloo) / eight logical ranks on one GPU: every rank's report
    -- of the schedule after 12 iterations of the real loop, and of a given profile -- equals the one-rank report in
    every bit (each node's sum is formed on one rank in the one-rank order; the all-reduce adds exact zeros)."""
    ref = _one_rank(SHARD_CASE)
    assert int(ref["iteration"]) == SHARD_CASE["steps"] and np.abs(ref["sch_flow"]).max() > 0
    if layout == "two_processes":
        port = 29900 + os.getpid() % 2000
        _run_workers(tmp_path, [dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE) for r in range(2)])
        files = [tmp_path / f"two_r{r}.npz" for r in range(2)]
    else:
        _run_workers(tmp_path, [dict(local=True, world=8, outdir=str(tmp_path), case=SHARD_CASE)])
        files = [tmp_path / f"local_r{r}.npz" for r in range(8)]
    for f in files:
        got = np.load(f)
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (f.name, k)


def test_config4_summary_only(gpu_lib):
    """1 000 000 residences x 96 slots on the 2048-node synthetic feeder: the summary alone (arrays=False), against the
    dense form applied to the node sums read back from the device."""
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    from network_worker import line_ratings
    w = make_workload(1_000_000, 96, seed=0, binary_feasible=False)
    assert w.M == 2048
    e = AdmmEngine(f32(w.cost), w.homes, f32(w.load), w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow,
                   vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    e.step()
    rating, nodes = line_ratings(w)
    rating *= 500.0                                             # (~490 residences below every node)
    rep = e.network_report(rating=rating, nodes=nodes, arrays=False)
    assert rep.flow is None and rep.loading is None and rep.volt is None
    g = rep.node_sums
    assert g.shape == (2048, 96) and g.min() > 0
    F, RP = dense_of_forest(w.parent, w.edge_r, g)
    rated = np.isfinite(rating)
    ld = np.full_like(F, np.nan)
    ld[rated] = np.abs(F[rated]) / rating[rated, None]
    V = np.sqrt(np.where(w.vset ** 2 - RP >= 0, w.vset ** 2 - RP, np.nan))
    eF, eV = BOUND * np.abs(F).max(), BOUND * np.abs(RP).max()
    keep = np.zeros(2048, bool)
    keep[nodes] = True
    for rec, ref, tol in ((rep.summary_loading, nr.summary(ld, rated, "loading"), eF / np.nanmin(rating) + U * np.nanmax(ld)),
                          (rep.summary_volt, nr.summary(V, keep, "volt", w.vlow, w.vhigh),
                           eV / (2 * np.sqrt(np.nanmin(w.vset ** 2 - RP[keep]) - eV)) + U * w.vset)):
        for t, r in enumerate(ref):
            got = rec[t]
            assert got["count"] == r["count"] and got["n_nan"] == r["n_nan"] == 0
            for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi"):
                # (an order statistic moves by no more than the data do; a quartile is a convex combination of two)
                assert abs(got[k] - r["box"][k]) <= tol + 4 * U, (t, k, got[k], r["box"][k], tol)
            assert abs(got["worst_value"] - r["worst_value"]) <= tol
    assert np.nanmin(w.vset ** 2 - RP[keep]) > 4 * eV
