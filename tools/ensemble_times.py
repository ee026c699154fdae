#!/usr/bin/env python3
"""Times of S scenarios on one feeder, one engine after the other against one ensemble:

    python tools/ensemble_times.py [--reps 15] [--cases golden24,config3] [--out FILE.json]

  (a) sequential          S AdmmEngine runs with the feeder's matrix and tree formed once -- what lpsolver.solve_ADMM with
                          feeder= does per scenario, and what REVS.study(ensemble=False) runs
  (b) sequential, general the same with OperatorOptions(speculate=False, chain=False, fuse_home_pass=False): step() on its
                          general branch, as an ensemble's -- separates what batching gains from what the chained and
                          speculative fast paths gain
  (c) ensemble            one AdmmEnsemble over the S scenarios -- what lpsolver.solve_ADMM_many runs

on the 121144 feeder: community 2, 90 % adoption, 4.8 kW, 15 iterations, on/off chargers, T = 24, S = 1, 4, 10, 36 (scenario
s: the EV homes of seed 1234 + s), and config 3's shape (all communities, T = 96; S = 1, 4, 10).  Every side is an engine
built, run for 15 iterations and read back (result()); construction and run are timed separately, by the host clock
around work that ends in a device synchronise.  Warm (one untimed round of all three sides), then the median and quartiles
of --reps rounds, the three sides taking turns inside every round.  The dict <-> array conversions of the call surface
are the same work on every side and are left out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS = 15


def feeder_case(T, all_communities):
    """-> (cost, load, R_res, feeder, draw(seed) -> ev mask, (first, end) slot of the charging window) of the golden
    feeder at T slots."""
    import networkx as nx
    from oracle import revs_oracle as ro
    from revs_admm_amd.lpsolver import feeder_of
    z, fd = ro.load_golden(os.path.join(ROOT, "tests", "golden", "revs_121144.npz"))
    g = nx.Graph()
    for nid, lab in zip(z["node_id"], fd.label):
        g.add_node(int(nid), label=lab.decode())
    for u, v, r in zip(fd.edge_u, fd.edge_v, fd.edge_r):
        g.add_edge(int(z["node_id"][u]), int(z["node_id"][v]), r=float(r))
    assert [n for n in g if g.nodes[n]["label"] == "H"] == z["res_id"].tolist()
    Rr, feeder = feeder_of(g)                                   # formed once, shared by every side
    rep = T // 24
    assert rep * 24 == T
    res_ids = z["res_id"]
    pool = res_ids if all_communities else z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]
    idx = {int(h): i for i, h in enumerate(res_ids)}

    def draw(seed):
        np.random.seed(int(seed))                               # revs_fixture.py:175-177
        ev = np.zeros(len(res_ids), bool)
        ev[[idx[int(h)] for h in np.random.choice(pool, int(0.9 * len(pool)), replace=False)]] = True
        return ev

    load = np.repeat(z["LOAD"], rep, axis=1).astype(np.float32)
    cost = np.repeat(z["tariff_shift6"], rep).astype(np.float32)
    return cost, load, Rr, feeder, draw, (11 * rep, 23 * rep)


def time_case(name, T, all_communities, S, reps):
    import torch
    from revs_admm_amd.engine import AdmmEngine, OperatorOptions, pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    cost, load, Rr, feeder, draw, (start, end) = feeder_case(T, all_communities)
    n = load.shape[0]
    recs = [pack_homes(draw(1234 + s), 4.8, 20.0, 0.2, start, end) for s in range(S)]
    kw = dict(kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="binary", feeder=feeder)
    general = OperatorOptions(speculate=False, chain=False, fuse_home_pass=False)
    sync = lambda: torch.cuda.synchronize()

    def sequential(op):
        build = run = 0.0
        out = []
        for rec in recs:
            sync(); t0 = time.perf_counter()
            e = AdmmEngine(cost, rec, load, np.arange(n), Rr, op=op, **kw)
            sync(); t1 = time.perf_counter()
            e.run(ITERS)
            out.append(e.result()[0])
            sync(); t2 = time.perf_counter()
            build, run = build + t1 - t0, run + t2 - t1
            del e
        return build, run, np.stack(out)

    def ensemble():
        sync(); t0 = time.perf_counter()
        e = AdmmEnsemble(cost, recs, load, np.arange(n), Rr, **kw)
        sync(); t1 = time.perf_counter()
        e.run(ITERS)
        out = e.result()[0]
        sync(); t2 = time.perf_counter()
        evals = sum(e.op_iters_hist)
        del e
        return t1 - t0, t2 - t1, out, evals

    sides = [("sequential", lambda: sequential(None)), ("sequential_general", lambda: sequential(general)),
             ("ensemble", ensemble)]
    warm = {k: fn() for k, fn in sides}                          # code objects loaded, allocator warm
    ts = {k: [] for k, _ in sides}
    for _ in range(reps):
        for k, fn in sides:
            r = fn()
            ts[k].append((r[0] * 1e3, r[1] * 1e3))
    row = {"case": name, "T": T, "S": S, "residences": n, "iterations": ITERS, "reps": reps,
           "ensemble_operator_evaluations": warm["ensemble"][3],
           # on/off chargers: closed loops part at exactly tied optima; reported, not asserted
           "max_abs_P_sch_ensemble_minus_sequential_kw": float(np.abs(warm["ensemble"][2] - warm["sequential"][2]).max())}
    for k, _ in sides:
        a = np.array(ts[k])
        for j, part in enumerate(("build_ms", "run_ms")):
            row[f"{k}_{part}"] = float(np.median(a[:, j]))
            row[f"{k}_{part}_iqr"] = [float(np.percentile(a[:, j], 25)), float(np.percentile(a[:, j], 75))]
        row[f"{k}_total_ms"] = float(np.median(a.sum(axis=1)))
    row["ensemble_over_sequential_run"] = row["ensemble_run_ms"] / row["sequential_run_ms"]
    row["ensemble_over_sequential_total"] = row["ensemble_total_ms"] / row["sequential_total_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="golden24,config3")
    ap.add_argument("--sizes", default="", help="comma-separated S (default: 1,4,10,36 at T = 24; 1,4,10 at T = 96)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import build
    build.build()
    rows = []
    for case in a.cases.split(","):
        T, allc, sizes = (24, False, (1, 4, 10, 36)) if case == "golden24" else (96, True, (1, 4, 10))
        for S in ([int(s) for s in a.sizes.split(",")] if a.sizes else sizes):
            rows.append(time_case(case, T, allc, S, a.reps))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
