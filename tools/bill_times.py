#!/usr/bin/env python3
"""Times of the bill report:

    python tools/bill_times.py [--reps 30] [--sizes 10,36] [--rows-only] [--out FILE.json]

  (i)  revs_bill_rows on an ensemble's P_sch against revs_net_node_sums_many (load = NULL) on the SAME state: both read
       the n S T floats once; by HIP events, warm, the median of --reps launches, the two taking turns.  State bytes
       moved (4 n S T), bytes / time of both and the ratio of the times.
  (ii) AdmmEnsemble.bill_report (baseline "individual", EV residences, two pools, records only) against the host
       route -- result(), the individual optimum per scenario (engine.residence_solve, lpsolver.solve_residences'
       core), the numpy formula sum_t P c, numpy.percentile per scenario and per pool -- by the host clock, warm, the
       median and quartiles of --reps rounds, the sides taking turns.  --rows-only leaves (ii) out (a tuning build of
       the other row mapping, REVS_LIB=..., made with -DREVS_BILL_ROWS_DIRECT).

Cases: the 121144 feeder (community 2, 90 % adoption, 4.8 kW, T = 24, scenario s: the EV homes of seed 1234 + s) after a
2-iteration ensemble run, S from --sizes; and 100 000 synthetic residences on 2048 nodes, T = 96, S = 8, the schedules
set directly (no run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def golden_case(S):
    from ensemble_times import feeder_case
    from revs_admm_amd.engine import pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    cost, load, Rr, feeder, draw, (start, end) = feeder_case(24, False)
    n = load.shape[0]
    recs = [pack_homes(draw(1234 + s), 4.8, 20.0, 0.2, start, end) for s in range(S)]
    ens = AdmmEnsemble(cost, recs, load, np.arange(n), Rr, kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="relaxed",
                       feeder=feeder)
    ens.run(2)
    return "golden24", ens, recs, np.asarray(load, np.float32), np.asarray(cost, np.float32)


def synthetic_case(S=8, n=100_000, nodes=2048, T=96):
    import torch
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(n, T, n_nodes=nodes, seed=3, binary_feasible=False)
    cost, load = w.cost.astype(np.float32), w.load.astype(np.float32)
    ens = AdmmEnsemble(cost, [w.homes] * S, load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow,
                       vhigh=w.vhigh, mode="relaxed_exact", feeder=w.feeder)
    gen = torch.Generator(device=ens.dev).manual_seed(5)
    ens.P_sch.copy_(ens.load.view_as(ens.P_sch) * (0.8 + 0.4 * torch.rand(ens.P_sch.shape, generator=gen, device=ens.dev)))
    return "synthetic100k_T96", ens, [w.homes] * S, load, cost


def kernel_times(ens, reps):
    """(bill_rows ms, node_sums_many ms): medians of `reps` warm launches each, by events, taking turns."""
    import torch
    from revs_admm_amd._lib import check, ptr
    S, M, T, n = ens.S_count, ens.M, ens.T_slot, ens.n_res
    bill = torch.empty(S, n, dtype=torch.float64, device=ens.dev)
    sums = torch.empty(S, M, T, dtype=torch.float64, device=ens.dev)
    tariff = ens.cost.double()
    calls = {
        "bill_rows": lambda: check(ens.lib.revs_bill_rows(S, n, T, ptr(ens.P_sch), 0, T, S * T, ptr(tariff), ptr(bill),
                                                         ens.stream), "revs_bill_rows"),
        "node_sums_many": lambda: check(ens.lib.revs_net_node_sums_many(S, M, T, ptr(ens.node_ptr), None, ptr(ens.P_sch),
                                                                        ptr(sums), ens.stream), "revs_net_node_sums_many"),
    }
    ts = {k: [] for k in calls}
    for r in range(reps + 3):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 3:
                ts[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ts.items()}


def host_route(ens, recs, load, cost, groups):
    """The numbers of bill_report by way of the host -> (per-scenario quartiles (S, 5), per-pool quartiles)."""
    from revs_admm_amd.engine import residence_solve
    P = ens.result()[0]
    c = cost.astype(np.float64)
    S = len(recs)
    ind = np.stack([residence_solve(cost, recs[s], load, str(ens.dev))[2] for s in range(S)])
    C2, C1 = (P.astype(np.float64) * c).sum(-1), (ind.astype(np.float64) * c).sum(-1)
    with np.errstate(all="ignore"):
        dev = 100 * (C2 - C1) / C1
    ev = np.stack([r["ev"] != 0 for r in recs])
    q = [0, 25, 50, 75, 100]
    per = np.array([np.percentile(dev[s][ev[s] & np.isfinite(dev[s])], q) for s in range(S)])
    pool = [np.percentile(np.concatenate([dev[s][ev[s] & np.isfinite(dev[s])] for s in range(S) if groups[s] == g]), q)
            for g in range(max(groups) + 1)]
    return per, np.array(pool)


def time_case(name, ens, recs, load, cost, reps, rows_only):
    S, T, n = ens.S_count, ens.T_slot, ens.n_res
    k = kernel_times(ens, reps)
    nbytes = 4 * n * S * T
    row = {"case": name, "S": S, "residences": n, "T": T, "reps": reps, "lib": os.environ.get("REVS_LIB", "product"),
           "state_bytes": nbytes, "bill_rows_ms": k["bill_rows"], "node_sums_many_ms": k["node_sums_many"],
           "bill_rows_GBps": nbytes / k["bill_rows"] * 1e-6, "node_sums_many_GBps": nbytes / k["node_sums_many"] * 1e-6,
           "bill_rows_over_node_sums_many": k["bill_rows"] / k["node_sums_many"]}
    if rows_only:
        return row
    groups = [s % 2 for s in range(S)]

    def host():
        t0 = time.perf_counter()
        out = host_route(ens, recs, load, cost, groups)
        return 1e3 * (time.perf_counter() - t0), out

    def device():
        t0 = time.perf_counter()
        rep = ens.bill_report(groups=groups, arrays=False)
        return 1e3 * (time.perf_counter() - t0), rep

    sides = [("host", host), ("device", device)]
    warm = {s: fn()[1] for s, fn in sides}
    ts = {s: [] for s, _ in sides}
    for _ in range(reps):
        for s, fn in sides:
            ts[s].append(fn()[0])
    per, pool = warm["host"]
    rep = warm["device"]
    got = np.stack([rep.summary_dev[:S][f] for f in ("min", "q1", "median", "q3", "max")], axis=1)
    gotp = np.stack([rep.pooled_dev[f] for f in ("min", "q1", "median", "q3", "max")], axis=1)
    # (the host's formula sums a row pairwise, the device in slot order: the quartiles agree to rounding, not bit for bit)
    row["max_abs_quartile_device_minus_host"] = float(max(np.abs(got - per).max(), np.abs(gotp - pool).max()))
    for s, _ in sides:
        v = np.array(ts[s])
        row[f"{s}_ms"] = float(np.median(v))
        row[f"{s}_ms_iqr"] = [float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    row["device_over_host"] = row["device_ms"] / row["host_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="10,36")
    ap.add_argument("--rows-only", action="store_true")
    ap.add_argument("--no-synthetic", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bill_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    _lib.load()
    rows = []
    cases = [lambda S=int(s): golden_case(S) for s in a.sizes.split(",") if s]
    if not a.no_synthetic:
        cases.append(synthetic_case)
    for make in cases:
        rows.append(time_case(*make(), a.reps, a.rows_only))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
