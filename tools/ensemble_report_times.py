#!/usr/bin/env python3
"""Times of reporting on the S scenarios of an ensemble, through the host against on the device:

    python tools/ensemble_report_times.py [--reps 30] [--sizes 1,10,36] [--out FILE.json]

  (a) host      AdmmEnsemble.result() -- every schedule read back and put in the caller's order --, the (S, M, T)
                float64 node sums formed on the host, study.study_report (tree, upload, revs_net_study, records back)
  (b) device    AdmmEnsemble.study_report(): revs_net_node_sums_many on the state, revs_net_study on the engine's
                tree, records back

Both with two pools, three bands, rated lines, no arrays.  Beside them revs_net_node_sums_many alone by HIP events
(median of the same number of launches, warm) with the bytes it moves -- the residences' floats in, the doubles out --
over that time.

Cases: the 121144 feeder (community 2, 90 % adoption, 4.8 kW, on/off chargers, T = 24, scenario s: the EV homes of seed
1234 + s) after a 15-iteration ensemble run, S from --sizes; and one synthetic case where the sums are real work --
100 000 residences on 2048 nodes, T = 24, S = 8, the schedules set directly (no run).  Warm (one untimed round of both
sides), then the median and quartiles of --reps rounds by the host clock (each side ends in the read-back of its
records), the two sides taking turns call by call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ITERS = 15
BANDS = (0.92, 0.95, 0.98)


def golden_case(S):
    from ensemble_times import feeder_case
    from revs_admm_amd.engine import pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    cost, load, Rr, feeder, draw, (start, end) = feeder_case(24, False)
    n = load.shape[0]
    recs = [pack_homes(draw(1234 + s), 4.8, 20.0, 0.2, start, end) for s in range(S)]
    ens = AdmmEnsemble(cost, recs, load, np.arange(n), Rr, kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="binary",
                       feeder=feeder)
    ens.run(ITERS)
    return "golden24", ens, feeder, np.arange(n), ITERS


def synthetic_case(S, n=100_000, nodes=2048, T=24):
    import torch
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(n, T, n_nodes=nodes, seed=3, binary_feasible=False)
    ens = AdmmEnsemble(w.cost.astype(np.float32), [w.homes] * S, w.load.astype(np.float32), w.node_of, w.Rn, kappa=w.kappa,
                       vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="relaxed_exact", feeder=w.feeder)
    gen = torch.Generator(device=ens.dev).manual_seed(5)
    ens.P_sch.copy_(ens.load.view_as(ens.P_sch) * (0.8 + 0.4 * torch.rand(ens.P_sch.shape, generator=gen, device=ens.dev)))
    return "synthetic100k", ens, w.feeder, np.asarray(w.node_of), 0


def time_case(name, ens, feeder, node_of, iters, reps):
    import torch
    from revs_admm_amd import study
    from revs_admm_amd._lib import check, ptr
    S, M, T, n = ens.S_count, ens.M, ens.T_slot, ens.n_res
    par, er, cons = feeder
    rng = np.random.default_rng(1)
    rating = rng.uniform(50.0, 500.0, len(par))
    nodes = np.flatnonzero(rng.random(len(par)) < 0.7)
    groups = [s % 2 for s in range(S)] if S > 1 else [0]
    kw = dict(groups=groups, rating=rating, nodes=nodes, bands=BANDS, arrays=False)
    order = np.argsort(node_of, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(node_of, minlength=M))])[:-1]
    empty = np.bincount(node_of, minlength=M) == 0

    def host():
        t0 = time.perf_counter()
        P = ens.result()[0]
        if n == M and not empty.any() and np.array_equal(node_of, np.arange(n)):
            g = P.astype(np.float64)                                  # one residence per row: the schedules themselves
        else:
            g = np.zeros((S, M, T))
            g[:, ~empty] = np.add.reduceat(P[:, order].astype(np.float64), starts[~empty], axis=1)
        rep = study.study_report(par, er, cons, g, vset=ens.vset, vmin=ens.vlow, vmax=ens.vhigh, device=ens.dev, **kw)
        return 1e3 * (time.perf_counter() - t0), rep

    def device():
        t0 = time.perf_counter()
        rep = ens.study_report(**kw)
        return 1e3 * (time.perf_counter() - t0), rep

    sides = [("host", host), ("device", device)]
    warm = {k: fn()[1] for k, fn in sides}
    ts = {k: [] for k, _ in sides}
    for _ in range(reps):
        for k, fn in sides:
            ts[k].append(fn()[0])
    # the node-sum launch alone, by events
    out = torch.empty(S, M, T, dtype=torch.float64, device=ens.dev)
    ev = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        check(ens.lib.revs_net_node_sums_many(S, M, T, ptr(ens.node_ptr), None, ptr(ens.P_sch), ptr(out), ens.stream),
              "revs_net_node_sums_many")
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    kernel_ms = float(np.median(ev[3:]))
    nbytes = 4 * n * S * T + 8 * S * M * T + 8 * (M + 1)
    a, b = warm["host"], warm["device"]
    same = all(getattr(a, k).tobytes() == getattr(b, k).tobytes()
               for k in ("summary_loading", "summary_volt", "pooled_loading", "pooled_volt", "band_counts"))
    row = {"case": name, "S": S, "residences": n, "rows": M, "T": T, "tree_nodes": len(par), "iterations": iters,
           "reps": reps, "max_abs_node_sum_device_minus_host": float(np.abs(b.node_p - a.node_p).max()),
           "records_identical": bool(same), "node_sums_many_ms": kernel_ms, "node_sums_many_bytes": nbytes,
           "node_sums_many_GBps": nbytes / kernel_ms * 1e-6}
    for k, _ in sides:
        v = np.array(ts[k])
        row[f"{k}_ms"] = float(np.median(v))
        row[f"{k}_ms_iqr"] = [float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    row["device_over_host"] = row["device_ms"] / row["host_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="1,10,36")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_report_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import build
    build.build()
    rows = []
    cases = [lambda S=int(s): golden_case(S) for s in a.sizes.split(",") if s]
    cases.append(lambda: synthetic_case(8))
    for make in cases:
        rows.append(time_case(*make(), a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
