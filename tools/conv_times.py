#!/usr/bin/env python3
"""Times of the convergence report:

    python tools/conv_times.py [--homes 100000] [--iters 500] [--reps 3] [--report-reps 15] [--no-device] [--out FILE.json]

At the bench workload (100 000 residences x 24 slots on 2048 nodes, PDHG residences, --iters iterations from the zero
state, ONE engine, after a warm-up run of the same length), by the host clock around a synchronised call, the median of
--reps runs from reset():
  (none) run(history=False)
  (a)    run(history=True): the history is fetched, in the caller's order
  (b)    run(history="device")
and on the history (b) leaves:
  (c)    revs_conv_report alone (every output but the per-residence records / with them), by HIP events, the median of
         --report-reps calls; AdmmEngine.convergence_report by the host clock, records read back; and the copy of the
         history to the host that (a) pays, by the host clock.
The bytes the kernels read are counted here from the history itself: every selection workgroup walks its row once per
pass -- pass 0, the neighbour pass and the whisker pass always, three more digit passes when a quartile's rank does not
fall among the zeros, the flier pass when a value lies beyond the whiskers -- and the per-residence kernel walks the
history once.  --no-device skips (b) and (c): the script then runs on a commit without the report.
Then an ensemble of 8 scenarios x 12 500 residences (--ens-iters iterations): run(history=True) against
run(history="device") and its report, pooled in two groups."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return 1e3 * (time.perf_counter() - t0), out


def median_ms(fn, reps, sync, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        ts.append(clock(fn, sync)[0])
    return float(np.median(ts)), ts


def passes_of(hist, S):
    """(K, n S) float32 on the host -> selection passes over the history, in units of one read of it: the sum over
    (row, scenario) of the passes its workgroup makes, divided by K S (every scenario of a block shares its workgroup's
    walk, so a block makes the passes of its neediest scenario: counted per scenario here, an upper estimate for S > 1)."""
    K, cols = hist.shape
    n = cols // S
    total = 0
    for k in range(K):
        row = hist[k].reshape(n, S)
        for s in range(S):
            x = row[:, s].astype(np.float64)
            x = x[np.isfinite(x)]
            p = 3
            if x.size:
                neg, zero = int((x < 0).sum()), int((x == 0).sum())
                ranks = [((x.size - 1) * e) // 4 for e in (1, 2, 3)]
                if any(not (neg <= r < neg + zero) for r in ranks):
                    p += 3
                q1, q3 = np.percentile(x, [25, 75])
                lo, hi = q1 - 1.5 * (q3 - q1), q3 + 1.5 * (q3 - q1)
                if (x < lo).any() or (x > hi).any():
                    p += 1
            total += p
    return total / (K * S)


def report_events(lib, hist, S, eps, groups, reps, with_res):
    """revs_conv_report on a device history by HIP events -> median ms."""
    import torch
    from revs_admm_amd._lib import BILL_DTYPE, CONV_RES_DTYPE, CONV_RUN_DTYPE, check, ptr
    K, cols = hist.shape
    n = cols // S
    dev = hist.device
    G = 0 if groups is None else max(groups) + 1
    u8 = dict(dtype=torch.uint8, device=dev)
    d_iter = torch.empty(S * K * BILL_DTYPE.itemsize, **u8)
    d_pool = torch.empty(G * K * BILL_DTYPE.itemsize, **u8) if G else None
    d_res = torch.empty(S * n * CONV_RES_DTYPE.itemsize, **u8) if with_res else None
    d_run = torch.empty(S * CONV_RUN_DTYPE.itemsize, **u8)
    d_settle = torch.empty(S * BILL_DTYPE.itemsize, **u8)
    d_scratch = torch.empty(int(lib.revs_conv_report_scratch(S, n, K, G)) // 8 + 1, dtype=torch.float64, device=dev)
    hg = None if groups is None else np.ascontiguousarray(groups, np.int32)
    st = torch.cuda.current_stream(dev).cuda_stream
    ts = []
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        check(lib.revs_conv_report(S, n, K, ptr(hist), hist.stride(0), None, None, hg.ctypes.data if G else None, G, eps, 8,
                                   ptr(d_iter), ptr(d_pool), ptr(d_res), ptr(d_run), ptr(d_settle), ptr(d_scratch), st),
              "revs_conv_report")
        b.record()
        b.synchronize()
        if r >= 2:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def single(a, torch):
    from revs_admm_amd.engine import AdmmEngine, OperatorOptions
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(a.homes, 24, n_nodes=2048, seed=0, adoption=0.5, binary_feasible=False, stress=1.0)
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", node_counts=np.bincount(w.node_of, minlength=w.M), op=OperatorOptions(voltage="auto"),
                   feeder=w.feeder)
    sync = torch.cuda.synchronize
    e.run(a.iters, history=False)                              # warm-up
    row = {"case": "bench workload, one engine", "residences": a.homes, "T": 24, "iterations": a.iters, "reps": a.reps,
           "history_bytes": 4 * a.homes * a.iters}
    row["run_history_false_ms"], row["run_history_false_all_ms"] = median_ms(
        lambda: e.run(a.iters, history=False), a.reps, sync, e.reset)
    row["a_run_history_true_ms"], row["a_all_ms"] = median_ms(lambda: e.run(a.iters, history=True), a.reps, sync, e.reset)
    if a.no_device:
        return row
    row["b_run_history_device_ms"], row["b_all_ms"] = median_ms(
        lambda: e.run(a.iters, history="device"), a.reps, sync, e.reset)
    hist = e.diff_history
    host = hist.cpu().numpy()
    mx = host.max(axis=1)
    eps = float(np.median(mx))
    row["eps"] = eps
    row["zeros_fraction"] = float((host == 0).mean())
    row["c_report_records_only_events_ms"] = report_events(e.lib, hist, 1, eps, None, a.report_reps, False)
    row["c_report_with_residences_events_ms"] = report_events(e.lib, hist, 1, eps, None, a.report_reps, True)
    row["c_engine_convergence_report_host_clock_ms"] = median_ms(
        lambda: e.convergence_report(eps, arrays=False), a.report_reps, sync)[0]
    row["c_engine_convergence_report_with_residences_host_clock_ms"] = median_ms(
        lambda: e.convergence_report(eps), a.report_reps, sync)[0]
    row["history_copy_to_host_ms"] = median_ms(lambda: hist.cpu(), a.report_reps, sync)[0]
    p = passes_of(host, 1)
    row["selection_passes_per_row"] = p
    row["bytes_read_records_only"] = int(p * row["history_bytes"])
    row["bytes_read_with_residences"] = int((p + 1) * row["history_bytes"])
    row["records_only_GBps_of_bytes_read"] = row["bytes_read_records_only"] / row["c_report_records_only_events_ms"] * 1e-6
    rep = e.convergence_report(eps)
    row["report"] = {"converged_at": int(rep.run["converged_at"][0]), "last_above": int(rep.run["last_above"][0]),
                     "n_unsettled": int(rep.run["n_unsettled"][0]), "n_never": int(rep.run["n_never"][0]),
                     "settle_median": float(rep.settle["median"][0])}
    return row


def ensemble(a, torch):
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    S, n = 8, a.ens_homes
    w = make_workload(n, 24, n_nodes=256, seed=0, adoption=0.5, binary_feasible=False, stress=1.0)
    homes = [w.homes] + [make_workload(n, 24, n_nodes=256, seed=s, adoption=0.5, binary_feasible=False).homes
                         for s in range(1, S)]
    load, cost = w.load.astype(np.float32), w.cost.astype(np.float32)
    sync = torch.cuda.synchronize

    def make():
        return AdmmEnsemble(cost, homes, load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                            mode="relaxed_exact", feeder=w.feeder)
    make().run(2)                                             # warm-up
    row = {"case": "ensemble", "S": S, "residences": n, "T": 24, "iterations": a.ens_iters,
           "history_bytes": 4 * n * S * a.ens_iters}
    row["a_run_history_true_ms"] = clock(lambda: make().run(a.ens_iters), sync)[0]
    if a.no_device:
        return row
    e = make()
    row["b_run_history_device_ms"] = clock(lambda: e.run(a.ens_iters, history="device"), sync)[0]
    hist = e.diff_history
    host = hist.cpu().numpy()
    eps = float(np.median(host.reshape(a.ens_iters, n, S).max(axis=1)))
    groups = [s % 2 for s in range(S)]
    row["eps"], row["zeros_fraction"] = eps, float((host == 0).mean())
    row["c_report_records_only_events_ms"] = report_events(e.lib, hist, S, eps, None, a.report_reps, False)
    row["c_report_two_pools_events_ms"] = report_events(e.lib, hist, S, eps, groups, a.report_reps, False)
    row["c_report_two_pools_with_residences_events_ms"] = report_events(e.lib, hist, S, eps, groups, a.report_reps, True)
    row["c_ensemble_convergence_report_host_clock_ms"] = median_ms(
        lambda: e.convergence_report(eps, groups=groups, arrays=False), a.report_reps, sync)[0]
    row["history_copy_to_host_ms"] = median_ms(lambda: hist.cpu(), a.report_reps, sync)[0]
    row["selection_passes_per_row_upper_estimate"] = passes_of(host, S)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--homes", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--report-reps", type=int, default=15)
    ap.add_argument("--ens-homes", type=int, default=12_500)
    ap.add_argument("--ens-iters", type=int, default=100)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("conv_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    _lib.load()
    rows = []
    for case in (single,) if a.no_ensemble else (single, ensemble):
        rows.append(case(a, torch))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
