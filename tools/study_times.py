#!/usr/bin/env python3
"""Times of the study report, HIP events, warm, median of --calls calls, the sides of every
comparison alternating in one process:

    python tools/study_times.py [--calls 30] [--out FILE.json]

  per-schedule numbers  revs_net_study (summaries only: no pools, no bands) against S sequential
                        revs_net_report(arrays=False) calls on the same inputs -- the only way before the study report
  with bands            the same batched call with three band counts
  pooled numbers        revs_net_study with G pools against the only way before it: S revs_net_report calls with the
                        three arrays, their copies to the host and numpy.percentile over the pooled values there
  the pooling launch    its time as the difference (study with pools) - (study without); the staged bytes its passes
                        read and the share of the HBM peak (8.0 TB/s) that implies

on the 121144 feeder (T = 24; S = 1, 8, 36) and a 16 384-node synthetic forest (T = 96; S = 8)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from network_times import forest, golden_feeder  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s
POOL_PASSES = 11             # reads of every staged key by the pooling launch


def alternating_median_us(fns, calls):
    """Median (and spread: the quartiles) of every fn's time in microseconds, the fns taking turns call by call."""
    import torch
    for _ in range(5):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [dict(median=float(np.median(t)), q1=float(np.percentile(t, 25)), q3=float(np.percentile(t, 75))) for t in ts]


def study_times(lib, name, feeder, M, T, S, G, calls, host_side=True):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import check, ptr
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.study import POOLED_DTYPE
    par, er, cons = feeder
    th = feeder_tree(par, er, cons, np.ones(M, bool))
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    d_pack, d_w = up(th["pack"].view(np.int64)), up(th["w"])
    tree = _lib.Tree(th["n"], ptr(d_pack), ptr(d_w))
    n = len(par)
    real = th["order"] < n
    d_nop = up(np.where(real, th["order"], -1).astype(np.int32))
    d_rating = up(np.where(real, rng.uniform(50.0, 500.0, th["n"]), 0.0))
    g = up(rng.uniform(0.0, 3.0, (S, M, T)))
    out = [torch.empty(S, n, T, dtype=torch.float64, device=dev) for _ in range(3)]
    summ = torch.zeros(S * 2 * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    pool = torch.zeros(G * 2 * T * POOLED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    counts = torch.zeros(S, T, 3, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.revs_net_study_scratch(S, T, th["n"])) // 8, dtype=torch.int64, device=dev)
    group = np.ascontiguousarray(np.arange(S) % G, np.int32)
    band = np.array([0.92, 0.95, 0.98])
    st = torch.cuda.current_stream(dev).cuda_stream
    g_rows = [g[s] for s in range(S)]
    s_rows = [summ[s * 2 * T * 96:] for s in range(S)]

    def sequential(arrays):
        for s in range(S):
            o = [out[k][s] if arrays else None for k in range(3)]
            check(lib.revs_net_report(M, T, C.byref(tree), ptr(g_rows[s]), ptr(d_rating), None, ptr(d_nop), n, 1.0, 0.95,
                                      1.05, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(s_rows[s]), st))

    def study(pools, bands):
        check(lib.revs_net_study(S, M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0, 0.95, 1.05,
                                 group.ctypes.data if pools else None, G if pools else 0, band.ctypes.data if bands else None,
                                 3 if bands else 0, None, None, None, ptr(summ), ptr(pool) if pools else None,
                                 ptr(counts) if bands else None, ptr(scratch) if pools else None, st))

    def host_pooling():
        sequential(True)
        ld, v = out[1].cpu().numpy(), out[2].cpu().numpy()
        for gi in range(G):
            for a in (ld, v):
                x = a[group == gi].reshape(-1, T)
                np.nanpercentile(x, [25, 50, 75], axis=0)

    fns = [lambda: sequential(False), lambda: study(False, False), lambda: study(False, True), lambda: study(True, True)]
    keys = ["sequential_summaries_us", "study_us", "study_bands_us", "study_bands_pools_us"]
    if host_side:
        fns.append(host_pooling)
        keys.append("sequential_arrays_host_percentile_us")
    r = {"case": name, "nodes": n, "T": T, "S": S, "G": G}
    for k, t in zip(keys, alternating_median_us(fns, calls)):
        r[k], r[k + "_iqr"] = t["median"], [t["q1"], t["q3"]]
    r["ratio_study_over_sequential"] = r["study_us"] / r["sequential_summaries_us"]
    r["pooling_launch_us"] = r["study_bands_pools_us"] - r["study_bands_us"]
    r["pooling_bytes_read"] = POOL_PASSES * 2 * S * T * th["n"] * 8
    r["pooling_share_of_hbm_peak"] = r["pooling_bytes_read"] / (max(r["pooling_launch_us"], 1e-3) * 1e-6) / HBM_PEAK
    if host_side:
        r["ratio_pools_over_host_way"] = r["study_bands_pools_us"] / r["sequential_arrays_host_percentile_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    from revs_admm_amd import _lib, build
    build.build()
    lib = _lib.load()
    gf = golden_feeder()
    rows = [study_times(lib, "121144 feeder", gf, 1126, 24, 1, 1, a.calls),
            study_times(lib, "121144 feeder", gf, 1126, 24, 8, 2, a.calls),
            study_times(lib, "121144 feeder", gf, 1126, 24, 36, 6, a.calls),
            study_times(lib, "synthetic forest", forest(16384), 16384, 96, 8, 2, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
