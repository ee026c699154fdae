#!/usr/bin/env python3
"""Times of the statistics across scenarios (revs_net_across), warm, --calls repeats, the two
sides of the comparison alternating in one process:

    python tools/across_times.py [--calls 20] [--out FILE.json]

  device way     study_report_device(across=True, arrays=False): the report with the per-node / per-line records
                 made on the device; wall time of the whole call (host clock, ends in the read-back of the records)
  host way       what a user did before: study_report_device(arrays=True) -- the arrays read back -- then per group
                 numpy.percentile and numpy.mean along the scenario axis, the counts of violations and bands, the daily
                 extremes and their percentiles in numpy; wall time.  The kept nodes' voltages and the rated lines'
                 loadings must hold no NaN (asserted): numpy.percentile is the baseline, not the per-cell nanpercentile
  host way, nan  the same with numpy.nanpercentile / nanmean, what a user whose voltages may collapse to NaN needs:
                 named as such, timed with a quarter of the calls (it runs a Python function per cell)
  the launches   revs_net_across alone on the voltage array (all three outputs; and the slot records alone), HIP events
  bytes read     COMPUTED, not read from a counter: what the slot launch's loads ask for, from the values themselves --
                 every member's value once for the counts, once per selection round of its cell (the bits below the
                 prefix the cell's extremes share), once for the neighbours -- against one pass, S n T 8 bytes

on the 121144 feeder (T = 24; S = 5, 10, 36) and a 2048-node synthetic forest (T = 24; S = 36)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from network_times import forest, golden_feeder  # noqa: E402

BANDS = (0.92, 0.95, 0.98)


def spread(t):
    return dict(median=float(np.median(t)), q1=float(np.percentile(t, 25)), q3=float(np.percentile(t, 75)))


def monotone_key(v):
    u = (v + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def rounds_per_cell(values, members):
    """Selection rounds of every cell over `members`: the position of the highest bit in which the cell's smallest and
    largest key differ, plus one (0: all equal); cells with a NaN are counted over their numbers."""
    v = values[members]
    k = monotone_key(np.ascontiguousarray(v))
    ok = ~np.isnan(v)
    kmin = np.where(ok, k, np.uint64(2 ** 64 - 1)).min(axis=0)
    kmax = np.where(ok, k, np.uint64(0)).max(axis=0)
    x = np.where(ok.any(axis=0), kmin ^ kmax, np.uint64(0))
    rounds = np.zeros(x.shape, np.int64)              # the bit length of x, in integers (a float log2 rounds above 2^53)
    for shift in (32, 16, 8, 4, 2, 1):
        big = (x >> np.uint64(shift)) > 0
        rounds += np.where(big, shift, 0)
        x = np.where(big, x >> np.uint64(shift), x)
    return rounds + (x > 0)


def across_times(lib, name, feeder, M, T, S, G, calls, scale):
    import torch
    from revs_admm_amd._lib import ACROSS_DTYPE, check, ptr
    from revs_admm_amd.network import tree_on_device
    from revs_admm_amd.study import study_report_device
    par, er, cons = feeder
    n = len(par)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    node_g = torch.from_numpy(rng.uniform(0.0, scale, (S, M, T)) * rng.uniform(0.5, 1.0, (S, 1, 1))).to(dev)
    th, tree, _keep = tree_on_device(dev, par, er, cons, M)
    rating = np.where(rng.random(n) < 0.9, rng.uniform(50.0, 500.0, n), 0.0)
    nodes = np.sort(rng.choice(n, n // 4, replace=False))
    groups = np.arange(S) % G
    kw = dict(tree=(tree, th, n), groups=groups, rating=rating, nodes=nodes, bands=BANDS, vset=1.0)

    def device_way():
        return study_report_device(node_g, across=True, **kw)

    def host_way(pct=np.percentile, mean=np.mean):
        rep = study_report_device(node_g, arrays=True, **kw)
        out = []
        with np.errstate(invalid="ignore"):
            for a, keep, lo, hi, bands, sense in ((rep.volt, nodes, 0.95, 1.05, BANDS, -1),
                                                  (rep.loading, np.flatnonzero(rating > 0), -np.inf, 1.0, (0.8, 1.0), 1)):
                a = a[:, keep]
                assert not np.isnan(a).any(), "the baseline numpy.percentile needs arrays without NaNs"
                for g in range(G):
                    x = a[groups == g]
                    d = x.min(axis=2) if sense < 0 else x.max(axis=2)
                    for y in (x, d):
                        out.append(pct(y, [0, 25, 50, 75, 100], axis=0))
                        out.append(mean(y, axis=0))
                        out.append(((y < lo) | (y > hi)).sum(axis=0))
                        out.append(np.argmax(np.nan_to_num(np.fmax(lo - y, y - hi), nan=-np.inf), axis=0))
                        out.extend(((y <= b) if sense < 0 else (y >= b)).sum(axis=0) for b in bands)
        return out

    fns = [device_way, host_way]
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    wall = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6)
    r = {"case": name, "nodes": n, "T": T, "S": S, "G": G}
    for key, t in zip(("device_way_wall_us", "host_way_wall_us"), wall):
        r[key] = spread(t)
    r["ratio_device_over_host_way"] = r["device_way_wall_us"]["median"] / r["host_way_wall_us"]["median"]
    nan_way = []
    for _ in range(max(2, calls // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_way(np.nanpercentile, np.nanmean)
        torch.cuda.synchronize()
        nan_way.append((time.perf_counter() - t0) * 1e6)
    r["host_way_nanpercentile_wall_us"] = spread(nan_way)

    # ---- the across launches alone, on the voltage array of the same report
    rep = study_report_device(node_g, arrays=True, **kw)
    volt = torch.from_numpy(rep.volt).to(dev)
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    keep[torch.from_numpy(nodes).to(dev)] = 1
    slot = torch.empty(G * n * T * ACROSS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    daily = torch.empty(G * n * ACROSS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    expo = torch.empty(G, n, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.revs_net_across_scratch(S, n)) // 8, dtype=torch.float64, device=dev)
    hg = np.ascontiguousarray(groups, np.int32)
    hb = np.ascontiguousarray(BANDS, np.float64)
    st = torch.cuda.current_stream(dev).cuda_stream

    def launches(everything, kp):
        check(lib.revs_net_across(S, n, T, ptr(volt), ptr(kp), hg.ctypes.data, G, 0.95, 1.05, -1, hb.ctypes.data, 3,
                                  ptr(slot), ptr(daily) if everything else None, ptr(expo) if everything else None,
                                  ptr(scratch), st), "revs_net_across")

    variants = [("across_all_outputs_us", True, keep), ("across_slots_only_us", False, keep),
                ("across_slots_only_every_node_us", False, None)]
    for _ in range(5):
        for _, ev, kp in variants:
            launches(ev, kp)
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _ in variants}
    for _ in range(calls):
        for k, ev, kp in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launches(ev, kp)
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    for k in ts:
        r[k] = spread(ts[k])
    one_pass = S * n * T * 8
    read = 0
    rounds = []
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        rd = rounds_per_cell(rep.volt, mem)
        rounds.append(rd)
        read += int(((rd + 2) * len(mem) * 8).sum())
    r["one_pass_bytes"] = one_pass
    r["slots_every_node_bytes_computed"] = read
    r["slots_every_node_passes"] = read / one_pass
    r["selection_rounds_mean"] = float(np.mean(rounds))
    r["selection_rounds_max"] = int(np.max(rounds))
    r["slots_every_node_computed_GBps"] = read / (r["across_slots_only_every_node_us"]["median"] * 1e-6) / 1e9
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    from revs_admm_amd import _lib, build
    build.build()
    lib = _lib.load()
    gf = golden_feeder()
    rows = [across_times(lib, "121144 feeder", gf, 1126, 24, 5, 1, a.calls, 3.0),
            across_times(lib, "121144 feeder", gf, 1126, 24, 10, 2, a.calls, 3.0),
            across_times(lib, "121144 feeder", gf, 1126, 24, 36, 2, a.calls, 3.0),
            across_times(lib, "synthetic forest", forest(2048), 2048, 24, 36, 2, a.calls, 3.0)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
