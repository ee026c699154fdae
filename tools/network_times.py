#!/usr/bin/env python3
"""Times of the network report, HIP events, warm, median of --calls calls:

    python tools/network_times.py [--calls 30] [--out FILE.json]

  revs_net_report   on the 121144 feeder (T = 24, 96) and on a 16 384-node synthetic forest (T = 96), with and without
                    the three arrays, beside revs_tree_voltage on the same tree and T (the same three scans, no
                    summary, one output) -- and their ratio
  revs_net_node_sums at 1 000 000 residences x 96 (2048 nodes), beside revs_aggregate_f32 on one profile"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_us(fn, calls):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def forest(M, seed=1):
    rng = np.random.default_rng(seed)
    parent = np.full(M, -1, np.int64)
    for i in range(1, M):
        parent[i] = rng.integers(max(0, i - 12), i) if rng.random() < 0.9 else rng.integers(0, i)
    parent[:max(1, M // 64)] = -1
    return parent, rng.uniform(0.5, 1.5, M) * 1e-7, np.arange(M)


def golden_feeder():
    import networkx as nx
    from oracle import revs_oracle as ro
    from revs_admm_amd.lpsolver import feeder_arrays
    z, fd = ro.load_golden(os.path.join(ROOT, "tests", "golden", "revs_121144.npz"))
    g = nx.Graph()
    for nid, lab in zip(z["node_id"], fd.label):
        g.add_node(int(nid), label=lab.decode())
    for u, v, r in zip(fd.edge_u, fd.edge_v, fd.edge_r):
        g.add_edge(int(z["node_id"][u]), int(z["node_id"][v]), r=float(r))
    return feeder_arrays(g, [n for n in g if g.nodes[n]["label"] == "H"])


def report_times(lib, name, feeder, M, T, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import check, ptr
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.network import SUMMARY_DTYPE
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
    g = up(rng.uniform(0.0, 3.0, (M, T)))
    out = [torch.empty(n, T, dtype=torch.float64, device=dev) for _ in range(3)]
    v = torch.zeros(M, T, dtype=torch.float64, device=dev)
    summ = torch.zeros(2 * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    full = lambda: check(lib.revs_net_report(M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0, 0.95,
                                             1.05, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(summ), st))
    summary = lambda: check(lib.revs_net_report(M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0,
                                                0.95, 1.05, None, None, None, ptr(summ), st))
    arrays = lambda: check(lib.revs_net_report(M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0,
                                               0.95, 1.05, ptr(out[0]), ptr(out[1]), ptr(out[2]), None, st))
    tv = lambda: check(lib.revs_tree_voltage(M, T, C.byref(tree), ptr(g), -0.1, 0.1, ptr(v), None, st))
    r = {"case": name, "nodes": n, "T": T}
    for k, fn in (("report_us", full), ("summary_only_us", summary), ("arrays_only_us", arrays), ("tree_voltage_us", tv)):
        r[k], r[k + "_min"] = median_us(fn, calls)
    r["ratio_report_over_tree_voltage"] = r["report_us"] / r["tree_voltage_us"]
    return r


def node_sum_times(lib, calls, n=1_000_000, T=96, M=2048):
    import torch
    from revs_admm_amd._lib import check, ptr
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    node_of = np.sort(rng.integers(0, M, n))
    node_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(node_of, minlength=M))]).astype(np.int64)).to(dev)
    load = torch.rand(n, T, dtype=torch.float32, device=dev)
    p = torch.rand(n, T, dtype=torch.float32, device=dev)
    g = torch.zeros(M, T, dtype=torch.float64, device=dev)
    a32 = torch.zeros(M, T, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    r = {"case": "node sums", "residences": n, "T": T, "nodes": M}
    r["net_node_sums_us"], _ = median_us(lambda: check(lib.revs_net_node_sums(M, T, ptr(node_ptr), ptr(load), ptr(p), ptr(g), st)), calls)
    r["net_node_sums_one_profile_us"], _ = median_us(lambda: check(lib.revs_net_node_sums(M, T, ptr(node_ptr), None, ptr(p), ptr(g), st)), calls)
    r["aggregate_f32_us"], _ = median_us(lambda: check(lib.revs_aggregate_f32(M, T, ptr(node_ptr), ptr(p), ptr(a32), st)), calls)
    r["ratio_over_aggregate_f32"] = r["net_node_sums_us"] / r["aggregate_f32_us"]
    r["GB_per_s"] = 2 * 4 * n * T / r["net_node_sums_us"] * 1e-3
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--skip-node-sums", action="store_true")
    a = ap.parse_args()
    from revs_admm_amd import _lib, build
    build.build()
    lib = _lib.load()
    gf = golden_feeder()
    rows = [report_times(lib, "121144 feeder", gf, 1126, 24, a.calls),
            report_times(lib, "121144 feeder", gf, 1126, 96, a.calls),
            report_times(lib, "synthetic forest", forest(2048), 2048, 96, a.calls),
            report_times(lib, "synthetic forest", forest(16384), 16384, 96, a.calls)]
    if not a.skip_node_sums:
        rows.append(node_sum_times(lib, a.calls))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
