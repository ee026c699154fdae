#!/usr/bin/env python3
"""Times of the risk report, HIP events, warm, median of --calls calls:

    python tools/risk_times.py [--calls 30] [--out profiles/risk_times.json]

  revs_net_risk  with K = 0 and K = 2 shared factors (node_var given in both): every output (arrays, slot records, summary,
                 day records), the first launch alone (the five arrays and the slot records), the summary and the day
                 records alone -- on tools/attribution_times.py's cases: the 121144 feeder (T = 24, 96), synthetic forests
                 of 2048 and 16 384 positions (T = 96) and the study's shape (S = 30 scenarios, 2048 positions, T = 96) --
                 beside revs_net_headroom's every output and its arrays launch on the same tree, T and S: the yard-stick.
                 The first launch runs 2 + K pairs of scans where headroom's arrays launch runs one (two in its 1024 x 16
                 shape): ratio_first_launch_over_headroom_arrays is to be read against 2 + K."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from network_times import forest, golden_feeder, median_us  # noqa: E402


def risk_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import HEADROOM_DAY_DTYPE, RISK_DAY_DTYPE, RISK_SLOT_DTYPE, check, ptr
    from revs_admm_amd.feeder import feeder_tree, risk_weights
    from revs_admm_amd.headroom import aux_on_device
    from revs_admm_amd.network import SUMMARY_DTYPE
    par, er, cons = feeder
    th = feeder_tree(par, er, cons, np.ones(M, bool))
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    d_pack, d_w = up(th["pack"].view(np.int64)), up(th["w"])
    tree = _lib.Tree(th["n"], ptr(d_pack), ptr(d_w))
    aux, _keep = aux_on_device(dev, th)
    d_w2 = up(risk_weights(th))
    n = len(par)
    real = th["order"] < n
    d_nop = up(np.where(real, th["order"], -1).astype(np.int32))
    d_rating = up(np.where(real, rng.uniform(50.0, 500.0, th["n"]), 0.0))
    g_host = rng.uniform(0.0, 3.0, (S, M, T))
    g, var = up(g_host), up((0.1 * g_host) ** 2)
    com = up(np.stack([0.05 * g_host, g_host * rng.uniform(0.0, 0.04, g_host.shape)]))
    f64 = dict(dtype=torch.float64, device=dev)
    sd, z, prob, dq, drop, head, flow = (torch.empty(S, n, T, **f64) for _ in range(7))
    lim = torch.empty(S, n, T, dtype=torch.int32, device=dev)
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    slot, summ, day = u8(S * T * RISK_SLOT_DTYPE.itemsize), u8(S * T * SUMMARY_DTYPE.itemsize), u8(S * n * RISK_DAY_DTYPE.itemsize)
    hday = u8(S * n * HEADROOM_DAY_DTYPE.itemsize)
    scratch = torch.empty(lib.revs_net_risk_scratch(S, T, th["n"]) // 8 + 1, **f64)
    hscratch = torch.empty(lib.revs_net_headroom_scratch(S, T, th["n"]) // 8, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(K, arrays, sl, su, dy):
        a = [ptr(x) for x in (sd, z, prob, dq, drop)] if arrays else [None] * 5
        return lambda: check(lib.revs_net_risk(S, M, T, C.byref(tree), C.byref(aux), ptr(g), ptr(var), ptr(com) if K else None, K,
                                               ptr(d_w2), None, None, ptr(d_nop), n, 0.0975, 1.6448536269514722, *a, ptr(sl),
                                               ptr(su), ptr(dy), ptr(scratch), st))

    def headroom(h, l, d, f, s, dy):
        return lambda: check(lib.revs_net_headroom(S, M, T, C.byref(tree), C.byref(aux), ptr(g), ptr(d_rating), None, None,
                                                   ptr(d_nop), n, 0.0975, 4.8, ptr(h), ptr(l), ptr(d), ptr(f), ptr(s), ptr(dy),
                                                   ptr(hscratch), st))
    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S}
    runs = [("headroom_us", headroom(head, lim, drop, flow, summ, hday)),
            ("headroom_arrays_only_us", headroom(head, lim, drop, flow, None, None))]
    for K in (0, 2):
        runs += [(f"risk_k{K}_us", call(K, True, slot, summ, day)),
                 (f"first_launch_only_k{K}_us", call(K, True, slot, None, None)),
                 (f"summary_and_day_only_k{K}_us", call(K, False, None, summ, day))]
    for k, fn in runs:
        r[k], r[k + "_min"] = median_us(fn, calls)
    for K in (0, 2):
        r[f"ratio_risk_k{K}_over_headroom"] = r[f"risk_k{K}_us"] / r["headroom_us"]
        r[f"ratio_first_launch_k{K}_over_headroom_arrays"] = r[f"first_launch_only_k{K}_us"] / r["headroom_arrays_only_us"]
        r[f"scan_pairs_k{K}"] = 2 + K
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
    rows = [risk_times(lib, "121144 feeder", gf, 1126, 24, 1, a.calls),
            risk_times(lib, "121144 feeder", gf, 1126, 96, 1, a.calls),
            risk_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            risk_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls),
            risk_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
