#!/usr/bin/env python3
"""Times of the price report, HIP events, warm, median of --calls calls:

    python tools/price_times.py [--calls 30] [--out profiles/price_times.json]

  revs_net_prices  with the loss term: every output (seven arrays, slot records, summary, node, line and day records),
                   the first launch alone (the seven arrays and the slot records), and the first launch without the loss
                   term -- on the 121144 feeder (T = 24, 96), a synthetic forest of 2048 positions (T = 96, S = 1 and the
                   study's S = 30) and, for the 1024 x 16 shape, one of 16 384 positions -- beside revs_net_losses' every
                   output and its first launch with its four arrays on the same inputs: the yard-stick (losses_kernels.hip
                   is the parent commit's).  The first launch runs five scans (four without the loss term) and gathers
                   twice where the loss report's runs three and gathers once."""
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


def price_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import (LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE, PRICE_DAY_DTYPE,
                                    PRICE_NODE_DAY_DTYPE, PRICE_SLOT_DTYPE, check, ptr)
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    from revs_admm_amd.network import SUMMARY_DTYPE
    par, er, cons = feeder
    th = feeder_tree(par, er, cons, np.ones(M, bool))
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    d_pack, d_w = up(th["pack"].view(np.int64)), up(th["w"])
    tree = _lib.Tree(th["n"], ptr(d_pack), ptr(d_w))
    n = len(par)
    d_nop = up(np.where(th["order"] < n, th["order"], -1).astype(np.int32))
    g_host = rng.uniform(0.0, 3.0, (S, M, T))
    g_host *= 0.15 / np.abs(tree_report_host(th, g_host[0], n)[1]).max()         # (no bad slot: the deepest drop is 0.15)
    y_host = np.where(rng.random((S, M, T)) < 0.05, rng.normal(0.0, 0.5, (S, M, T)), 0.0)
    g, y, cost = up(g_host), up(y_host), up(rng.uniform(0.05, 0.3, T))
    f64 = dict(dtype=torch.float64, device=dev)
    arr = [torch.empty(S, n, T, **f64) for _ in range(7)]
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    summ, slot, nday = u8(S * T * SUMMARY_DTYPE.itemsize), u8(S * T * PRICE_SLOT_DTYPE.itemsize), u8(S * n * PRICE_NODE_DAY_DTYPE.itemsize)
    lday, day = u8(S * n * LOSS_LINE_DAY_DTYPE.itemsize), u8(S * PRICE_DAY_DTYPE.itemsize)
    lslot, ldayrec = u8(S * T * LOSS_SLOT_DTYPE.itemsize), u8(S * LOSS_DAY_DTYPE.itemsize)
    scratch = torch.empty(lib.revs_net_prices_scratch(S, T, th["n"]) // 8 + 1, **f64)
    lscratch = torch.empty(lib.revs_net_losses_scratch(S, T, th["n"]) // 8 + 1, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream

    def prices(with_loss, staged):
        rec = [ptr(summ), ptr(slot), ptr(nday), ptr(lday), ptr(day)] if staged else [None, ptr(slot), None, None, None]
        return lambda: check(lib.revs_net_prices(S, M, T, C.byref(tree), ptr(g), ptr(y), None, ptr(cost), None, None, ptr(d_nop),
                                                 n, 1.0, with_loss, 24.0 / T, 0.2, *[ptr(a) for a in arr], *rec,
                                                 ptr(scratch) if staged else None, st))

    def losses(staged):
        rec = [ptr(summ), ptr(lslot), ptr(lday), ptr(ldayrec)] if staged else [None, ptr(lslot), None, None]
        return lambda: check(lib.revs_net_losses(S, M, T, C.byref(tree), ptr(g), None, None, None, 0, ptr(d_nop), n, 1.0,
                                                 24.0 / T, 0.01, ptr(cost), *[ptr(a) for a in arr[:4]], *rec,
                                                 ptr(lscratch) if staged else None, st))

    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S}
    for k, fn in (("losses_us", losses(True)), ("losses_first_launch_us", losses(False)), ("prices_us", prices(1, True)),
                  ("prices_first_launch_us", prices(1, False)), ("prices_first_launch_no_loss_us", prices(0, False))):
        r[k], r[k + "_min"] = median_us(fn, calls)
    r["ratio_prices_over_losses"] = r["prices_us"] / r["losses_us"]
    r["ratio_first_launch_over_losses_first_launch"] = r["prices_first_launch_us"] / r["losses_first_launch_us"]
    r["ratio_first_launch_no_loss_over_losses_first_launch"] = r["prices_first_launch_no_loss_us"] / r["losses_first_launch_us"]
    r["scans"] = {"prices": 5, "prices_no_loss": 4, "losses": 3}
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
    rows = [price_times(lib, "121144 feeder", gf, 1126, 24, 1, a.calls),
            price_times(lib, "121144 feeder", gf, 1126, 96, 1, a.calls),
            price_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            price_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls),
            price_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
