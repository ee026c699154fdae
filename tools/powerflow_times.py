#!/usr/bin/env python3
"""Times of the power-flow report, HIP events, warm, median of --calls calls:

    python tools/powerflow_times.py [--calls 30] [--out profiles/powerflow_times.json]

  revs_net_powerflow  every output (four or five arrays, slot records, summary, node and day records) and the first launch
                      alone (the arrays and the slot records), with and without xw (xw = 0.5 w, a power factor of 0.95) --
                      on a synthetic forest of 2048 and of 16 384 positions (T = 96, S = 1) and on the study's shape
                      (S = 30, 2048 positions, T = 96) -- beside revs_net_losses' every output and its first launch with its
                      four arrays on the same inputs: the yard-stick.  The loss report's first launch runs 3 scans; the
                      power-flow launch runs 2 passes + 1 scans, 3 passes + 1 with xw (passes: pass 0 and the `iters`
                      behind it, the largest over the slots, written beside the times)."""
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

from network_times import forest, median_us  # noqa: E402


def powerflow_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import (LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE, PF_DAY_DTYPE, PF_NODE_DAY_DTYPE,
                                    PF_SLOT_DTYPE, check, ptr)
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    from revs_admm_amd.network import SUMMARY_DTYPE
    par, er, cons = feeder
    th = feeder_tree(par, er, cons, np.ones(M, bool))
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    d_pack, d_w = up(th["pack"].view(np.int64)), up(th["w"])
    d_xw = up(0.5 * th["w"])
    tree = _lib.Tree(th["n"], ptr(d_pack), ptr(d_w))
    n = len(par)
    d_nop = up(np.where(th["order"] < n, th["order"], -1).astype(np.int32))
    g_host = rng.uniform(0.0, 3.0, (S, M, T))
    g_host *= 0.15 / np.abs(tree_report_host(th, g_host[0], n)[1]).max()         # (no bad slot: the deepest drop is 0.15)
    g, cost = up(g_host), up(rng.uniform(0.05, 0.3, T))
    f64 = dict(dtype=torch.float64, device=dev)
    arr = [torch.empty(S, n, T, **f64) for _ in range(5)]
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    summ, slot, nday = u8(S * T * SUMMARY_DTYPE.itemsize), u8(S * T * PF_SLOT_DTYPE.itemsize), u8(S * n * PF_NODE_DAY_DTYPE.itemsize)
    day = u8(S * PF_DAY_DTYPE.itemsize)
    lslot, lday, ldayrec = u8(S * T * LOSS_SLOT_DTYPE.itemsize), u8(S * n * LOSS_LINE_DAY_DTYPE.itemsize), u8(S * LOSS_DAY_DTYPE.itemsize)
    scratch = torch.empty(lib.revs_net_powerflow_scratch(S, T, th["n"]) // 8 + 1, **f64)
    lscratch = torch.empty(lib.revs_net_losses_scratch(S, T, th["n"]) // 8 + 1, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream
    tan_phi = float(np.tan(np.arccos(0.95)))

    def powerflow(with_x, staged):
        rec = [ptr(summ), ptr(slot), ptr(nday), ptr(day)] if staged else [None, ptr(slot), None, None]
        outs = [ptr(a) for a in arr[:4]] + [ptr(arr[4]) if with_x else None]
        return lambda: check(lib.revs_net_powerflow(S, M, T, C.byref(tree), ptr(g), ptr(d_xw) if with_x else None,
                                                    tan_phi if with_x else 0.0, None, ptr(d_nop), n, 1.0, 0.95, 1e-12, 32,
                                                    24.0 / T, ptr(cost), *outs, *rec, ptr(scratch), st))

    def losses(staged):
        rec = [ptr(summ), ptr(lslot), ptr(lday), ptr(ldayrec)] if staged else [None, ptr(lslot), None, None]
        return lambda: check(lib.revs_net_losses(S, M, T, C.byref(tree), ptr(g), None, None, None, 0, ptr(d_nop), n, 1.0,
                                                 24.0 / T, 0.01, ptr(cost), *[ptr(a) for a in arr[:4]], *rec,
                                                 ptr(lscratch) if staged else None, st))

    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S}
    for k, fn in (("losses_us", losses(True)), ("losses_first_launch_us", losses(False))):
        r[k], r[k + "_min"] = median_us(fn, calls)
    for tag, with_x in (("", False), ("_x", True)):
        for k, fn in (("powerflow%s_us" % tag, powerflow(with_x, True)),
                      ("powerflow%s_first_launch_us" % tag, powerflow(with_x, False))):
            r[k], r[k + "_min"] = median_us(fn, calls)
        torch.cuda.synchronize()
        rec = slot.cpu().numpy().view(PF_SLOT_DTYPE)
        assert (rec["status"] == 0).all()
        passes = 1 + int(rec["iters"].max())
        scans = (3 if with_x else 2) * passes + 1
        r["passes" + tag] = passes
        r["passes_mean" + tag] = 1.0 + float(rec["iters"].mean())
        r["scans" + tag] = scans
        ratio = r["powerflow%s_first_launch_us" % tag] / r["losses_first_launch_us"]
        r["ratio_first_launch%s_over_losses_first_launch" % tag] = ratio
        r["scan_count_ratio" + tag] = scans / 3.0
        r["ratio%s_over_scan_count_ratio" % tag] = ratio / (scans / 3.0)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    from revs_admm_amd import _lib, build
    build.build()
    lib = _lib.load()
    rows = [powerflow_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            powerflow_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls),
            powerflow_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
