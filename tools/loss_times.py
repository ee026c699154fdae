#!/usr/bin/env python3
"""Times of the loss report, by tools/headroom_times.py's method -- HIP events, warm, median of
--calls calls -- on that tool's five cases:

    python tools/loss_times.py [--calls 30] [--out FILE.json]

  revs_net_losses  every output (four arrays, summary, slot, line-day and day records: four launches), the arrays alone
                   (one launch), the loss array alone, the records alone -- on the 121144 feeder (T = 24, 96), on
                   synthetic forests of 2048 and 16 384 positions (T = 96) and at the study's shape (S = 30 scenarios,
                   2048 positions, T = 96) -- beside revs_net_study (arrays + summary) on the same tree, T and S: the
                   yard-stick.  The loads are small enough that no slot is bad (bad_slots is read back and stored)."""
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


def loss_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE, check, ptr
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
    d_cls = up(np.where(real, rng.integers(0, 3, th["n"]), 255).astype(np.uint8))
    d_cost = up(rng.uniform(0.05, 0.3, T))
    g = up(rng.uniform(0.0, 3.0, (S, M, T)) * 1e-7)
    f64 = dict(dtype=torch.float64, device=dev)
    loss, mlf, drop, flow = (torch.empty(S, n, T, **f64) for _ in range(4))
    rec = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    summ, slot = rec(S * T * SUMMARY_DTYPE.itemsize), rec(S * T * LOSS_SLOT_DTYPE.itemsize)
    lday, day = rec(S * n * LOSS_LINE_DAY_DTYPE.itemsize), rec(S * LOSS_DAY_DTYPE.itemsize)
    scratch = torch.empty(lib.revs_net_losses_scratch(S, T, th["n"]) // 8, **f64)
    out = [torch.empty(S, n, T, **f64) for _ in range(3)]
    summ2 = torch.zeros(S * 2 * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(ls, ml, d, f, s, sl, ld, dy):
        return lambda: check(lib.revs_net_losses(S, M, T, C.byref(tree), ptr(g), None, None, ptr(d_cls), 3, ptr(d_nop), n, 1.0,
                                                 24.0 / T, 1e-3, ptr(d_cost), ptr(ls), ptr(ml), ptr(d), ptr(f), ptr(s), ptr(sl),
                                                 ptr(ld), ptr(dy), ptr(scratch), st))
    study = lambda: check(lib.revs_net_study(S, M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0, 0.95,
                                             1.05, None, 0, None, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(summ2), None,
                                             None, None, st))
    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S}
    for k, fn in (("losses_us", call(loss, mlf, drop, flow, summ, slot, lday, day)),
                  ("arrays_only_us", call(loss, mlf, drop, flow, None, None, None, None)),
                  ("loss_array_only_us", call(loss, None, None, None, None, None, None, None)),
                  ("records_only_us", call(None, None, None, None, summ, slot, lday, day)),
                  ("net_report_us", study)):
        r[k], r[k + "_min"] = median_us(fn, calls)
    torch.cuda.synchronize()
    r["bad_slots"] = int(day.cpu().numpy().view(LOSS_DAY_DTYPE)["n_bad_slots"].sum())
    r["ratio_losses_over_net_report"] = r["losses_us"] / r["net_report_us"]
    r["ratio_arrays_over_net_report"] = r["arrays_only_us"] / r["net_report_us"]
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
    rows = [loss_times(lib, "121144 feeder", gf, 1126, 24, 1, a.calls),
            loss_times(lib, "121144 feeder", gf, 1126, 96, 1, a.calls),
            loss_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            loss_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls),
            loss_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
