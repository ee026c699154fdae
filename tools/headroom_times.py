#!/usr/bin/env python3
"""Times of the headroom report, HIP events, warm, median of --calls calls:

    python tools/headroom_times.py [--calls 30] [--out FILE.json]

  revs_net_headroom  every output (arrays, summary, day records), the arrays alone (one launch), the summary and the day
                     records alone -- on the 121144 feeder (T = 24, 96), on synthetic forests of 2048 and 16 384 positions
                     (T = 96) and at the study's shape (S = 30 scenarios, 2048 positions, T = 96) -- beside
                     revs_net_report / revs_net_study (arrays + summary) on the same tree, T and S: the yard-stick"""
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


def headroom_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import HEADROOM_DAY_DTYPE, check, ptr
    from revs_admm_amd.feeder import feeder_tree
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
    n = len(par)
    real = th["order"] < n
    d_nop = up(np.where(real, th["order"], -1).astype(np.int32))
    d_rating = up(np.where(real, rng.uniform(50.0, 500.0, th["n"]), 0.0))
    g = up(rng.uniform(0.0, 3.0, (S, M, T)))
    f64 = dict(dtype=torch.float64, device=dev)
    head, drop, flow = (torch.empty(S, n, T, **f64) for _ in range(3))
    lim = torch.empty(S, n, T, dtype=torch.int32, device=dev)
    summ = torch.zeros(S * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    day = torch.zeros(S * n * HEADROOM_DAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    scratch = torch.empty(lib.revs_net_headroom_scratch(S, T, th["n"]) // 8, **f64)
    out = [torch.empty(S, n, T, **f64) for _ in range(3)]
    summ2 = torch.zeros(S * 2 * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(h, l, d, f, s, dy):
        return lambda: check(lib.revs_net_headroom(S, M, T, C.byref(tree), C.byref(aux), ptr(g), ptr(d_rating), None, None,
                                                   ptr(d_nop), n, 0.0975, 4.8, ptr(h), ptr(l), ptr(d), ptr(f), ptr(s), ptr(dy),
                                                   ptr(scratch), st))
    study = lambda: check(lib.revs_net_study(S, M, T, C.byref(tree), ptr(g), ptr(d_rating), None, ptr(d_nop), n, 1.0, 0.95,
                                             1.05, None, 0, None, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(summ2), None,
                                             None, None, st))
    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S,
         "rounds": int(aux.n_jump) + 1}
    for k, fn in (("headroom_us", call(head, lim, drop, flow, summ, day)),
                  ("arrays_only_us", call(head, lim, drop, flow, None, None)),
                  ("headroom_and_limiter_only_us", call(head, lim, None, None, None, None)),
                  ("summary_and_day_only_us", call(None, None, None, None, summ, day)),
                  ("net_report_us", study)):
        r[k], r[k + "_min"] = median_us(fn, calls)
    r["ratio_headroom_over_net_report"] = r["headroom_us"] / r["net_report_us"]
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
    rows = [headroom_times(lib, "121144 feeder", gf, 1126, 24, 1, a.calls),
            headroom_times(lib, "121144 feeder", gf, 1126, 96, 1, a.calls),
            headroom_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            headroom_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls),
            headroom_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
