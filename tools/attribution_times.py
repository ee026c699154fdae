#!/usr/bin/env python3
"""Times of the attribution report, HIP events, warm, median of --calls calls:

    python tools/attribution_times.py [--calls 30] [--out profiles/attribution_times.json]

  revs_net_attribution  every output (arrays, slot records, summary, day records), the first launch alone (the arrays),
                        the summary and the day records alone -- on tools/headroom_times.py's cases: the 121144 feeder
                        (T = 24, 96), synthetic forests of 2048 and 16 384 positions (T = 96) and the study's shape (S = 30
                        scenarios, 2048 positions, T = 96) -- beside revs_net_headroom's every output and its arrays
                        launch on the same tree, T and S: the yard-stick"""
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


def attribution_times(lib, name, feeder, M, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import ATTR_DAY_DTYPE, ATTR_SLOT_DTYPE, HEADROOM_DAY_DTYPE, check, ptr
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
    d_cls = up((np.arange(th["n"]) % 3).astype(np.uint8))
    g_host = rng.uniform(0.0, 3.0, (S, M, T))
    g, ev = up(g_host), up(g_host * rng.uniform(0.0, 1.0, g_host.shape))
    f64 = dict(dtype=torch.float64, device=dev)
    sens, con, evc, drop, head, flow = (torch.empty(S, n, T, **f64) for _ in range(6))
    lim = torch.empty(S, n, T, dtype=torch.int32, device=dev)
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    slot, summ, day = u8(S * T * ATTR_SLOT_DTYPE.itemsize), u8(S * T * SUMMARY_DTYPE.itemsize), u8(S * n * ATTR_DAY_DTYPE.itemsize)
    hday = u8(S * n * HEADROOM_DAY_DTYPE.itemsize)
    scratch = torch.empty(lib.revs_net_attribution_scratch(S, T, th["n"]) // 8 + 1, **f64)
    hscratch = torch.empty(lib.revs_net_headroom_scratch(S, T, th["n"]) // 8, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(se, co, ec, dr, sl, su, dy):
        return lambda: check(lib.revs_net_attribution(S, M, T, C.byref(tree), C.byref(aux), ptr(g), ptr(ev), None, None,
                                                      ptr(d_cls), 3, ptr(d_nop), n, -1, 0.0975, 0.01, ptr(se), ptr(co), ptr(ec),
                                                      ptr(dr), ptr(sl), ptr(su), ptr(dy), ptr(scratch), st))

    def headroom(h, l, d, f, s, dy):
        return lambda: check(lib.revs_net_headroom(S, M, T, C.byref(tree), C.byref(aux), ptr(g), ptr(d_rating), None, None,
                                                   ptr(d_nop), n, 0.0975, 4.8, ptr(h), ptr(l), ptr(d), ptr(f), ptr(s), ptr(dy),
                                                   ptr(hscratch), st))
    r = {"case": name, "nodes": n, "positions": int(th["n"]), "T": T, "S": S}
    for k, fn in (("attribution_us", call(sens, con, evc, drop, slot, summ, day)),
                  ("first_launch_only_us", call(sens, con, evc, drop, None, None, None)),
                  ("summary_and_day_only_us", call(None, None, None, None, None, summ, day)),
                  ("headroom_us", headroom(head, lim, drop, flow, summ, hday)),
                  ("headroom_arrays_only_us", headroom(head, lim, drop, flow, None, None))):
        r[k], r[k + "_min"] = median_us(fn, calls)
    r["ratio_attribution_over_headroom"] = r["attribution_us"] / r["headroom_us"]
    r["ratio_first_launch_over_headroom_arrays"] = r["first_launch_only_us"] / r["headroom_arrays_only_us"]
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
    rows = [attribution_times(lib, "121144 feeder", gf, 1126, 24, 1, a.calls),
            attribution_times(lib, "121144 feeder", gf, 1126, 96, 1, a.calls),
            attribution_times(lib, "synthetic forest", forest(2048), 2048, 96, 1, a.calls),
            attribution_times(lib, "synthetic forest", forest(16384), 16384, 96, 1, a.calls),
            attribution_times(lib, "study shape", forest(2048), 2048, 96, 30, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
