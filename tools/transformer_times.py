#!/usr/bin/env python3
"""Times of the transformer report, by tools/loss_times.py's method -- HIP events, warm, median
of --calls calls:

    python tools/transformer_times.py [--calls 30] [--out profiles/transformer_times.json]

  revs_xf_report   every output (five arrays, two summaries, day and fleet records: three launches), the arrays alone (one
                   launch), the records alone -- on the 121144 feeder's 462 transformers (owners from the labels, ratings
                   from the base load; T = 24 and 96), on 65 535 transformers of 1 row each (T = 96) and at the study's
                   shape (S = 30 scenarios, 1000 transformers of 7 rows, T = 96), substeps = 1, cyclic start -- beside two
                   yard-sticks: revs_net_losses with its four arrays alone on a feeder of the same number of rows, and the
                   device-to-host copy of the node sums (pageable host memory, torch's .cpu()) that the report makes
                   unnecessary."""
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


def golden_fleet():
    from oracle import revs_oracle as ro
    from test_network_host import golden_graph
    from revs_admm_amd.transformers import rows_by_transformer, size_ratings
    golden = ro.load_golden(os.path.join(ROOT, "tests", "golden", "revs_121144.npz"))
    xf_of = rows_by_transformer(golden_graph(golden))[1]
    load = np.asarray(golden[0]["LOAD"], np.float64)
    base = np.zeros((int(xf_of.max()) + 1, load.shape[1]))
    np.add.at(base, xf_of, load)
    return xf_of, size_ratings(base.max(axis=1)) * 0.95, base.max(axis=1)


def xf_times(lib, name, xf_of, rated_kw, peak_kw, feeder, T, S, calls):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import XF_DAY_DTYPE, XF_FLEET_DTYPE, check, ptr
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.transformers import ThermalModel, build_csr
    M, K = len(xf_of), len(rated_kw)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    xf_ptr, xf_rows = build_csr(xf_of, M, K)
    # loads around each transformer's sizing peak, up to twice it: ratios 0 - 2
    per_row = (peak_kw / np.maximum(np.bincount(xf_of[xf_of >= 0], minlength=K), 1))[np.maximum(xf_of, 0)]
    g = up(rng.uniform(0.0, 2.0, (S, M, T)) * per_row[None, :, None])
    d_ptr, d_rows, d_rated, d_amb = up(xf_ptr), up(xf_rows), up(rated_kw), up(np.full(T, 30.0))
    mdl = ThermalModel()
    ms, hours = mdl.struct(), 24.0 / T
    d_to, d_w = mdl.decays(hours, 1)
    f64 = dict(dtype=torch.float64, device=dev)
    arrays = [torch.empty(S, K, T, **f64) for _ in range(5)]
    rec = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    records = [rec(S * T * SUMMARY_DTYPE.itemsize), rec(S * T * SUMMARY_DTYPE.itemsize), rec(S * K * XF_DAY_DTYPE.itemsize),
               rec(S * XF_FLEET_DTYPE.itemsize)]
    scratch = torch.empty(lib.revs_xf_report_scratch(S, T, K) // 8, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(outs):
        return lambda: check(lib.revs_xf_report(S, M, T, K, len(xf_rows), ptr(g), ptr(d_ptr), ptr(d_rows), ptr(d_rated),
                                                ptr(d_amb), C.byref(ms), hours, 1, d_to, d_w, 1, 0.0, 0.0, 1.0, 110.0,
                                                *[ptr(o) for o in outs], ptr(scratch), st))
    # the yard-sticks: the loss report's arrays on a feeder of M rows, and the node sums' way to the host
    par, er, cons = feeder
    th = feeder_tree(par, er, cons, np.ones(M, bool))
    d_pack, d_w_ = up(th["pack"].view(np.int64)), up(th["w"])
    tree = _lib.Tree(th["n"], ptr(d_pack), ptr(d_w_))
    n = len(par)
    d_nop = up(np.where(th["order"] < n, th["order"], -1).astype(np.int32))
    g_small = g * 1e-9                                # (no bad slot on the synthetic forests' resistances)
    lo = [torch.empty(S, n, T, **f64) for _ in range(4)]
    losses = lambda: check(lib.revs_net_losses(S, M, T, C.byref(tree), ptr(g_small), None, None, None, 0, ptr(d_nop), n, 1.0,
                                               hours, 1e-3, None, ptr(lo[0]), ptr(lo[1]), ptr(lo[2]), ptr(lo[3]), None, None,
                                               None, None, None, st))
    r = {"case": name, "rows": M, "transformers": K, "T": T, "S": S, "loss_report_nodes": n}
    for k, fn in (("report_us", call(arrays + records)), ("arrays_only_us", call(arrays + [None] * 4)),
                  ("records_only_us", call([None] * 5 + records)), ("loss_arrays_us", losses),
                  ("node_sums_to_host_us", lambda: g.cpu())):
        r[k], r[k + "_min"] = median_us(fn, calls)
    torch.cuda.synchronize()
    fleet = records[3].cpu().numpy().view(XF_FLEET_DTYPE)
    r["bad_transformers"], r["overloaded"] = int(fleet["n_nan"].sum()), int(fleet["n_overloaded"].sum())
    r["node_sums_bytes"] = int(g.numel() * 8)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    from revs_admm_amd import _lib, build
    build.build()
    lib = _lib.load()
    xf_of, rated, peak = golden_fleet()
    gf = golden_feeder()
    big = np.arange(65535)
    study = np.concatenate([np.repeat(np.arange(1000), 7), np.full(48, -1)])        # 7048 rows
    rows = [xf_times(lib, "121144 feeder", xf_of, rated, peak, gf, 24, 1, a.calls),
            xf_times(lib, "121144 feeder", xf_of, rated, peak, gf, 96, 1, a.calls),
            xf_times(lib, "65535 transformers of one row", big, np.full(65535, 9.5), np.full(65535, 9.5), forest_rows(65535), 96, 1,
                     a.calls),
            xf_times(lib, "study shape", study, np.full(1000, 23.75), np.full(1000, 23.75), forest_rows(len(study)), 96, 30,
                     a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


def forest_rows(M):
    """A feeder whose M rows sit on the first M nodes of a forest that the tree form holds (at most 16 384 positions):
    the loss report's yard-stick scans min(M, 16384) nodes -- its largest shape -- whatever M is."""
    n = min(M, 16384)
    par, er, _ = forest(n)
    cons = np.full(n, -1, np.int64)
    cons[:] = np.arange(n)
    return par, er, cons


if __name__ == "__main__":
    main()
