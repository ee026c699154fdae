#!/usr/bin/env python3
"""Times of the flexibility report beside the charging report's on the same inputs:

    python tools/flex_times.py [--reps 20] [--out profiles/flex_times.json]

revs_flex_report and revs_charge_report on charging_times.py's synthetic charger power on the device (half the
residences own a 7.2 kW on/off charger that runs T / 8 slots in two sessions inside an evening window), in ONE process,
by HIP events around `inner` back-to-back calls, warm, the two reports alternating sample by sample, the median (min -
max) of --reps samples, at 100 000 x 24 and 1 000 000 x 96 with S = 1 and at the study shape 2 000 x 24 x S = 30:
  every output without the node arrays;  every output with them (ten consecutive rows a node);
  the rows pass alone (keep_out and hist only: one launch, 1 byte written a row) -- of both reports.
Bytes of the rows pass: 4 T per EV row and 32 per record read, 1 a row written; reported as GB/s and as the share of
8 TB/s -- the pass is bound by memory, so that is its share of peak.  The ratio flex / charging of the rows pass and of
every output is the figure DESIGN.md quotes: the charging report reads the same bytes through the same staging.  The
counts of every case are checked against numpy first."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12


def alternating(torch, fns, reps, inner):
    """{name: stats} of the calls `fns` ({name: callable}), one sample of each in turn, `inner` calls a sample."""
    from charging_times import stats
    ts = {k: [] for k in fns}
    for r in range(reps + 3):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if r >= 3:
                ts[k].append(a.elapsed_time(b) / inner)
    return {k: stats(v) for k, v in ts.items()}


def case(torch, lib, n, S, T, reps, inner):
    from charging_times import make_case
    from revs_admm_amd._lib import FLEX_DAY_DTYPE, FLEX_SLOT_DTYPE, check, ptr
    p, homes, rec = make_case(torch, n, S, T)
    tariff = torch.linspace(0.05, 0.3, T, dtype=torch.float64, device="cuda")
    u8 = dict(dtype=torch.uint8, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    m = (n + 9) // 10
    node_ptr = torch.from_numpy(np.minimum(np.arange(m + 1, dtype=np.int64) * 10, n)).cuda()
    d_row, d_slot, d_day = torch.empty(S * n * 64, **u8), torch.empty(S * T * 32, **u8), torch.empty(S * 64, **u8)
    d_hist = torch.empty(S, 3, T + 1, dtype=torch.int32, device="cuda")
    d_val, d_keep = torch.empty(4, S, n, **f64), torch.empty(S, n, **u8)
    d_nup, d_ndn = torch.empty(S, m, T, **f64), torch.empty(S, m, T, **f64)
    fbytes, cbytes = int(lib.revs_flex_report_scratch(S, n, T)), int(lib.revs_charge_report_scratch(S, n, T))
    d_scratch = torch.empty(max(fbytes, cbytes) // 8 + 1, **f64)
    st = torch.cuda.current_stream().cuda_stream

    def flex(row=None, slot=None, day=None, hist=None, nup=None, ndn=None, val=None, keep=None):
        check(lib.revs_flex_report(S, n, T, ptr(p), T, S * T, ptr(homes), 1, 0.0, 1e-6, ptr(node_ptr), m, ptr(row),
                                   ptr(slot), ptr(day), ptr(hist), ptr(nup), ptr(ndn), ptr(val), ptr(keep), ptr(d_scratch),
                                   st), "revs_flex_report")

    def charge(row=None, slot=None, day=None, hist=None, val=None, keep=None):
        check(lib.revs_charge_report(S, n, T, ptr(p), T, S * T, ptr(homes), ptr(tariff), 0.0, 1e-6, ptr(row), ptr(slot),
                                     ptr(day), ptr(hist), ptr(val), ptr(keep), ptr(d_scratch), st), "revs_charge_report")
    every = dict(row=d_row, slot=d_slot, day=d_day, hist=d_hist, val=d_val, keep=d_keep)
    flex(nup=d_nup, ndn=d_ndn, **every)
    slot = d_slot.cpu().numpy().view(FLEX_SLOT_DTYPE).reshape(S, T)
    day = d_day.cpu().numpy().view(FLEX_DAY_DTYPE).reshape(S)
    ev = rec["ev"][:, S - 1] != 0
    plugged = ev.sum() * ((np.arange(T) >= T * 11 // 24) & (np.arange(T) < T * 23 // 24))
    assert (slot["n_plugged"][S - 1] == plugged).all() and int(day["n_ev"][S - 1]) == int(ev.sum())
    # (on/off chargers at 7.2 kW: every reserve is a multiple of the rating, the node sums and the slot sums are exact)
    assert d_nup[S - 1].sum(0).cpu().numpy().tobytes() == slot["up"][S - 1].tobytes()
    assert d_ndn[S - 1].sum(0).cpu().numpy().tobytes() == slot["down"][S - 1].tobytes()
    assert (slot["down"][S - 1] / np.float64(np.float32(7.2)) == slot["n_down"][S - 1]).all() and slot["n_down"][S - 1].max() > 0
    n_ev = int((rec["ev"] != 0).sum())
    read = 4 * T * n_ev + 32 * n * S
    out = {"residences": n, "S": S, "T": T, "reps": reps, "calls_per_sample": inner, "ev_rows": n_ev, "nodes": m,
           "power_bytes": 4 * n * S * T, "flex_scratch_bytes": fbytes, "charge_scratch_bytes": cbytes,
           "rows_pass_bytes": read + n * S, "peak_up_kw": float(day["peak_up"][S - 1]),
           "peak_down_kw": float(day["peak_down"][S - 1])}
    out.update(alternating(torch, {
        "flex_all_outputs_events": lambda: flex(**every),
        "charge_all_outputs_events": lambda: charge(**every),
        "flex_with_nodes_events": lambda: flex(nup=d_nup, ndn=d_ndn, **every),
        "flex_rows_pass_alone_events": lambda: flex(hist=d_hist, keep=d_keep),
        "charge_rows_pass_alone_events": lambda: charge(hist=d_hist, keep=d_keep),
    }, reps, inner))
    med = lambda k: out[k]["median_ms"]
    for k in ("flex", "charge"):
        ms = med(k + "_rows_pass_alone_events")
        out[k + "_rows_pass_GBps"] = (read + n * S) / ms * 1e-6
        out[k + "_rows_pass_share_of_8TBps"] = (read + n * S) / (ms * 1e-3) / PEAK_BYTES_PER_S
    out["rows_pass_flex_over_charge"] = med("flex_rows_pass_alone_events") / med("charge_rows_pass_alone_events")
    out["all_outputs_flex_over_charge"] = med("flex_all_outputs_events") / med("charge_all_outputs_events")
    out["with_nodes_over_without"] = med("flex_with_nodes_events") / med("flex_all_outputs_events")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the residences (a quick look)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("flex_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    lib = _lib.load()
    k = 10 if a.small else 1
    rows = []
    for n, S, T, inner in ((100_000 // k, 1, 24, 20), (1_000_000 // k, 1, 96, 4), (2_000, 30, 24, 20)):
        rows.append(case(torch, lib, n, S, T, a.reps, inner))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
