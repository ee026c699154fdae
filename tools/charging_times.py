#!/usr/bin/env python3
"""Times of the charging report:

    python tools/charging_times.py [--reps 20] [--out profiles/charging_times.json]

revs_charge_report on synthetic charger power on the device (half the residences own a 7.2 kW on/off charger that runs
T / 8 slots in two sessions inside an evening window), by HIP events around the call, warm, the median (min - max) of
--reps, at 100 000 x 24 and 1 000 000 x 96 with S = 1 and at the study shape 2 000 x 24 x S = 30:
  every output;  the rows pass alone (keep_out and hist only: one launch, 1 byte written a row);
  slot and day records alone (rows pass and fold, no per-row output).
Beside it revs_bill_rows on the same tensor -- it reads every row, the report the EV rows only, so its bytes are given
for both -- the copy of the power and the records to the host (host clock), which is what the report replaces, and
charging_report_device(rows=False): the call, the four revs_bill_study selections and the read-back of the records
(host clock).  Bytes of the rows pass: 4 T per EV row and 32 per record read; with every output 64 + 32 + 1 a row
written.  Reported as GB/s and as the share of 8 TB/s.  The counts of one case are checked against numpy first."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def events(torch, fn, reps):
    ts = []
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= 3:
            ts.append(a.elapsed_time(b))
    return stats(ts)


def host_clock(torch, fn, reps):
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= 1:
            ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts)


def make_case(torch, n, S, T, seed=0):
    """-> (p (n, S, T) float32 on the device, homes uint8 (n S 32,) on the device, the records on the host (n, S))."""
    from revs_admm_amd._lib import HOME_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, S), HOME_DTYPE)
    rec["ev"] = rng.random((n, S)) < 0.5
    rec["start"], rec["end"] = T * 11 // 24, T * 23 // 24
    k = max(T // 8, 2)
    rec["rating"], rec["capacity"], rec["initial"] = 7.2, 10.0 * k, 0.2           # (k slots at the rating: 0.2 -> 0.92)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    first = torch.randint(T * 11 // 24, T * 23 // 24 - k - 1, (n, S), device="cuda", generator=gen)
    t = torch.arange(T, device="cuda")[None, None, :]
    a = first[:, :, None]
    on = ((t >= a) & (t < a + k // 2)) | ((t >= a + k // 2 + 1) & (t < a + k + 1))
    ev = torch.from_numpy(rec["ev"] != 0).cuda()
    p = (7.2 * (on & ev[:, :, None])).float().contiguous()
    return p, torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(), rec


def case(torch, lib, n, S, T, reps):
    from revs_admm_amd import charging
    from revs_admm_amd._lib import CHARGE_DAY_DTYPE, CHARGE_SLOT_DTYPE, check, ptr
    p, homes, rec = make_case(torch, n, S, T)
    tariff = torch.linspace(0.05, 0.3, T, dtype=torch.float64, device="cuda")
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_row, d_slot, d_day = torch.empty(S * n * 64, **u8), torch.empty(S * T * 32, **u8), torch.empty(S * 64, **u8)
    d_hist = torch.empty(S, 3, T + 1, dtype=torch.int32, device="cuda")
    d_val, d_keep = torch.empty(4, S, n, dtype=torch.float64, device="cuda"), torch.empty(S, n, **u8)
    nbytes = int(lib.revs_charge_report_scratch(S, n, T))
    d_scratch = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(row=None, slot=None, day=None, hist=None, val=None, keep=None):
        check(lib.revs_charge_report(S, n, T, ptr(p), T, S * T, ptr(homes), ptr(tariff), 0.0, 1e-6, ptr(row), ptr(slot),
                                     ptr(day), ptr(hist), ptr(val), ptr(keep), ptr(d_scratch), st), "revs_charge_report")
    every = dict(row=d_row, slot=d_slot, day=d_day, hist=d_hist, val=d_val, keep=d_keep)
    call(**every)
    slot = d_slot.cpu().numpy().view(CHARGE_SLOT_DTYPE).reshape(S, T)
    day = d_day.cpu().numpy().view(CHARGE_DAY_DTYPE).reshape(S)
    on = (p[:, S - 1, :] > 0).sum(0).cpu().numpy()
    assert (slot["n_on"][S - 1] == on).all() and int(day["peak_on"][S - 1]) == on.max() and int(day["n_ev"][S - 1]) == int(rec["ev"][:, S - 1].sum())
    assert int(day["n_interrupted"][S - 1]) == int(day["n_ev"][S - 1]) and int(day["n_under"][S - 1]) == 0
    n_ev = int((rec["ev"] != 0).sum())
    read = 4 * T * n_ev + 32 * n * S
    row = {"residences": n, "S": S, "T": T, "reps": reps, "ev_rows": n_ev, "power_bytes": 4 * n * S * T,
           "scratch_bytes": nbytes, "rows_pass_bytes_read": read, "all_outputs_bytes_written": (64 + 32 + 1) * n * S,
           "peak_on": int(day["peak_on"][S - 1]), "coincidence": float(day["coincidence"][S - 1])}
    row["all_outputs_events"] = events(torch, lambda: call(**every), reps)
    row["rows_pass_alone_events"] = events(torch, lambda: call(hist=d_hist, keep=d_keep), reps)
    row["slot_and_day_events"] = events(torch, lambda: call(slot=d_slot, day=d_day), reps)
    ms = row["rows_pass_alone_events"]["median_ms"]
    row["rows_pass_GBps"] = (read + n * S) / ms * 1e-6
    row["rows_pass_share_of_8TBps"] = (read + n * S) / (ms * 1e-3) / PEAK_BYTES_PER_S
    ms = row["all_outputs_events"]["median_ms"]
    row["all_outputs_GBps"] = (read + (64 + 32 + 1) * n * S) / ms * 1e-6
    d_bill = torch.empty(S, n, dtype=torch.float64, device="cuda")
    row["bill_rows_events"] = events(torch, lambda: check(lib.revs_bill_rows(S, n, T, ptr(p), 0, T, S * T, ptr(tariff),
                                                                             ptr(d_bill), st), "revs_bill_rows"), reps)
    bms = row["bill_rows_events"]["median_ms"]
    row["bill_rows_GBps"] = (4 * n * S * T + 8 * n * S) / bms * 1e-6
    row["rows_pass_over_bill_rows"] = row["rows_pass_alone_events"]["median_ms"] / bms
    row["all_outputs_over_bill_rows"] = ms / bms
    row["copy_to_host_clock"] = host_clock(torch, lambda: (p.cpu(), homes.cpu()), max(3, reps // 4))
    row["copy_over_all_outputs"] = row["copy_to_host_clock"]["median_ms"] / ms
    row["report_device_rows_false_clock"] = host_clock(
        torch, lambda: charging.charging_report_device(p, homes, tariff, rows=False, lib=lib), max(3, reps // 4))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the residences (a quick look)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("charging_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    lib = _lib.load()
    k = 10 if a.small else 1
    rows = []
    for n, S, T in ((100_000 // k, 1, 24), (1_000_000 // k, 1, 96), (2_000, 30, 24)):
        rows.append(case(torch, lib, n, S, T, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
