#!/usr/bin/env python3
"""Times of the load-profile report:

    python tools/load_profile_times.py [--reps 20] [--out profiles/load_profile_times.json]

revs_load_profile on a synthetic schedule on the device (log-normal base load, half the residences with a 7.2 kW charger
in an evening window; classes: without / with EV), by HIP events around the call, warm, the median (min - max) of --reps:
  100 000 x 24 and 1 000 000 x 96 with S = 1, C = 2 -- slot, peak and day records;
  2 000 x 24 x S = 30, C = 2, three pools of ten -- every output.
Beside it the two routes it replaces: the copy of the profile to the host (profile.cpu(), host clock), and, where
S T <= 4096, revs_conv_report with K = 1 over the same buffer, its S T columns as scenarios -- one call gives the slot
records of ONE set (timed: the set "all", keep = NULL, and one class through a keep mask repeated T times); Q calls
give what the new call gives, without peaks, day figures or pools.
Bytes: every walk reads the profile once -- pass 0, three digit walks, neighbour, whisker and flier walk: 7 reads at the
most (a tile whose ranks are settled, or that has no flier, returns at once) -- the row kernel once more, and the
selection over the peaks 7 reads of n S floats; per pool sequence the same again.  Reported as an upper count and as
its share of 8 TB/s.  One cell of every case is checked against numpy before anything is timed."""
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


def make_profile(torch, n, S, T, seed=0):
    """-> (g (n, S, T) float32 on the device, cls (S, n) uint8 on the device)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g = torch.empty(n, S, T, dtype=torch.float32, device="cuda").log_normal_(-0.5, 0.6, generator=gen)
    ev = torch.rand(S, n, device="cuda", generator=gen) < 0.5
    start = torch.randint(T * 17 // 24, T * 20 // 24 + 1, (n, S), device="cuda", generator=gen)
    t = torch.arange(T, device="cuda")[None, None, :]
    on = (t >= start[:, :, None]) & (t < start[:, :, None] + max(T // 8, 1)) & ev.t()[:, :, None]
    g += 7.2 * on
    return g.contiguous(), ev.to(torch.uint8).contiguous()


def case(torch, lib, n, S, T, groups, reps):
    from revs_admm_amd._lib import BILL_DTYPE, PROFILE_DAY_DTYPE, check, ptr
    C, Q = 2, 3
    g, cls = make_profile(torch, n, S, T)
    G = 0 if groups is None else max(groups) + 1
    hg = None if groups is None else np.ascontiguousarray(groups, np.int32)
    u8 = dict(dtype=torch.uint8, device="cuda")
    rec = BILL_DTYPE.itemsize
    d_slot, d_peak = torch.empty(S * Q * T * rec, **u8), torch.empty(S * Q * rec, **u8)
    d_day = torch.empty(S * Q * PROFILE_DAY_DTYPE.itemsize, **u8)
    d_pslot = torch.empty(G * Q * T * rec, **u8) if G else None
    d_ppeak = torch.empty(G * Q * rec, **u8) if G else None
    nbytes = int(lib.revs_load_profile_scratch(S, n, T, C, G))
    d_scratch = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        check(lib.revs_load_profile(S, n, T, ptr(g), T, S * T, ptr(cls), C, None, hg.ctypes.data if G else None, G, 1.0,
                                    ptr(d_slot), ptr(d_peak), ptr(d_day), ptr(d_pslot), ptr(d_ppeak), ptr(d_scratch), st),
              "revs_load_profile")
    call()
    slot = d_slot.cpu().numpy().view(BILL_DTYPE).reshape(S, Q, T)
    day = d_day.cpu().numpy().view(PROFILE_DAY_DTYPE).reshape(S, Q)
    # one cell against numpy: the median and the count of the EV class at the aggregate's peak slot, last scenario
    s, t = S - 1, int(day[S - 1, 2]["peak_slot"])
    col = g[:, s, t].cpu().numpy().astype(np.float64)[cls[s].cpu().numpy() == 1]
    assert int(slot[s, 1, t]["count"]) == col.size and abs(slot[s, 1, t]["median"] - np.median(col)) <= 1e-15 * np.median(col)
    assert slot[s, 1, t]["max"] == col.max() and abs(slot[s, 1, t]["total"] - col.sum()) <= 1e-9 * col.sum()
    profile_bytes = 4 * n * S * T
    sequences = 2 if G else 1
    bytes_read = sequences * (7 * profile_bytes + 7 * 4 * n * S) + profile_bytes
    row = {"residences": n, "S": S, "T": T, "classes": C, "groups": G, "reps": reps, "profile_bytes": profile_bytes,
           "scratch_bytes": nbytes, "launch_bytes_read_upper": bytes_read,
           "day_all": {k: float(day[S - 1, 2][k]) for k in ("peak", "valley", "load_factor", "diversity")},
           "peak_slot": t}
    row["revs_load_profile_events"] = events(torch, call, reps)
    ms = row["revs_load_profile_events"]["median_ms"]
    row["bytes_read_upper_GBps"] = bytes_read / ms * 1e-6
    row["share_of_8TBps_upper"] = bytes_read / (ms * 1e-3) / PEAK_BYTES_PER_S
    row["profile_copy_to_host_clock"] = host_clock(torch, lambda: g.cpu(), max(3, reps // 4))
    if S * T <= 4096:
        cols = S * T
        d_iter = torch.empty(cols * rec, **u8)
        d_cs = torch.empty(int(lib.revs_conv_report_scratch(cols, n, 1, 0)) // 8 + 1, dtype=torch.float64, device="cuda")
        keep = (cls == 1).to(torch.uint8).repeat_interleave(T, dim=0).contiguous()          # (S T, n)

        def conv(k):
            check(lib.revs_conv_report(cols, n, 1, ptr(g), n * cols, ptr(k), None, None, 0, 1.0, 1, ptr(d_iter), None, None,
                                       None, None, ptr(d_cs), st), "revs_conv_report")
        conv(keep)
        it = d_iter.cpu().numpy().view(BILL_DTYPE).reshape(S, T)
        assert it["median"].tobytes() == slot[:, 1, :]["median"].tobytes() and it["count"].tobytes() == slot[:, 1, :]["count"].tobytes()
        row["conv_report_K1_one_set_all_events"] = events(torch, lambda: conv(None), reps)
        row["conv_report_K1_one_set_by_keep_events"] = events(torch, lambda: conv(keep), reps)
        row["conv_report_K1_keep_mask_bytes"] = int(keep.numel())
        row["conv_report_K1_three_sets_ms"] = (row["conv_report_K1_one_set_all_events"]["median_ms"]
                                               + 2 * row["conv_report_K1_one_set_by_keep_events"]["median_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the residences (a quick look)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("load_profile_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    lib = _lib.load()
    k = 10 if a.small else 1
    rows = []
    for n, S, T, groups in ((100_000 // k, 1, 24, None), (1_000_000 // k, 1, 96, None),
                            (2_000, 30, 24, [s // 10 for s in range(30)])):
        rows.append(case(torch, lib, n, S, T, groups, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
