#!/usr/bin/env python3
"""Times of revs_rule_schedule:

    python tools/rule_schedule_times.py [--reps 20] [--out profiles/rule_schedule_times.json]

Sizes 100 000 x 24 and 1 000 000 x 96 (rows x slots) of random records; output sets `g` alone (what rule_schedule() of an
engine and the bill report's rule baseline ask for) and all four (p, soc, g, status).  Warm, by HIP events around one
call, the median and the spread of --reps repeats.  Beside it revs_residence_solve (the individual mode's kernel, all its
outputs: p, soc, g) on the same records, the calls taking turns; and p, soc and status each alone: the launches all four
are made of.  Bytes: what a call must move at the least -- the load
read once, every wanted array written once, the 32-byte records once per launch that reads them (the rule call is one
launch per kind of output: p / g, soc, status) -- over the time, as a fraction of the HBM peak the project's rooflines
use (8.0 TB/s).  No threshold anywhere: a record of what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # bytes/s
SIZES = ((100_000, 24), (1_000_000, 96))


def records(rng, n, T):
    from revs_admm_amd.engine import pack_homes
    start = rng.integers(0, T // 2 + 1, n)
    end = np.minimum(start + rng.integers(T // 4, T, n), T)
    return pack_homes(rng.random(n) < 0.75, rng.choice([3.6, 4.8, 7.2], n) * 24.0 / T, rng.choice([20.0, 40.0, 60.0], n),
                      rng.uniform(0.1, 0.85, n), start, end)


def spread(ms):
    v = np.asarray(ms)
    return dict(median_us=float(np.median(v) * 1e3), min_us=float(v.min() * 1e3), max_us=float(v.max() * 1e3),
                iqr_us=[float(np.percentile(v, 25) * 1e3), float(np.percentile(v, 75) * 1e3)])


def time_size(lib, n, T, reps):
    import torch
    from revs_admm_amd._lib import HOME_DTYPE, check, ptr
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n + T)
    rec = records(rng, n, T)
    homes = torch.from_numpy(rec.view(np.uint8).reshape(n, HOME_DTYPE.itemsize)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    load = torch.rand(n, T, generator=gen, device=dev) * 3.0
    tariff = torch.linspace(0.05, 0.3, T, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    p, g, soc = torch.empty(n, T, **f32), torch.empty(n, T, **f32), torch.empty(n, T + 1, **f32)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    rule = lambda want: check(lib.revs_rule_schedule(n, T, ptr(homes), ptr(load), 0, 0, 1, ptr(p) if "p" in want else None,
                                                     ptr(soc) if "s" in want else None, ptr(g) if "g" in want else None,
                                                     ptr(status) if "x" in want else None, st), "revs_rule_schedule")
    calls = {
        "rule_g": lambda: rule("g"),
        "rule_all": lambda: rule("psgx"),
        "rule_p": lambda: rule("p"),              # (the launches of rule_all one by one: where its time goes)
        "rule_soc": lambda: rule("s"),
        "rule_status": lambda: rule("x"),
        "residence_solve": lambda: check(lib.revs_residence_solve(n, T, ptr(tariff), ptr(homes), ptr(load), ptr(p), ptr(soc),
                                                                 ptr(g), st), "revs_residence_solve"),
    }
    nT, rec_b = 4 * n * T, 32 * n
    nbytes = {"rule_g": 2 * nT + rec_b,
              "rule_all": 3 * nT + 4 * n * (T + 1) + 4 * n + 3 * rec_b,
              "rule_p": nT + rec_b, "rule_soc": 4 * n * (T + 1) + rec_b, "rule_status": 4 * n + rec_b,
              "residence_solve": 3 * nT + 4 * n * (T + 1) + rec_b + 4 * T}
    ts = {k: [] for k in calls}
    for r in range(reps + 3):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 3:
                ts[k].append(a.elapsed_time(b))
    row = {"rows": n, "T": T, "reps": reps, "policy": "uncontrolled", "fill": "target", "charger": "binary"}
    for k in calls:
        s = spread(ts[k])
        s["bytes"] = nbytes[k]
        s["TBps"] = nbytes[k] / (s["median_us"] * 1e-6) / 1e12
        s["share_of_hbm_peak"] = nbytes[k] / (s["median_us"] * 1e-6) / HBM_PEAK
        row[k] = s
    row["rule_all_over_residence_solve"] = row["rule_all"]["median_us"] / row["residence_solve"]["median_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rule_schedule_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import _lib
    lib = _lib.load()
    rows = []
    for n, T in SIZES:
        rows.append(time_size(lib, n, T, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
