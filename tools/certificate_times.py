#!/usr/bin/env python3
"""Times of certifying S scenarios of one feeder, one engine per scenario against the ensemble:

    python tools/certificate_times.py [--reps 15] [--sizes 1,10,36] [--out FILE.json]

  (a) single    S AdmmEngine.certificate(multipliers=y_s, search=True) calls, one after the other, on S engines that
                hold the scenarios' states -- about 30 bound evaluations each, every one a launch and a read-back
  (b) ensemble  one AdmmEnsemble.certificates(multipliers=y, search=True) -- the S searches in lock-step, one launch
                and one read-back per round

on the 121144 feeder: community 2, 90 % adoption, 4.8 kW, on/off chargers, T = 24 (scenario s: the EV homes of seed
1234 + s), after the same 15-iteration ensemble run; both sides get that run's multipliers and schedules.  Only the
calls are timed -- (a)'s S engine constructions and state uploads, which (b) does not need, are reported beside them
(once, not in the rounds).  Warm (one untimed round of both sides), then the median and quartiles of --reps rounds by the
host clock (each call ends in a read-back), the two sides taking turns inside every round.  The launch counts
(`evaluations`) are deterministic and reported as they are."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ITERS = 15


def time_case(S, reps):
    import torch
    from ensemble_times import feeder_case
    from revs_admm_amd.engine import AdmmEngine, pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    cost, load, Rr, feeder, draw, (start, end) = feeder_case(24, False)
    n = load.shape[0]
    recs = [pack_homes(draw(1234 + s), 4.8, 20.0, 0.2, start, end) for s in range(S)]
    kw = dict(kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="binary", feeder=feeder)
    ens = AdmmEnsemble(cost, recs, load, np.arange(n), Rr, **kw)
    ens.run(ITERS)
    y = np.stack([ens.multipliers(s) for s in range(S)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engines = []
    for s in range(S):
        e = AdmmEngine(cost, recs[s], load, np.arange(n), Rr, **kw)
        e.set_state(*ens.get_state(s))
        engines.append(e)
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)

    def single():
        t0 = time.perf_counter()
        out = [e.certificate(multipliers=y[s], search=True) for s, e in enumerate(engines)]
        return 1e3 * (time.perf_counter() - t0), out

    def ensemble():
        t0 = time.perf_counter()
        out = ens.certificates(multipliers=y, search=True)
        return 1e3 * (time.perf_counter() - t0), out

    sides = [("single", single), ("ensemble", ensemble)]
    warm = {k: fn()[1] for k, fn in sides}
    ts = {k: [] for k, _ in sides}
    for _ in range(reps):
        for k, fn in sides:
            ts[k].append(fn()[0])
    a, b = warm["single"], warm["ensemble"]
    row = {"case": "golden24", "S": S, "residences": n, "iterations": ITERS, "reps": reps,
           "scenarios_with_multipliers": int(sum(bool(np.any(y[s])) for s in range(S))),
           "single_evaluations": [c.evaluations for c in a], "single_evaluations_total": int(sum(c.evaluations for c in a)),
           "ensemble_evaluations": int(b[0].evaluations),
           "max_rel_lower_ensemble_minus_single": float(max(abs(p.lower - q.lower) / abs(q.lower) for p, q in zip(b, a))),
           "max_rel_upper_ensemble_minus_single": float(max(abs(p.upper - q.upper) / abs(q.upper) for p, q in zip(b, a))),
           "single_engines_build_and_state_ms_once": build_ms}
    for k, _ in sides:
        v = np.array(ts[k])
        row[f"{k}_ms"] = float(np.median(v))
        row[f"{k}_ms_iqr"] = [float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    row["ensemble_over_single"] = row["ensemble_ms"] / row["single_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="1,10,36")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("certificate_times: no GPU (times are taken on the device or not at all)")
    from revs_admm_amd import build
    build.build()
    rows = []
    for S in [int(s) for s in a.sizes.split(",")]:
        rows.append(time_case(S, a.reps))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
