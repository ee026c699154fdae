"""float64 numpy restatement of revs_charge_report (include/revs_admm_ops.h, "charging report"): the contract, a plain
loop over the slots with every double operation a numpy operation of its own.  Nothing here knows how the device maps
rows to threads.  Also the records and powers the charging tests share: random ones and one of each awkward row."""
import numpy as np

ROW_INT = ("n_on", "n_full", "first_on", "last_on", "sessions", "wait", "n_outside", "flags")
SLOT_INT = ("n_ev", "n_plugged", "n_on", "n_full", "n_starts", "reserved")
DAY_INT = ("peak_on", "peak_on_slot", "peak_power_slot", "n_ev", "n_under", "n_never", "n_interrupted", "n_outside")


class Ref:
    """row: dict of (S, n) arrays; slot: dict of (S, T); day: dict of (S,); hist (S, 3, T + 1); val (4, S, n); keep (S, n);
    abs_power (S, T), abs_cost (S,): the sums of magnitudes the summation bounds are made of."""


def report(p, homes, tariff=None, on_frac=0.0, short_tol=1e-6):
    """p (S, n, T) float32, homes HOME_DTYPE (S, n), tariff (T,) float64 or None -> Ref."""
    p = np.asarray(p, np.float32)
    S, n, T = p.shape
    assert homes.shape == (S, n)
    ev = homes["ev"] != 0
    ws = np.clip(homes["start"].astype(np.int64), 0, T)
    we = np.clip(homes["end"].astype(np.int64), 0, T)
    rating = homes["rating"].astype(np.float64)
    cap = homes["capacity"].astype(np.float64)
    ini = homes["initial"].astype(np.float64)
    thr = np.float64(on_frac) * rating
    z = lambda: np.zeros((S, n), np.int64)
    energy, cost = np.zeros((S, n)), np.zeros((S, n)) if tariff is not None else np.full((S, n), np.nan)
    n_on, n_full, sessions, n_outside = z(), z(), z(), z()
    first_on, last_on = z() - 1, z() - 1
    prev, bad = np.zeros((S, n), bool), np.zeros((S, n), bool)
    slot = {k: np.zeros((S, T), np.int64) for k in SLOT_INT}
    slot["power"], abs_power = np.zeros((S, T)), np.zeros((S, T))
    with np.errstate(all="ignore"):
        for t in range(T):
            d = p[:, :, t].astype(np.float64)
            energy = energy + d
            if tariff is not None:
                cost = cost + np.float64(tariff[t]) * d
            bad |= ~np.isfinite(d)
            on = ev & (d > thr)
            full = on & (d >= rating)
            start = on & ~prev
            plugged = ev & (ws <= t) & (t < we)
            n_on += on
            n_full += full
            sessions += start
            n_outside += on & ~plugged
            first_on = np.where(on & (first_on < 0), t, first_on)
            last_on = np.where(on, t, last_on)
            prev = on
            slot["n_plugged"][:, t], slot["n_on"][:, t] = plugged.sum(1), on.sum(1)
            slot["n_full"][:, t], slot["n_starts"][:, t] = full.sum(1), start.sum(1)
            for s in range(S):
                x = d[s][ev[s]]
                slot["power"][s, t] = sum(x.tolist(), 0.0)            # (any fixed order: within the bound)
                abs_power[s, t] = np.abs(x[np.isfinite(x)]).sum()
        soc = ini + energy / cap
        under = ev & (np.where(ini > 0.9, ini, 0.9) - soc > np.float64(short_tol))
    slot["n_ev"][:] = ev.sum(1)[:, None]
    wait = np.where(first_on >= 0, first_on - ws, -1)
    out = Ref()
    mask = lambda a, fill=0: np.where(ev, a, fill)
    out.row = dict(energy=mask(energy, 0.0), cost=mask(cost, 0.0), soc_end=mask(soc.astype(np.float32), np.float32(0)),
                   reserved0=np.zeros((S, n), np.float32), n_on=n_on, n_full=n_full, first_on=first_on, last_on=last_on,
                   sessions=sessions, wait=wait, n_outside=n_outside,
                   flags=mask(1 + 2 * under.astype(np.int64) + 4 * bad.astype(np.int64)))
    out.slot = slot
    keep = ev & ~bad
    nan = np.nan
    out.keep = keep.astype(np.uint8)
    out.val = np.stack([np.where(keep, energy, nan), np.where(keep, cost, nan),
                        np.where(keep, soc.astype(np.float32).astype(np.float64), nan),
                        np.where(keep & (first_on >= 0), wait.astype(np.float64), nan)])
    hist = np.zeros((S, 3, T + 1), np.int64)
    day = {k: np.zeros(S, np.int64) for k in DAY_INT}
    day.update(peak_power=np.zeros(S), energy=np.zeros(S), coincidence=np.zeros(S), cost=np.zeros(S))
    abs_cost = np.zeros(S)
    for s in range(S):
        e = ev[s]
        np.add.at(hist[s, 0], n_on[s][e], 1)
        np.add.at(hist[s, 1], wait[s][e & (first_on[s] >= 0) & (wait[s] >= 0)], 1)
        np.add.at(hist[s, 2], sessions[s][e], 1)
        pw, no = slot["power"][s], slot["n_on"][s]
        pk, pks, po, pos, en = pw[0], 0, no[0], 0, 0.0
        with np.errstate(all="ignore"):
            for t in range(T):
                en = en + pw[t]
                if pw[t] > pk:
                    pk, pks = pw[t], t
                if no[t] > po:
                    po, pos = no[t], t
            day["cost"][s] = sum(cost[s][e].tolist(), 0.0)
        c = cost[s][e]
        abs_cost[s] = np.abs(c[np.isfinite(c)]).sum()
        nev = int(e.sum())
        day["peak_power"][s], day["energy"][s] = pk, en
        day["coincidence"][s] = po / nev if nev else np.nan
        day["peak_on"][s], day["peak_on_slot"][s], day["peak_power_slot"][s] = po, pos if nev else -1, pks if nev else -1
        day["n_ev"][s], day["n_under"][s], day["n_never"][s] = nev, under[s].sum(), (e & (n_on[s] == 0)).sum()
        day["n_interrupted"][s], day["n_outside"][s] = (e & (sessions[s] > 1)).sum(), (e & (n_outside[s] > 0)).sum()
    out.day, out.hist, out.abs_power, out.abs_cost = day, hist, abs_power, abs_cost
    return out


def same_or_within(a, b, bound, what):
    """a and b agree within `bound` where both are finite, and are the same special value elsewhere."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    assert (np.isnan(a) == np.isnan(b)).all() and (a[~fin & ~np.isnan(a)] == b[~fin & ~np.isnan(a)]).all(), what
    assert (np.abs(a - b)[fin] <= np.broadcast_to(bound, a.shape)[fin]).all(), (what, np.abs(a - b)[fin].max())


def same_bits(a, b):
    """Bit for bit, except that a NaN equals any NaN: IEEE leaves the sign and payload of a NaN an operation makes
    (inf - inf, 0 inf) to the machine, and the host's and the device's differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def check(ref, row=None, slot=None, day=None, hist=None, val=None, keep=None, what=""):
    """The outputs of revs_charge_report (structured arrays; None: not asked for) against `ref`: integers, flags, hist and
    keep equal; energy, cost, soc_end and val bit for bit; slot power, day energy and day cost within the summation bound
    count 2^-53 sum|x| (a non-finite sum: the same special value, where the order cannot change it)."""
    u = 2.0 ** -53
    if row is not None:
        for k in ROW_INT:
            assert (row[k] == ref.row[k]).all(), (what, "row", k)
        for k in ("energy", "cost"):
            assert same_bits(row[k], ref.row[k].astype(np.float64)), (what, "row", k)
        assert same_bits(row["soc_end"], ref.row["soc_end"].astype(np.float32)), (what, "soc_end")
        assert not row["reserved"].any() and not row["reserved0"].any(), (what, "row reserved")
    n_ev = ref.day["n_ev"]
    if slot is not None:
        for k in SLOT_INT:
            assert (slot[k] == ref.slot[k]).all(), (what, "slot", k)
        same_or_within(slot["power"], ref.slot["power"], n_ev[:, None] * u * ref.abs_power, (what, "power"))
    if day is not None:
        for k in DAY_INT:
            if k in ("peak_power_slot",):
                continue
            assert (day[k] == ref.day[k]).all(), (what, "day", k)
        assert (np.isnan(day["coincidence"]) == (n_ev == 0)).all()
        ok = n_ev > 0
        assert day["coincidence"][ok].tobytes() == ref.day["coincidence"][ok].tobytes(), (what, "coincidence")
        T = ref.slot["power"].shape[1]
        fin = np.isfinite(ref.slot["power"]).all(1)
        bound = (n_ev[:, None] * u * ref.abs_power).sum(1) + T * u * np.abs(np.where(fin[:, None], ref.slot["power"], 0)).sum(1)
        same_or_within(day["energy"], ref.day["energy"], bound, (what, "day energy"))
        same_or_within(day["cost"], ref.day["cost"], n_ev * u * ref.abs_cost, (what, "day cost"))
        if slot is not None:                       # the day record is a function of the slot records of the same call
            for s in range(len(n_ev)):
                pw = slot["power"][s]
                pk, pks, en = pw[0], 0, 0.0
                with np.errstate(all="ignore"):
                    for t in range(T):
                        en = en + pw[t]
                        if pw[t] > pk:
                            pk, pks = pw[t], t
                assert same_bits(np.float64(pk), day["peak_power"][s]), (what, "peak_power", s)
                assert same_bits(np.float64(en), day["energy"][s]), (what, "day energy of the slots", s)
                assert int(day["peak_power_slot"][s]) == (pks if n_ev[s] else -1), (what, "peak_power_slot", s)
    if hist is not None:
        assert (hist == ref.hist).all(), (what, "hist")
    if val is not None:
        assert val.tobytes() == ref.val.astype(np.float64).tobytes(), (what, "val")
    if keep is not None:
        assert (keep == ref.keep).all(), (what, "keep")


# ---- records and powers -------------------------------------------------------------------------------------------------
AWKWARD = ("on_at_0", "on_at_last", "alternating", "exactly_rating", "just_below_rating", "just_above_threshold",
           "at_threshold", "negative", "nan", "pos_inf", "neg_inf", "start_below_0", "end_beyond_T", "end_before_start",
           "no_ev_with_power", "short_by_more", "short_by_less")


def awkward_rows(T, on_frac, short_tol):
    """(records, p (len, T) float32): one row of each awkward case, in AWKWARD's order."""
    from revs_admm_amd.engine import pack_homes
    f = np.float32
    r = f(4.8)
    rec = pack_homes([True] * len(AWKWARD), 4.8, 20.0, 0.2, min(1, T - 1), T)
    p = np.zeros((len(AWKWARD), T), f)
    k = {name: i for i, name in enumerate(AWKWARD)}
    p[k["on_at_0"], 0] = r
    p[k["on_at_last"], T - 1] = r
    p[k["alternating"], ::2] = r
    p[k["exactly_rating"], T // 2] = r
    p[k["just_below_rating"], T // 2] = np.nextafter(r, f(0))
    thr = f(np.float64(on_frac) * np.float64(r))             # at or just below the double threshold
    p[k["at_threshold"], T // 2] = thr if np.float64(thr) <= np.float64(on_frac) * np.float64(r) else np.nextafter(thr, f(-1))
    p[k["just_above_threshold"], T // 2] = np.nextafter(p[k["at_threshold"], T // 2], f(10))
    if np.float64(p[k["just_above_threshold"], T // 2]) <= np.float64(on_frac) * np.float64(r):
        p[k["just_above_threshold"], T // 2] = np.nextafter(p[k["just_above_threshold"], T // 2], f(10))
    p[k["negative"]] = -1.5
    p[k["negative"], T - 1] = r
    p[k["nan"], T - 1], p[k["nan"], 0] = r, np.nan           # (T == 1: the NaN stays)
    p[k["pos_inf"], T // 2], p[k["neg_inf"], T // 2] = np.inf, -np.inf
    for name in ("start_below_0", "end_beyond_T", "end_before_start"):
        p[k[name]] = r
    rec["start"][k["start_below_0"]] = -3
    rec["end"][k["end_beyond_T"]] = T + 7
    rec["start"][k["end_before_start"]], rec["end"][k["end_before_start"]] = T - 1, 0
    rec["ev"][k["no_ev_with_power"]] = 0
    p[k["no_ev_with_power"]] = np.nan
    p[k["no_ev_with_power"], 0] = r
    # the shortfall 0.9 - (0.2 + e / capacity) straddles short_tol: e = 1 (float32, exact), capacities either side
    want = (0.7 - np.array([2.0, 0.5]) * max(short_tol, 1e-9))
    for name, w in zip(("short_by_more", "short_by_less"), want):
        p[k[name], 0] = 1.0
        rec["capacity"][k[name]] = f(1.0 / w)
    return rec, p


def random_case(rng, S, n, T, on_frac=0.0, short_tol=1e-6):
    """-> (p (S, n, T) float32, homes (S, n)): the awkward rows first (as many as fit), then rows of three kinds -- on/off at
    the rating, continuous powers, mostly idle -- with windows in and beyond 0..T; with S > 1, scenario 1 has no EV."""
    from revs_admm_amd.engine import pack_homes
    f = np.float32
    start = rng.integers(-2, T + 1, (S, n))
    end = start + rng.integers(0, T + 4, (S, n))
    homes = np.empty((S, n), awkward_rows(max(T, 1), on_frac, short_tol)[0].dtype)
    p = np.zeros((S, n, T), f)
    for s in range(S):
        homes[s] = pack_homes(rng.random(n) < 0.7, rng.choice([1.2, 3.3, 4.8, 7.2], n), rng.uniform(10.0, 80.0, n),
                              rng.uniform(0.05, 0.98, n), start[s], end[s])
        kind = rng.integers(0, 3, n)
        onoff = (rng.random((n, T)) < 0.35) * homes[s]["rating"][:, None]
        cont = rng.uniform(-0.2, 1.1, (n, T)) * homes[s]["rating"][:, None]
        idle = (rng.random((n, T)) < 0.05) * rng.uniform(0, 5, (n, T))
        p[s] = np.where(kind[:, None] == 0, onoff, np.where(kind[:, None] == 1, cont, idle)).astype(f)
    arec, ap = awkward_rows(T, on_frac, short_tol)
    m = min(n, len(arec))
    pick = rng.permutation(len(arec))[:m] if m < len(arec) else np.arange(m)
    homes[0, :m], p[0, :m] = arec[pick], ap[pick]
    if S > 1:
        homes["ev"][1] = 0
    return p, homes
