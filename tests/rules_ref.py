"""float64 numpy restatement of revs_rule_schedule (include/revs_admm_ops.h, "rule schedules"): the contract, row by row,
with every double operation a numpy operation of its own.  Nothing here knows how the device maps elements to threads.
Also the records the tests of the rule schedules share: random ones and one of each edge case."""
import numpy as np

ASAP, ALAP, EVEN = 0, 1, 2
TARGET, FULL = 0, 1
POLICY = {"uncontrolled": ASAP, "last_minute": ALAP, "trickle": EVEN}
FILL = {"target": TARGET, "full": FULL}


def combos():
    """Every (policy, fill, integral) the entry point accepts."""
    return [(p, f, i) for p in (ASAP, ALAP, EVEN) for f in (TARGET, FULL) for i in (1, 0) if not (p == EVEN and i)]


def plan(homes, T, policy, fill, integral):
    """The per-row quantities every element is a function of -> dict of (n,) arrays."""
    ev = homes["ev"] != 0
    ws = np.clip(homes["start"].astype(np.int64), 0, T)
    we = np.clip(homes["end"].astype(np.int64), 0, T)
    W = np.maximum(we - ws, 0)
    nmin, nmax = homes["nmin"].astype(np.int64), homes["nmax"].astype(np.int64)
    rating = homes["rating"].astype(np.float64)
    cap = homes["capacity"].astype(np.float64)
    ini = homes["initial"].astype(np.float64)
    empty = ev & ((nmax < 0) | ((nmin > nmax) if integral else False))
    act = ev & ~empty
    rem = np.zeros(len(homes))
    even = np.zeros(len(homes))
    with np.errstate(all="ignore"):
        if integral:
            k = nmax if fill == FULL else nmin
            on = np.minimum(k, W)
            status = on < nmin
            kf = np.maximum(on, 0)
            partial = np.zeros(len(homes), bool)
            E_want = k.astype(np.float64)
        else:
            top = np.where(ini > 0.9, ini, 0.9)
            elo = (top - ini) * cap
            ehi = (1.0 - ini) * cap
            E = ehi if fill == FULL else elo
            rw = rating * W.astype(np.float64)
            D = np.where(rw < E, rw, E)
            status = D < elo
            E_want = E
            if policy == EVEN:
                even = np.where(W > 0, D / np.where(W > 0, W, 1).astype(np.float64), 0.0)
                kf = np.zeros(len(homes), np.int64)
                partial = np.zeros(len(homes), bool)
            else:
                q = np.floor(D / rating)
                kf = np.where(rating > 0.0, np.where(q >= W, W, np.where(q > 0.0, q, 0.0)), 0.0).astype(np.int64)
                r = D - kf.astype(np.float64) * rating
                partial = kf < W
                rem = np.where(partial & (r > 0.0), r, 0.0)
    W = np.where(act, W, 0)
    kf = np.where(act, kf, 0)
    partial = partial & act
    if policy == ALAP:
        first = W - kf
        part = np.where(partial, W - kf - 1, -1)
    else:
        first = np.zeros_like(W)
        part = np.where(partial, kf, -1)
    status = np.where(act, status, empty).astype(np.int32)
    return dict(ev=ev, empty=empty, act=act, ws=ws, W=W, kf=kf, first=first, part=part, rem=rem, even=even, rating=rating,
                cap=cap, ini=ini, status=status, E_want=E_want)


def rule_schedule(homes, load, policy, fill, integral, T=None):
    """-> (p (n, T) float32, soc (n, T + 1) float32, g (n, T) float32 or None without load, status (n,) int32)."""
    if load is not None:
        load = np.asarray(load, np.float32)
        T = load.shape[1]
    P = plan(homes, T, policy, fill, integral)
    col = lambda a: a[:, None]
    j = np.arange(T)[None, :] - col(P["ws"])
    inwin = (j >= 0) & (j < col(P["W"]))
    rating32 = homes["rating"].astype(np.float32)
    if policy == EVEN and not integral:
        p = np.where(inwin, col(P["even"].astype(np.float32)), np.float32(0))
    else:
        full = inwin & (j >= col(P["first"])) & (j < col(P["first"] + P["kf"]))
        part = inwin & (j == col(P["part"]))
        p = np.where(full, col(rating32), np.where(part, col(P["rem"].astype(np.float32)), np.float32(0)))
    p = p.astype(np.float32)
    jt = np.clip(np.arange(T + 1)[None, :] - col(P["ws"]), 0, col(P["W"]))
    with np.errstate(all="ignore"):
        if policy == EVEN and not integral:
            E = jt.astype(np.float64) * col(P["even"])
        else:
            nf = np.clip(jt - col(P["first"]), 0, col(P["kf"]))
            E = nf.astype(np.float64) * col(P["rating"])
            E = np.where((col(P["part"]) >= 0) & (jt > col(P["part"])), E + col(P["rem"]), E)
        soc = (col(P["ini"]) + E / col(P["cap"])).astype(np.float32)
    ini32 = homes["initial"].astype(np.float32)
    soc[:, 0] = ini32
    soc = np.where(col(P["empty"]), col(ini32), soc)
    soc = np.where(col(P["ev"]), soc, np.float32(0)).astype(np.float32)
    g = None if load is None else (load + p).astype(np.float32)
    return p, soc, g, P["status"]


def soc_recurrence(homes, p):
    """s[t + 1] = s[t] + p[t] / capacity in float64 over the float32 powers, from the record's initial; 0 without an EV."""
    p = np.asarray(p, np.float32).astype(np.float64)
    cap = homes["capacity"].astype(np.float64)
    s = np.empty((p.shape[0], p.shape[1] + 1))
    s[:, 0] = homes["initial"].astype(np.float64)
    for t in range(p.shape[1]):
        s[:, t + 1] = s[:, t] + p[:, t] / cap
    return np.where((homes["ev"] != 0)[:, None], s, 0.0)


# ---- records ---------------------------------------------------------------------------------------------------------
EDGE_CASES = ("no_ev", "empty_window", "end_beyond_T", "one_slot_at_end", "k_zero", "k_equals_W", "k_above_W",
              "exact_multiple", "nmax_negative", "nmin_above_nmax", "rating_zero", "rating_zero_rows_open")


def edge_records(T):
    """One record of each edge case, in EDGE_CASES' order.  (At a T too small for a case's window the window is what
    fits: the record is still a valid one.)"""
    from revs_admm_amd.engine import pack_homes
    r48 = float(np.float32(4.8))
    one = lambda ev=True, rating=4.8, cap=20.0, ini=0.2, start=0, end=T: pack_homes([ev], rating, cap, ini, start, end)[0]
    recs = [
        one(ev=False, start=1, end=T),
        one(start=min(3, T), end=min(2, T)),                     # start >= end
        one(start=max(T - 2, 0), end=T + 5),
        one(start=T - 1, end=T),
        one(ini=0.93),                                           # nmin = 0, E_lo = 0
        one(start=max(T - 3, 0), end=T),                         # 4.8 kW, 20 kWh from 0.2: nmin = nmax = 3 = W (T >= 3)
        one(start=max(T - 2, 0), end=T),                         # ... and W = 2 < 3
        one(rating=r48, cap=4 * r48, ini=0.5, start=max(T - 4, 0), end=T),    # E_hi = 2 rating exactly
        one(ini=1.3),                                            # nmax = -1
        one(ini=0.85),                                           # nmin = 1 > nmax = 0
        one(rating=0.0),
        one(rating=0.0),
    ]
    rec = np.array(recs, dtype=recs[0].dtype)
    rec["nmin"][-1], rec["nmax"][-1] = 0, 5                      # rating = 0 with the on/off rows open
    assert len(rec) == len(EDGE_CASES)
    return rec


def random_records(rng, n, T):
    from revs_admm_amd.engine import pack_homes
    start = rng.integers(-2, T + 1, n)
    end = start + rng.integers(0, T + 4, n)
    return pack_homes(rng.random(n) < 0.75, rng.choice([1.2, 3.3, 4.8, 7.2, 11.5], n), rng.uniform(10.0, 80.0, n),
                      rng.uniform(0.05, 0.98, n), start, end)


def records(rng, n, T):
    """n records: the edge cases first (as many as fit, at least the whole set when n allows), random ones behind."""
    edge = edge_records(T)
    if n <= len(edge):
        return edge[rng.permutation(len(edge))[:n]] if n < len(edge) else edge
    return np.concatenate([edge, random_records(rng, n - len(edge), T)])
