"""float64 numpy restatement of revs_flex_report (include/revs_admm_ops.h, "flexibility report"): the contract, a plain
loop over the slots with every double operation a numpy operation of its own.  Nothing here knows how the device maps
rows to threads.  The records and powers are charge_ref's."""
import numpy as np

from charge_ref import same_bits, same_or_within

ROW_F = ("up_energy", "down_energy", "laxity", "energy")
ROW_INT = ("ready", "slack", "n_up", "n_down", "flags")
SLOT_INT = ("n_plugged", "n_up", "n_down", "reserved")
DAY_INT = ("n_ev", "n_never_ready", "n_unservable", "n_late", "n_rigid", "reserved")
QUANTITIES = ("up_energy", "down_energy", "slack", "laxity")


class Ref:
    """up, down: (S, n, T) float64, every row's reserve per slot; row: dict of (S, n) arrays; slot: dict of (S, T);
    day: dict of (S,); hist (S, 2, T + 1); val (4, S, n); keep (S, n); abs_up, abs_down (S, T): the sums of magnitudes the
    summation bounds are made of."""


def min2(a, b):
    return np.where(b < a, b, a)


def q36(x):
    """common.h's revs_q36: rounding to a multiple of 2^-36 (below 2^16 in magnitude)."""
    return (x + 98304.0) - 98304.0


def scan_peaks(x):
    """The day record's scan of one scenario's slot sums -> (energy, peak, peak slot): t ascending from +0.0, the peak
    moves on `>` only."""
    pk, pks, en = x[0], 0, 0.0
    with np.errstate(all="ignore"):
        for t in range(len(x)):
            en = en + x[t]
            if x[t] > pk:
                pk, pks = x[t], t
    return np.float64(en), np.float64(pk), pks


def report(p, homes, integral=0, on_frac=0.0, short_tol=1e-6):
    """p (S, n, T) float32, homes HOME_DTYPE (S, n) -> Ref."""
    p = np.asarray(p, np.float32)
    S, n, T = p.shape
    assert homes.shape == (S, n)
    ev = homes["ev"] != 0
    ws = np.clip(homes["start"].astype(np.int64), 0, T)
    we = np.clip(homes["end"].astype(np.int64), 0, T)
    W = np.maximum(we - ws, 0)
    r = homes["rating"].astype(np.float64)
    c = homes["capacity"].astype(np.float64)
    i0 = homes["initial"].astype(np.float64)
    tol = np.float64(short_tol)
    up, down = np.zeros((S, n, T)), np.zeros((S, n, T))
    done = np.zeros((S, n))
    bad = np.zeros((S, n), bool)
    ready = np.full((S, n), -1, np.int64)
    with np.errstate(all="ignore"):
        tgt = np.where(i0 > 0.9, i0, 0.9)
        E_lo = (tgt - i0) * c
        E_hi = (1.0 - i0) * c
        thr = np.float64(on_frac) * r
        for t in range(T + 1):
            short = tgt - (i0 + done / c) > tol
            ready = np.where((ready < 0) & ~short, t, ready)
            if t == T:
                break
            d = p[:, :, t].astype(np.float64)
            inwin = (ws <= t) & (t < we)
            m = min2(r - d, (E_hi - done) - d)
            u = np.where(m > 0, np.where(m < r, m, r), 0.0)
            A = np.maximum(we - np.maximum(t + 1, ws), 0).astype(np.float64) * r
            m = ((done + d) + A) - E_lo
            q = np.where(d < r, d, r)
            dn = np.where((m > 0) & (q > 0), min2(q, m), 0.0)
            if integral:
                u = np.where(u >= r, r, 0.0)
                dn = np.where((d > thr) & (m >= d) & (q > 0), q, 0.0)
            up[:, :, t] = np.where(inwin & ev, u, 0.0)
            down[:, :, t] = np.where(inwin & ev, dn, 0.0)
            bad |= ~np.isfinite(d)
            done = done + d
        laxity = W.astype(np.float64) - E_lo / r
        unserv = E_lo > W.astype(np.float64) * r
    up_e, down_e = np.zeros((S, n)), np.zeros((S, n))
    for t in range(T):
        up_e, down_e = up_e + up[:, :, t], down_e + down[:, :, t]
    ready = np.where(ev, ready, -1)
    slack = np.where(ready >= 0, we - ready, 0)
    n_up, n_down = (up > 0).sum(2), (down > 0).sum(2)
    flags = 1 + 2 * (ready < 0) + 4 * bad + 8 * unserv + 16 * (ready > we)
    mask = lambda a, fill=0: np.where(ev, a, fill)
    out = Ref()
    out.up, out.down = up, down
    out.row = dict(up_energy=mask(up_e, 0.0), down_energy=mask(down_e, 0.0), laxity=mask(laxity, 0.0), energy=mask(done, 0.0),
                   ready=ready, slack=mask(slack), n_up=mask(n_up), n_down=mask(n_down), flags=mask(flags))
    keep = ev & ~bad
    out.keep = keep.astype(np.uint8)
    nan = np.nan
    out.val = np.stack([np.where(keep, up_e, nan), np.where(keep, down_e, nan),
                        np.where(keep & (ready >= 0), slack.astype(np.float64), nan), np.where(keep, laxity, nan)])
    slot = {k: np.zeros((S, T), np.int64) for k in SLOT_INT}
    slot["up"], slot["down"] = np.zeros((S, T)), np.zeros((S, T))
    t_ = np.arange(T)[None, None, :]
    slot["n_plugged"][:] = (ev[:, :, None] & (ws[:, :, None] <= t_) & (t_ < we[:, :, None])).sum(1)
    slot["n_up"][:], slot["n_down"][:] = (up > 0).sum(1), (down > 0).sum(1)
    for s in range(S):
        for t in range(T):                                   # (any fixed order: within the bound)
            slot["up"][s, t] = sum(up[s, :, t].tolist(), 0.0)
            slot["down"][s, t] = sum(down[s, :, t].tolist(), 0.0)
    out.abs_up, out.abs_down = np.abs(up).sum(1), np.abs(down).sum(1)
    day = {k: np.zeros(S, np.int64) for k in DAY_INT + ("peak_up_slot", "peak_down_slot")}
    day.update({k: np.zeros(S) for k in ("up_energy", "down_energy", "peak_up", "peak_down")})
    hist = np.zeros((S, 2, T + 1), np.int64)
    for s in range(S):
        e = ev[s]
        nev = int(e.sum())
        for k in ("up", "down"):
            en, pk, pks = scan_peaks(slot[k][s])
            day[k + "_energy"][s], day["peak_" + k][s], day["peak_" + k + "_slot"][s] = en, pk, pks if nev else -1
        day["n_ev"][s], day["n_never_ready"][s] = nev, (e & (ready[s] < 0)).sum()
        day["n_unservable"][s], day["n_late"][s] = (e & unserv[s]).sum(), (e & (ready[s] > we[s])).sum()
        day["n_rigid"][s] = (e & (n_up[s] == 0) & (n_down[s] == 0)).sum()
        ok = e & (ready[s] >= 0)
        np.add.at(hist[s, 0], ready[s][ok], 1)
        np.add.at(hist[s, 1], slack[s][ok & (slack[s] >= 0) & (slack[s] <= T)], 1)
    out.slot, out.day, out.hist = slot, day, hist
    return out


def node_sums(x, node_ptr):
    """x (S, n, T) -> (S, m, T): the sum of q36(x) over each node's rows (exact additions: any order gives these bits)."""
    S, n, T = x.shape
    m = len(node_ptr) - 1
    out = np.zeros((S, m, T))
    q = q36(x)
    for j in range(m):
        if node_ptr[j + 1] > node_ptr[j]:
            out[:, j] = q[:, node_ptr[j]:node_ptr[j + 1]].sum(1)
    return out


def check(ref, row=None, slot=None, day=None, hist=None, val=None, keep=None, node_up=None, node_down=None,
          node_ptr=None, what=""):
    """The outputs of revs_flex_report (structured arrays; None: not asked for) against `ref`: row records, val, keep,
    hist, every integer and the node sums bit for bit; the slot and day sums within count 2^-53 sum|x|; the day record
    equals the function of the slot records of the same call bit for bit."""
    u = 2.0 ** -53
    if row is not None:
        for k in ROW_INT:
            assert (row[k] == ref.row[k]).all(), (what, "row", k)
        for k in ROW_F:
            assert same_bits(row[k], ref.row[k].astype(np.float64)), (what, "row", k)
        assert not row["reserved"].any(), (what, "row reserved")
    n_ev = ref.day["n_ev"]
    T = ref.up.shape[2]
    if slot is not None:
        for k in SLOT_INT:
            assert (slot[k] == ref.slot[k]).all(), (what, "slot", k)
        same_or_within(slot["up"], ref.slot["up"], n_ev[:, None] * u * ref.abs_up, (what, "slot up"))
        same_or_within(slot["down"], ref.slot["down"], n_ev[:, None] * u * ref.abs_down, (what, "slot down"))
    if day is not None:
        for k in DAY_INT:
            assert (day[k] == ref.day[k]).all(), (what, "day", k)
        for k, a in (("up", ref.abs_up), ("down", ref.abs_down)):
            bound = (n_ev[:, None] * u * a).sum(1) + T * u * np.abs(ref.slot[k]).sum(1)
            same_or_within(day[k + "_energy"], ref.day[k + "_energy"], bound, (what, "day energy", k))
            same_or_within(day["peak_" + k], ref.day["peak_" + k], (n_ev[:, None] * u * a).max(1), (what, "day peak", k))
            assert ((day["peak_" + k + "_slot"] >= 0) == (n_ev > 0)).all(), (what, "peak slot", k)
        if slot is not None:
            for s in range(len(n_ev)):
                for k in ("up", "down"):
                    en, pk, pks = scan_peaks(slot[k][s])
                    assert same_bits(en, day[k + "_energy"][s]), (what, "day energy of the slots", k, s)
                    assert same_bits(pk, day["peak_" + k][s]), (what, "peak", k, s)
                    assert int(day["peak_" + k + "_slot"][s]) == (pks if n_ev[s] else -1), (what, "peak slot", k, s)
    if hist is not None:
        assert (hist == ref.hist).all(), (what, "hist")
    if val is not None:
        assert same_bits(val, ref.val.astype(np.float64)), (what, "val")
    if keep is not None:
        assert (keep == ref.keep).all(), (what, "keep")
    if node_up is not None:
        assert node_up.tobytes() == node_sums(ref.up, node_ptr).tobytes(), (what, "node_up")
    if node_down is not None:
        assert node_down.tobytes() == node_sums(ref.down, node_ptr).tobytes(), (what, "node_down")
