"""numpy yard-stick of the load-profile report (test-altered-profile.py:25-57: the residences' load per slot, with and
without EVs): every cell a bills_ref.record -- numpy.percentile / boxplot_stats, math.fsum for the total -- with n_above
as conv_ref.record counts it, built by plain loops over scenarios, sets and slots; the residences' own peaks by numpy.max
per row; the day figures by the formulas of revs_profile_day_t from given totals.  Nothing here knows of tiles, chunks
or the order of a sum.  Profiles are (S, n, T): scenario, residence, slot; classes (S, n) integers or None."""
import numpy as np

import bills_ref as br
import conv_ref as cr


def set_masks(classes, C, S, n):
    """-> Q = C + 1 boolean (S, n) masks: class 0 .. C-1, then every residence with a class; C == 0: the one set of all."""
    if C == 0:
        assert classes is None
        return [np.ones((S, n), bool)]
    c = np.asarray(classes).astype(np.int64).reshape(S, n)
    masks = [c == q for q in range(C)]
    return masks + [(c >= 0) & (c < C)]


def peaks(g):
    """(S, n, T) -> (S, n) float32: every residence's own daily peak, numpy.max per row; a row that holds a value that is
    not finite gives a NaN (numpy.max propagates a NaN; the report's contract treats an infinity in the row alike)."""
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        x = np.max(g, axis=2)
    return np.where(np.isfinite(g).all(axis=2), x, np.float32(np.nan)).astype(np.float32)


def slot_records(g, masks, members, above, index=None):
    """-> [Q][T] dicts over g[s, i, t] for s in members, residences of the set."""
    g = np.asarray(g, np.float32)
    return [[cr.record(g[:, :, t], m, members, above, index) for t in range(g.shape[2])] for m in masks]


def peak_records(g, masks, members, above, index=None):
    x = peaks(g)
    return [cr.record(x, m, members, above, index) for m in masks]


def day_record(totals, counts, sum_peaks):
    """revs_profile_day_t from the slot totals A[t] (over the slots with count > 0) and the peak record's total."""
    nan = float("nan")
    d = dict(peak=nan, valley=nan, energy=nan, load_factor=nan, sum_peaks=nan, diversity=nan, peak_slot=-1, valley_slot=-1,
             slots=0, reserved=0)
    energy = np.float64(0.0)
    for t, (a, c) in enumerate(zip(totals, counts)):
        if c <= 0:
            continue
        a = np.float64(a)
        if d["slots"] == 0 or a > d["peak"]:
            d["peak"], d["peak_slot"] = a, t
        if d["slots"] == 0 or a < d["valley"]:
            d["valley"], d["valley_slot"] = a, t
        energy = energy + a
        d["slots"] += 1
    if d["slots"]:
        with np.errstate(all="ignore"):
            d["energy"] = energy
            d["load_factor"] = (energy / np.float64(d["slots"])) / d["peak"]
            d["sum_peaks"] = np.float64(sum_peaks)
            d["diversity"] = d["sum_peaks"] / d["peak"]
    return d


def check_day(got, ref, what=""):
    """A PROFILE_DAY_DTYPE record against day_record(): bit for bit."""
    for k in ("peak_slot", "valley_slot", "slots", "reserved"):
        assert int(got[k]) == ref[k], (what, k, got, ref)
    for k in ("peak", "valley", "energy", "load_factor", "sum_peaks", "diversity"):
        a, b = np.float64(got[k]), np.float64(ref[k])
        assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (what, k, got[k], ref[k])


def check_days(day, slot, peak, what=""):
    """day (S, Q) against the formulas applied to the SAME report's slot (S, Q, T) and peak (S, Q) records."""
    for s in range(slot.shape[0]):
        for q in range(slot.shape[1]):
            check_day(day[s, q], day_record(slot[s, q]["total"], slot[s, q]["count"], peak[s, q]["total"]), (what, s, q))


def check_report(rep, g, classes, C, above, index=None, groups=None, what=""):
    """Every record of a LoadProfileReport-like (slot, peak, day, pooled_slot, pooled_peak; any may be None) against the
    yard-stick on g (S, n, T) float32."""
    g = np.asarray(g, np.float32)
    S, n, T = g.shape
    masks = set_masks(classes, C, S, n)
    Q = len(masks)
    for s in range(S):
        if rep.slot is not None:
            assert rep.slot.shape == (S, Q, T)
            ref = slot_records(g, masks, [s], above, index)
            for q in range(Q):
                for t in range(T):
                    br.check_record(rep.slot[s, q, t], ref[q][t], (what, "slot", s, q, t))
        if rep.peak is not None:
            assert rep.peak.shape == (S, Q)
            ref = peak_records(g, masks, [s], above, index)
            for q in range(Q):
                br.check_record(rep.peak[s, q], ref[q], (what, "peak", s, q))
    if rep.day is not None and rep.slot is not None and rep.peak is not None:
        check_days(rep.day, rep.slot, rep.peak, what)
    if groups is not None:
        G = int(max(groups)) + 1
        for gid in range(G):
            members = [s for s in range(S) if groups[s] == gid]
            if rep.pooled_slot is not None:
                assert rep.pooled_slot.shape == (G, Q, T)
                ref = slot_records(g, masks, members, above, index)
                for q in range(Q):
                    for t in range(T):
                        br.check_record(rep.pooled_slot[gid, q, t], ref[q][t], (what, "pool slot", gid, q, t))
            if rep.pooled_peak is not None:
                ref = peak_records(g, masks, members, above, index)
                for q in range(Q):
                    br.check_record(rep.pooled_peak[gid, q], ref[q], (what, "pool peak", gid, q))
