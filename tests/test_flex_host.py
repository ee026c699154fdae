"""The numpy restatement of the flexibility report (tests/flex_ref.py) is the definition it claims to be: no GPU here.  The
two anchors -- a last-minute schedule to the target has nothing left to cut, an uncontrolled one to full nothing left to
add -- on the rule schedules of rules_ref; what up and down mean, by applying them to the schedule and following the state
of charge; and the awkward rows of charge_ref."""
import numpy as np
import pytest

import charge_ref as cr
import flex_ref as fr
import rules_ref as rr

N = 3000


def _rule_case(T, policy, fill, integral):
    rng = np.random.default_rng(100 + T)
    homes = rr.records(rng, N, T)
    p, _, _, status = rr.rule_schedule(homes, None, policy, fill, integral, T)
    ok = status == 0
    assert (ok & (homes["ev"] != 0)).sum() > N // 3
    return fr.report(p[None], homes[None], integral), homes, p, ok


@pytest.mark.parametrize("T", [24, 96])
def test_on_off_last_minute_to_target_has_nothing_to_cut(T):
    ref, homes, p, ok = _rule_case(T, rr.ALAP, rr.TARGET, 1)
    assert (ref.down[0][ok] == 0).all()
    assert (ref.row["n_down"][0][ok] == 0).all() and (ref.row["down_energy"][0][ok] == 0).all()
    assert (ref.up[0][ok] > 0).any()               # (the cars that wait could start earlier)


@pytest.mark.parametrize("T", [24, 96])
def test_on_off_uncontrolled_to_full_has_nothing_to_add(T):
    ref, homes, p, ok = _rule_case(T, rr.ASAP, rr.FULL, 1)
    assert (ref.up[0][ok] == 0).all()
    assert (ref.row["n_up"][0][ok] == 0).all() and (ref.row["up_energy"][0][ok] == 0).all()
    assert (ref.down[0][ok] > 0).any()


@pytest.mark.parametrize("T", [24, 96])
def test_continuous_anchors_within_the_float32_rounding_of_the_partial_slot(T):
    """The schedule's one partial slot is a float32: the energy delivered misses E_lo (E_hi) by at most half an ulp of it,
    below rating 2^-24; the bound is rating 2^-23."""
    for policy, fill, which in ((rr.ALAP, rr.TARGET, "down"), (rr.ASAP, rr.FULL, "up")):
        ref, homes, p, ok = _rule_case(T, policy, fill, 0)
        x = getattr(ref, which)[0]
        bound = homes["rating"].astype(np.float64) * 2.0 ** -23
        worst = (x / np.where(bound > 0, bound, 1.0)[:, None])[ok].max()
        print(f"T={T} {which}: worst / bound = {worst:.3f}")
        assert (x[ok] <= bound[ok, None]).all(), (which, worst)
        assert (getattr(ref, "down" if which == "up" else "up")[0][ok] > 1.0).any()


def _feasible_case(T, seed):
    """Continuous powers in [0, r], finite, over random records whose batteries are small and well charged: at T <= 8
    both the target and a full battery are within reach of many rows."""
    from revs_admm_amd.engine import pack_homes
    rng = np.random.default_rng(seed)
    start = rng.integers(-2, T + 1, 400)
    homes = pack_homes(np.ones(400, bool), rng.choice([1.2, 3.3, 4.8, 7.2, 11.5], 400), rng.uniform(5.0, 40.0, 400),
                       rng.uniform(0.5, 0.98, 400), start, start + rng.integers(0, T + 4, 400))
    r = homes["rating"].astype(np.float64)
    p = (rng.uniform(0, 1, (400, T)) * (rng.random((400, T)) < 0.6) * r[:, None] * rng.choice([0.1, 0.4, 1.0], 400)[:, None])
    p = np.minimum(p.astype(np.float32), homes["rating"][:, None])
    return p, homes


@pytest.mark.parametrize("T", [1, 3, 8])
def test_up_is_the_largest_raise_that_keeps_the_battery_within_full(T):
    """In a window slot the schedule itself has not overfilled (done(t) + p[t] <= E_hi): raising p[t] by up[t] and zeroing
    every later slot leaves the state of charge at or below 1 (within a rounding of the energies); 1 % of the rating more
    does not, unless up[t] is capped by r - p[t]."""
    p, homes = _feasible_case(T, 11 + T)
    ref = fr.report(p[None], homes[None], 0)
    r, c, i0 = (homes[k].astype(np.float64) for k in ("rating", "capacity", "initial"))
    ws, we = np.clip(homes["start"], 0, T), np.clip(homes["end"], 0, T)
    E_hi = (1.0 - i0) * c
    done = np.zeros(len(homes))
    cells = tight = 0
    for t in range(T):
        d = p[:, t].astype(np.float64)
        up = ref.up[0][:, t]
        inwin = (ws <= t) & (t < we)
        assert (up[~inwin] == 0).all()
        ok = inwin & (done + d <= E_hi) & (r > 0)
        eps = 2.0 ** -50 * (np.abs(E_hi) + done + d + r)
        assert (up[ok] >= 0).all() and (up[ok] <= (r - d)[ok] + eps[ok]).all()
        assert ((done + d + up)[ok] <= (E_hi + eps)[ok]).all(), t
        capped = up >= (r - d) - eps
        more = ok & ~capped
        assert ((done + d + up + 0.01 * r)[more] > E_hi[more]).all(), t
        cells += int(ok.sum())
        tight += int(more.sum())
        done = done + d
    assert cells > 50 and (tight > 0 or T == 1)


@pytest.mark.parametrize("T", [1, 3, 8])
def test_down_is_the_largest_cut_full_rate_charging_can_still_make_up(T):
    """In a window slot from which the target is still within reach (done(t) + p[t] + A(t) >= E_lo): cutting p[t] by
    down[t] and charging at the rating in every later window slot reaches E_lo (within a rounding of the energies); 1 % of
    the rating more does not, unless down[t] == p[t]."""
    p, homes = _feasible_case(T, 23 + T)
    ref = fr.report(p[None], homes[None], 0)
    r, c, i0 = (homes[k].astype(np.float64) for k in ("rating", "capacity", "initial"))
    ws, we = np.clip(homes["start"], 0, T), np.clip(homes["end"], 0, T)
    E_lo = (np.where(i0 > 0.9, i0, 0.9) - i0) * c
    done = np.zeros(len(homes))
    cells = tight = 0
    for t in range(T):
        d = p[:, t].astype(np.float64)
        down = ref.down[0][:, t]
        inwin = (ws <= t) & (t < we)
        assert (down[~inwin] == 0).all()
        A = np.maximum(we - np.maximum(t + 1, ws), 0) * r
        ok = inwin & (done + d + A >= E_lo)
        eps = 2.0 ** -50 * (np.abs(E_lo) + done + d + A)
        assert (down[ok] >= 0).all() and (down[ok] <= d[ok]).all()
        assert ((done + (d - down) + A)[ok] >= (E_lo - eps)[ok]).all(), t
        more = ok & (down < d)
        assert ((done + (d - down - 0.01 * r) + A)[more] < E_lo[more]).all(), t
        cells += int(ok.sum())
        tight += int(more.sum())
        done = done + d
    assert cells > 50 and tight > 0


@pytest.mark.parametrize("integral", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 24])
def test_awkward_rows_stay_finite_and_flags_match_their_definitions(T, integral):
    rng = np.random.default_rng(T)
    on_frac, tol = 0.25, 1e-3
    p, homes = cr.random_case(rng, 2, 200, T, on_frac, tol)
    ref = fr.report(p, homes, integral, on_frac, tol)
    ev = homes["ev"] != 0
    r = homes["rating"].astype(np.float64)
    for x in (ref.up, ref.down):
        assert np.isfinite(x).all() and (x >= 0).all() and (x <= r[:, :, None]).all()
        assert (x[~ev] == 0).all()
    if integral:
        assert np.isin(ref.up, (0.0,) + tuple(np.unique(r))).all() and ((ref.up == 0) | (ref.up == r[:, :, None])).all()
    ws, we = np.clip(homes["start"], 0, T).astype(np.int64), np.clip(homes["end"], 0, T).astype(np.int64)
    W = np.maximum(we - ws, 0)
    c, i0 = homes["capacity"].astype(np.float64), homes["initial"].astype(np.float64)
    tgt = np.maximum(i0, 0.9)
    pd = p.astype(np.float64)
    with np.errstate(all="ignore"):
        soc = i0[:, :, None] + np.concatenate([np.zeros((2, 200, 1)), np.cumsum(pd, axis=2)], axis=2) / c[:, :, None]
        short = tgt[:, :, None] - soc > tol
    never = short.all(2)
    ready = np.where(never, -1, np.argmin(short, axis=2))
    fin = np.isfinite(pd).all(2)                   # (cumsum and the loop's accumulator add in the same order)
    f = ref.row["flags"]
    assert (f[~ev] == 0).all() and (ref.row["ready"][~ev] == -1).all()
    assert ((f & 1) != 0)[ev].all()
    assert (((f & 4) != 0) == ~fin)[ev].all() and ((f & 4) != 0)[0].any()
    assert (ref.row["ready"][ev & fin] == ready[ev & fin]).all()
    assert (((f & 2) != 0) == (ref.row["ready"] < 0))[ev].all() and ((f & 2) != 0)[0].any()
    assert (((f & 8) != 0) == ((tgt - i0) * c > W * r))[ev].all() and ((f & 8) != 0).any()
    assert (((f & 16) != 0) == (ref.row["ready"] > we))[ev].all()
    assert (ref.row["slack"] == np.where(ev & (ref.row["ready"] >= 0), we - ref.row["ready"], 0)).all()
    assert (ref.keep == (ev & fin)).all()
    assert np.isnan(ref.val[:, ~(ev & fin)]).all() and np.isnan(ref.val[2][ev & fin & (ref.row["ready"] < 0)]).all()
    assert (ref.hist[:, 0].sum(1) == (ev & (ref.row["ready"] >= 0)).sum(1)).all()
    # the node sums are exact: any order of summation, any grouping, the same bits
    ptr = np.array([0, 0, 7, 7, 150, 200])
    a = fr.node_sums(ref.up, ptr)
    b = fr.q36(ref.up)[:, ::-1].cumsum(1)[:, ::-1]
    assert a[:, 0].tobytes() == np.zeros((2, T)).tobytes() and a[:, 1].tobytes() == (b[:, 0] - b[:, 7]).tobytes()
    assert a.sum(1).tobytes() == b[:, 0].tobytes()
