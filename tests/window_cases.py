"""A deterministic atlas of residences per horizon: the charging windows and energy needs at which a kernel that spreads a
residence's slots over lanes is most likely to be wrong, and which revs_admm_amd.synthetic.make_workload never draws
(its windows start at {10..13} T // 24, end at {21..24} T // 24 and need between one slot and all but one).

A lane shape is (lpa lanes per residence) x (spl slots per lane): lane k owns the slots [k spl, (k + 1) spl), the lanes
from ceil(T / spl) on are dead and the last live lane is ragged where spl does not divide T.

Window categories (tags of the same names):
  one_slot      [t, t + 1) for t = k spl - 1 and t = k spl at every lane boundary, t = 0 and t = T - 1
  lane          exactly one lane, [k spl, (k + 1) spl): the first, a middle and the last live lane
  lane_shifted  the same three windows moved by one slot
  inside_lane   strictly inside one of these lanes (spl >= 3)
  horizon       [0, T)
  outside       [-3, T + 5), [-3, 2) and [T - 2, T + 5): windows that reach outside the horizon (over the dead lanes)
  ragged_lane   the live slots of the last live lane, [(L - 1) spl, T)
For T <= 16 every pair 0 <= start < end <= T takes the place of the first five lists, each pair tagged with every category
whose description it meets.

Need classes, through `initial` and `capacity` as revs_admm_amd.engine.pack_homes turns them into slot counts (W: the
window's slots inside the horizon; one slot moves the state of charge by per = rating / capacity = 0.75 / (W + 1)):
  nmin0         initial = 0.95: charged past 90 %, no slot needed
  nmin1         0.9 - initial = 0.75 per
  nmin_half     0.9 - initial = (max(1, W // 2) - 0.25) per
  nmin_W        0.9 - initial = W per, rounded towards the feasible side: every slot of the window at full rating
  nmin_W1       0.9 - initial = (W + 0.75) per: one slot more than the window has -- "No solution found"
  nmax_lt_nmin  per = 0.3, initial = 0.5: 1.33 slots to 90 %, 1.67 to 100 %, so nmin = 2 > nmax = 1.  The on/off problem
                has no solution; the continuous one has (any W >= 2 holds 1.33 slots' energy)
The chargers are 3.6 / 7.2 kW up to W = 48 and 0.9 / 1.8 kW beyond: a float kernel forms the energy to 90 % from 0.9f,
2.4e-8 off 0.9, times a capacity of 1.33 (W + 1) rating, and on an nmin_W residence all of that error lands in one slot
-- 1.3e-4 kW at W = 192 x 7.2 kW, which is the inputs' rounding and no kernel's; at 1.8 kW it is 3e-5.

Every 7th record (0, 7, 14, ...) has no EV (tag no_ev); these are inserted between the others, so every (category, need
class) pair keeps its EV record.  Where windows x classes exceeds `limit` records, a category of m windows gets
max(m, 6) records: window r % m with class (r + r // 6) % 6 (the classes in turn, moved on
by one after every six windows, so that no class keeps to one side of the lane boundaries).  Horizons up to 16 always
take the full cross product.

Load: uniform in (0.2, 5) kW; cost: five tariff levels in (0.05, 0.3), so that slots tie -- as
tests/test_gpu_agent.py::test_edge_parameters.  Everything is float32-representable."""
from collections import namedtuple

import numpy as np

CATEGORIES = ("one_slot", "lane", "lane_shifted", "inside_lane", "horizon", "outside", "ragged_lane")
NEEDS = ("nmin0", "nmin1", "nmin_half", "nmin_W", "nmin_W1", "nmax_lt_nmin")
INFEASIBLE = ("nmin_W1", "nmax_lt_nmin")
# lanes per residence x slots per lane of every shape (revs_admm_amd/csrc/agent_kernels.hip: pick_shape)
SHAPES = {"8x1": (8, 1), "8x2": (8, 2), "8x3": (8, 3), "8x4": (8, 4), "16x3": (16, 3), "16x4": (16, 4), "16x6": (16, 6),
          "32x4": (32, 4), "64x3": (64, 3)}

Atlas = namedtuple("Atlas", "homes load cost tags")


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def live_lanes(T, spl):
    return -(-T // spl)


def boundaries(T, spl):
    """The first slot of every live lane but lane 0."""
    return [k * spl for k in range(1, live_lanes(T, spl))]


def clipped(start, end, T):
    return min(end, T) - max(start, 0)


def _three_lanes(T, spl):
    L = live_lanes(T, spl)
    return sorted({0, L // 2, L - 1})


def _categories_of(s, e, T, spl):
    """Every category whose description the window [s, e) meets."""
    L = live_lanes(T, spl)
    k = max(s, 0) // spl
    lane_end = min((k + 1) * spl, T)
    out = set()
    if s < 0 or e > T:
        out.add("outside")
        return out
    if e - s == 1 and (s % spl == 0 or (s + 1) % spl == 0 or s == T - 1):
        out.add("one_slot")
    if s == k * spl and e == lane_end:
        out.add("lane")
    if s >= 1 and (s - 1) % spl == 0 and e == min(s + spl, T):
        out.add("lane_shifted")
    if spl >= 3 and s > k * spl and e < lane_end:
        out.add("inside_lane")
    if s == 0 and e == T:
        out.add("horizon")
    if s == (L - 1) * spl and e == T:
        out.add("ragged_lane")
    return out


def windows(T, spl):
    """-> list of (start, end, set of categories), every window with at least one slot inside the horizon."""
    L = live_lanes(T, spl)
    out = []
    if T <= 16:
        for s in range(T):
            for e in range(s + 1, T + 1):
                out.append((s, e, _categories_of(s, e, T, spl)))
    else:
        ts = sorted({0, T - 1} | {b - 1 for b in boundaries(T, spl)} | set(boundaries(T, spl)))
        out += [(t, t + 1, {"one_slot"}) for t in ts]
        out += [(k * spl, (k + 1) * spl, {"lane"}) for k in _three_lanes(T, spl)]
        out += [(k * spl + 1, (k + 1) * spl + 1, {"lane_shifted"}) for k in _three_lanes(T, spl)]
        if spl >= 3:
            out += [(k * spl + 1, (k + 1) * spl - 1, {"inside_lane"}) for k in _three_lanes(T, spl)
                    if (k + 1) * spl - 1 < min((k + 1) * spl, T)]
        out.append((0, T, {"horizon"}))
    out += [(-3, T + 5, {"outside"}), (-3, 2, {"outside"}), (T - 2, T + 5, {"outside"})]
    out.append(((L - 1) * spl, T, {"ragged_lane"}))
    return [w for w in out if clipped(w[0], w[1], T) >= 1]


def _need(cls, W, rating):
    """-> (capacity, initial) of need class `cls` on a window of W slots, float32-representable."""
    if cls == "nmax_lt_nmin":
        return float(_f32(rating / 0.3)), float(_f32(0.5))
    cap = float(_f32(rating * (W + 1) / 0.75))
    per = rating / cap
    if cls == "nmin0":
        return cap, float(_f32(0.95))
    x = {"nmin1": 0.75, "nmin_half": max(1, W // 2) - 0.25, "nmin_W": float(W), "nmin_W1": W + 0.75}[cls]
    ini = np.float32(0.9 - x * per)
    if cls == "nmin_W":            # the smallest float at which W slots still reach 90 % (pack_homes allows 1e-9 slot)
        while (0.9 - float(ini)) / per > W:
            ini = np.nextafter(ini, np.float32(1.0))
    return cap, float(ini)


def atlas(T, lpa, spl, seed, feasible_only=False, limit=800):
    """-> Atlas(homes, load, cost, tags).  homes: pack_homes records; load (n, T), cost (T,): float64 holding float32
    values; tags: category / need class / "no_ev" / "feasible" / "infeasible" -> indices of the residences (sorted).
    feasible_only: without the need classes nmin_W1 and nmax_lt_nmin (the closed loop's variant: the reference stops
    at "No solution found")."""
    from revs_admm_amd.engine import pack_homes
    assert lpa * spl >= T >= 1, (T, lpa, spl)
    needs = [c for c in NEEDS if not (feasible_only and c in INFEASIBLE)]
    wins = windows(T, spl)
    recs = []                                   # (start, end, categories, need class)
    if T <= 16 or len(wins) * len(needs) <= limit:
        recs = [(s, e, cats, c) for s, e, cats in wins for c in needs]
    else:
        for cat in CATEGORIES:
            mine = [w for w in wins if cat in w[2]]
            for r in range(max(len(mine), len(needs)) if mine else 0):
                s, e, _ = mine[r % len(mine)]
                recs.append((s, e, {cat}, needs[(r + r // len(needs)) % len(needs)]))
    # a residence without EV in front of every six with one
    rows = []
    for i, rec in enumerate(recs):
        if i % 6 == 0:
            rows.append(rec[:3] + (None,))
        rows.append(rec)
    n = len(rows)
    ev = np.array([r[3] is not None for r in rows])
    assert not ev[::7].any() and ev.sum() == len(recs)
    start = np.array([r[0] for r in rows])
    end = np.array([r[1] for r in rows])
    rating, cap, ini = np.zeros(n), np.zeros(n), np.zeros(n)
    tags = {k: [] for k in CATEGORIES + NEEDS + ("no_ev", "feasible", "infeasible")}
    for i, (s, e, cats, cls) in enumerate(rows):
        W = clipped(s, e, T)
        rating[i] = float(_f32((3.6 if W <= 48 else 0.9) * (1 + i % 2)))
        cap[i], ini[i] = _need(cls or "nmin1", W, rating[i])
        if cls is None:
            tags["no_ev"].append(i)
        else:
            tags[cls].append(i)
            for c in cats:
                tags[c].append(i)
        tags["infeasible" if cls in INFEASIBLE else "feasible"].append(i)
    homes = pack_homes(ev, rating, cap, ini, start, end)
    rng = np.random.default_rng(seed)
    load = _f32(rng.uniform(0.2, 5, (n, T)))
    cost = _f32(rng.uniform(0.05, 0.3, 5)[rng.integers(0, 5, T)])
    return Atlas(homes, load, cost, {k: np.array(v, np.int64) for k, v in tags.items()})


def atlas_of(T, seed=None, **kw):
    """atlas() at the lane shape pick_shape gives horizon T."""
    from test_gpu_shapes import shape_of
    lpa, spl = SHAPES[shape_of(T)]
    return atlas(T, lpa, spl, T if seed is None else seed, **kw)


def reordered(a, perm):
    """The atlas with residence perm[i] at place i."""
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return Atlas(a.homes[perm], a.load[perm], a.cost, {k: np.sort(inv[v]) for k, v in a.tags.items()})


def workload(a, kappa=5.0):
    """The atlas as a Workload without a feeder (one node), for the launches that take none."""
    from revs_admm_amd.synthetic import Workload
    n = len(a.homes)
    return Workload(a.cost, a.load, a.homes, np.zeros(n, np.int64), np.eye(1), None, None, 1.0, 0.95, 1.05, kappa)


def describe(a, i):
    """Where residence i sits in the atlas: its tags, window and slot counts (for a failure's message)."""
    h = a.homes[i]
    names = [k for k, v in a.tags.items() if k not in ("feasible", "infeasible") and i in v]
    return (f"residence {i} [{' '.join(names)}] window [{h['start']}, {h['end']}) nmin {h['nmin']} nmax {h['nmax']} "
            f"rating {h['rating']:.1f}")
