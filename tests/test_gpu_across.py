"""Statistics across scenarios on the GPU (revs_net_across; study.across_report_device, study_report(across=True),
AdmmEnsemble.study_report / voltages, REVS.study) against tests/across_ref.py: counts, violations, band counts, the
worst scenario, min, max, mean and the exposure exactly, the quartiles within 2 ulps (study_ref.check_pooled's bar for
the same np_lerp) -- at the smallest shapes at which the mapping can go wrong: cell counts that are no multiple of the
workgroup, scenario counts on both sides of a mask word, more groups than one launch's masks hold."""
import ctypes as C

import numpy as np
import pytest

import across_ref as ar
from test_gpu_network import golden_net  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SIZES = (0, 1, 2, 3, 4, 5, 8)            # every remainder of (count - 1) e mod 4, and the empty group
GUARD = 256


def make_groups(S, rng, straddle=None, singles=0):
    """Group ids: groups of SIZES members drawn at random (as far as S reaches), with `straddle` a pair of scenarios
    on both sides of a mask word in one group, `singles` further groups of one, then one large group of half the rest;
    the others are in no group."""
    gid = np.full(S, -1, np.int32)
    free = [int(s) for s in rng.permutation(S)]
    g = 0
    if straddle is not None:
        for s in straddle:
            gid[s] = g
            free.remove(s)
        g += 1
    for k in SIZES:
        if k > len(free):
            break
        for _ in range(k):
            gid[free.pop()] = g
        g += 1
    for _ in range(singles):
        gid[free.pop()] = g
        g += 1
    if len(free) >= 2:
        for _ in range(len(free) // 2):
            gid[free.pop()] = g
        g += 1
    return gid, g


def make_values(S, n, T, sense, rng):
    """Values on a 2^-10 grid (ties are common) with NaNs, a -0.0, negatives, an infinity and a cell of NaNs alone."""
    v = rng.normal(0.97, 0.04, (S, n, T)) if sense < 0 else rng.uniform(0.0, 1.4, (S, n, T))
    v = np.round(v * 1024) / 1024
    v[rng.random(v.shape) < 0.05] = NAN
    flat = v.reshape(-1)
    pick = rng.choice(flat.size, 8, replace=False)
    flat[pick[0]] = -0.0
    flat[pick[1]] = 0.0
    flat[pick[2:6]] = -0.25
    flat[pick[6]] = INF
    v[:, n // 2, 0] = NAN
    v[0, 0, 0] = -0.0                   # (beside whatever scenario 1 holds there)
    return v


def call(lib, values, keep, gid, G, lo, hi, sense, bands, slot=True, daily=True, expo=True):
    """revs_net_across itself on junk-filled outputs with guard bytes behind them -> (slot, daily, exposure) arrays."""
    import torch
    from revs_admm_amd._lib import ACROSS_DTYPE, check, ptr
    S, n, T = values.shape
    dev = "cuda:0"
    d_val = torch.from_numpy(values).to(dev)
    d_keep = None if keep is None else torch.from_numpy(keep.astype(np.uint8)).to(dev)
    size = {"slot": G * n * T * 96, "daily": G * n * 96, "expo": G * n * 4}
    want = {"slot": slot, "daily": daily, "expo": expo}
    buf = {k: torch.full((size[k] + GUARD,), 0xA5, dtype=torch.uint8, device=dev) if want[k] else None for k in size}
    nbytes = int(lib.revs_net_across_scratch(S, n))
    assert nbytes == 8 * S * n
    scratch = torch.full((nbytes // 8 + GUARD // 8,), -7.0, dtype=torch.float64, device=dev)
    hb = np.ascontiguousarray(bands, np.float64)
    hg = np.ascontiguousarray(gid, np.int32)
    check(lib.revs_net_across(S, n, T, ptr(d_val), ptr(d_keep), hg.ctypes.data, G, lo, hi, sense,
                              hb.ctypes.data if len(hb) else None, len(hb), ptr(buf["slot"]), ptr(buf["daily"]),
                              ptr(buf["expo"]), ptr(scratch), torch.cuda.current_stream().cuda_stream), "revs_net_across")
    torch.cuda.synchronize()
    out = {}
    for k, b in buf.items():
        if b is None:
            out[k] = None
            continue
        h = b.cpu().numpy()
        assert (h[size[k]:] == 0xA5).all(), f"{k}: bytes past the output were written"
        out[k] = h[:size[k]].copy()
    assert (scratch.cpu().numpy()[nbytes // 8:] == -7.0).all(), "bytes past the scratch were written"
    assert d_val.cpu().numpy().tobytes() == values.tobytes()                   # (the input is left alone)
    rec = lambda a, shape: None if a is None else a.view(ACROSS_DTYPE).reshape(shape)
    return (rec(out["slot"], (G, n, T)), rec(out["daily"], (G, n)),
            None if out["expo"] is None else out["expo"].view(np.int32).reshape(G, n))


CASES = [((5, 37, 5), None, 0), ((64, 3, 1), None, 0), ((65, 7, 3), (63, 64), 0), ((130, 9, 24), (127, 128), 0),
         ((192, 2, 2), (63, 64), 151)]


@pytest.mark.parametrize("sense", [-1, 1])
@pytest.mark.parametrize("shape, straddle, singles", CASES, ids=[str(c[0]) for c in CASES])
def test_kernel_against_the_yardstick(gpu_lib, shape, straddle, singles, sense):
    S, n, T = shape
    rng = np.random.default_rng(S * 1000 + n + (sense > 0))
    values = make_values(S, n, T, sense, rng)
    gid, G = make_groups(S, rng, straddle, singles)
    if S == 5:
        gid, G = np.array([2, 0, -1, 0, 2], np.int32), 4                       # sizes 2, 0, 2, 0
    if S == 192:
        assert G == 160                                                          # (one launch's masks hold 149 groups of 3 words)
    sizes = np.bincount(gid[gid >= 0], minlength=G)
    assert (gid == -1).any() and (S < 64 or set(SIZES) <= set(sizes.tolist()))
    keep = None
    if n > 2:
        keep = np.ones(n, bool)
        keep[[1, n - 1]] = False                                                 # holes
    lo, hi, bands = (0.95, 1.05, (0.92, 0.95, 0.98)) if sense < 0 else (-INF, 1.0, (0.8, 1.0))
    slot, daily, expo = call(gpu_lib, values, keep, gid, G, lo, hi, sense, bands)
    rslot, rdaily, rexpo = ar.across(values, keep, gid, G, lo, hi, sense, bands)
    ar.check_records(slot, rslot, "slot")
    ar.check_records(daily, rdaily, "daily")
    assert np.array_equal(expo, rexpo)
    # cells left out hold the empty record, whatever their values
    if keep is not None:
        assert slot[:, ~keep].tobytes() == ar.empty(slot[:, ~keep].shape).tobytes()
        assert daily[:, ~keep].tobytes() == ar.empty(daily[:, ~keep].shape).tobytes() and (expo[:, ~keep] == 0).all()
    assert (slot["band_count"][..., len(bands):] == 0).all()
    # the input is not trivial
    assert slot["n_nan"].max() > 0 and (slot["count"] == 0).any() and slot["n_violations"].max() > 0
    assert np.array_equal(expo, slot["n_violations"].sum(axis=2))
    # a group of one: the value itself in all six numbers, bit for bit (-0.0 is reported as +0.0), where it is finite
    seen = 0
    for g in np.flatnonzero(sizes == 1):
        s = int(np.flatnonzero(gid == g)[0])
        v = values[s] + 0.0
        ok = np.isfinite(v) & (np.ones(n, bool) if keep is None else keep)[:, None]
        seen += int(ok.sum())
        assert (slot["worst_scenario"][g][ok] == s).all()
        for k in ar.QS + ("mean",):
            assert slot[k][g][ok].tobytes() == v[ok].tobytes(), (g, k)
    assert seen > 0 or S == 5
    # the same bits from call to call; each output alone; the daily records without the slots'
    again = call(gpu_lib, values, keep, gid, G, lo, hi, sense, bands)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (slot, daily, expo)))
    only_daily = call(gpu_lib, values, keep, gid, G, lo, hi, sense, bands, slot=False, expo=False)
    assert only_daily[0] is None and only_daily[2] is None and only_daily[1].tobytes() == daily.tobytes()
    if T == 1:
        assert daily.tobytes() == slot[:, :, 0].tobytes()


def test_no_bands_no_keep_and_one_output(gpu_lib):
    rng = np.random.default_rng(77)
    values = make_values(9, 70, 4, -1, rng)                                      # 280 cells: a workgroup and a part
    gid = np.array([0, 0, 1, 0, -1, 1, 0, 0, 1], np.int32)
    slot, daily, expo = call(gpu_lib, values, None, gid, 2, 0.95, 1.05, -1, (), daily=False, expo=False)
    assert daily is None and expo is None and (slot["band_count"] == 0).all()
    ar.check_records(slot, ar.across_cells(values, None, gid, 2, 0.95, 1.05, -1, ()), "slot")
    _, _, expo = call(gpu_lib, values, None, gid, 2, 0.95, 1.05, -1, (), slot=False, daily=False)
    assert np.array_equal(expo, slot["n_violations"].sum(axis=2))


def test_golden_across_agrees_with_the_pooled_records(gpu_lib, golden, golden_net):
    """The five stored 121144 results over community 2 in two groups: summed or reduced over the nodes, the records
    across scenarios are the existing kernels' pooled records and band counts; and the whole report is the
    yard-stick's on the kernel's own arrays."""
    from test_gpu_study import BANDS, TAGS
    from revs_admm_amd.study import across_report_device, study_report
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    nodes = np.array([gn["nonsub"].index(h) for h in com])
    p = np.stack([z[t + "_P_res"] for t in TAGS])
    groups = np.array([1, 0, 0, 0, 1])
    rep = study_report(par, er, cons, p, groups=groups, rating=gn["rating"], nodes=nodes, bands=BANDS, vset=1.0,
                       arrays=True, across=True)
    acr = rep.across
    assert acr.slot_volt.shape == (2, gn["n"], 24) and acr.group_sizes.tolist() == [3, 2]
    rated = np.asarray(gn["rating"]) > 0
    with np.errstate(invalid="ignore"):
        for kind, slot, pooled, kept in (("volt", acr.slot_volt, rep.pooled_volt, nodes),
                                         ("loading", acr.slot_loading, rep.pooled_loading, np.flatnonzero(rated))):
            assert np.array_equal(slot["count"].sum(axis=1), pooled["count"]), kind
            assert np.array_equal(slot["n_violations"].sum(axis=1), pooled["n_violations"]), kind
            assert np.array_equal(slot["n_nan"].sum(axis=1), pooled["n_nan"]), kind
            assert np.array_equal(slot["min"][:, kept].min(axis=1), pooled["min"]), kind
            assert np.array_equal(slot["max"][:, kept].max(axis=1), pooled["max"]), kind
    assert (rep.pooled_volt["count"] == np.array([3, 2])[:, None] * 297).all() and rep.pooled_loading["count"].min() > 0
    for g in range(2):
        assert np.array_equal(acr.slot_volt["band_count"][g][..., :3].sum(axis=0), rep.band_counts[groups == g].sum(axis=0))
    assert acr.slot_volt["n_violations"].max() > 0 and acr.daily_volt["band_count"][0, :, 0].max() > 0      # (not trivial)
    ar.check_report(acr, rep.volt, rep.loading, groups, nodes, gn["rating"], BANDS, (0.8, 1.0), 0.95, 1.05)
    # without the arrays read back, and from the arrays uploaded again: the same report
    lean = study_report(par, er, cons, p, groups=groups, rating=gn["rating"], nodes=nodes, bands=BANDS, vset=1.0, across=True)
    assert lean.volt is None and ar.same_across(lean.across, acr)
    import torch
    direct = across_report_device(torch.from_numpy(rep.volt).cuda(), torch.from_numpy(rep.loading).cuda(), groups,
                                  nodes=nodes, rated=gn["rating"], bands=BANDS)
    assert ar.same_across(direct, acr)
    no_slots = across_report_device(torch.from_numpy(rep.volt).cuda(), None, groups, nodes=nodes, bands=BANDS, slots=False)
    assert no_slots.slot_volt is None and no_slots.daily_volt.tobytes() == acr.daily_volt.tobytes()
    assert no_slots.exposure_volt.tobytes() == acr.exposure_volt.tobytes()
    # the question the report answers: the node of community 2 most often below 0.95 at some hour among the three
    # individual optima, and its median daily minimum
    prob = acr.probability("volt", 1)[0]
    worst = int(np.nanargmax(prob))
    print(f"node {worst}: below 0.95 at some hour in {acr.daily_volt['band_count'][0, worst, 1]} of 3 results, median "
          f"daily minimum {acr.daily_volt['median'][0, worst]:.4f}, {acr.expected_slots('volt')[0, worst]:.1f} slots per result")
    assert worst in nodes.tolist() and prob[worst] == 1.0


def test_ensemble_across_and_voltages(gpu_lib):
    """A synthetic ensemble (600 residences on 60 nodes, S = 6, T = 24): study_report(across=True) is
    across_report_device on the arrays study_report(arrays=True) gives, voltages() the stacked volt of
    network_reports(), and the run's state is left alone."""
    import torch
    from network_worker import line_ratings
    from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
    from revs_admm_amd import study
    w = _workload()
    e = _ensemble(w, _mixed_scenarios(w, 6), "relaxed_exact")
    e.run(2)
    rating, nodes = line_ratings(w)
    groups = [0, 1, 0, 1, -1, 0]
    state = [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)]
    rep = e.study_report(groups=groups, rating=rating, nodes=nodes, arrays=True, across=True)
    ref = study.across_report_device(torch.from_numpy(rep.volt).cuda(), torch.from_numpy(rep.loading).cuda(), groups,
                                     nodes=nodes, rated=rating, bands=rep.bands, vmin=e.vlow, vmax=e.vhigh)
    assert ar.same_across(rep.across, ref) and rep.across.group_sizes.tolist() == [3, 2]
    ar.check_report(rep.across, rep.volt, rep.loading, groups, nodes, rating, rep.bands, (0.8, 1.0), e.vlow, e.vhigh)
    lean = e.study_report(groups=groups, rating=rating, nodes=nodes, across=True)
    assert lean.volt is None and ar.same_across(lean.across, ref)
    assert e.study_report(groups=groups, rating=rating, nodes=nodes).across is None
    # voltages(): every scenario's network_report().volt, on the device
    volt = e.voltages()
    reports = e.network_reports(rating=rating, nodes=nodes)
    assert volt.is_cuda and volt.dtype == torch.float64 and tuple(volt.shape) == (6, len(w.feeder[0]), 24)
    assert volt.cpu().numpy().tobytes() == np.stack([r.volt for r in reports]).tobytes()
    some = e.voltages(nodes=nodes)
    assert some.cpu().numpy().tobytes() == np.stack([r.volt[np.asarray(nodes)] for r in reports]).tobytes()
    out = torch.zeros_like(volt)
    assert e.voltages(out=out).data_ptr() == out.data_ptr() and torch.equal(out, volt)
    with pytest.raises(ValueError, match="out must be"):
        e.voltages(out=torch.zeros(6, 3, 24, dtype=torch.float64, device=volt.device))
    for a, b in zip(state, (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_revs_study_across_on_both_paths(gpu_lib):
    """REVS.study(ensemble=True, across=True) on a small feeder: with device_report=True the report across scenarios is
    the host-upload path's on the same node sums, bit for bit, and on the host-upload path it is there too."""
    from test_gpu_ensemble_report import _small_graph
    from revs_admm_amd import study
    from revs_admm_amd.drawing import line_nodes
    from revs_admm_amd.lpsolver import feeder_of
    from revs_admm_amd.revs_fixture import REVS
    g = _small_graph()
    for k, e in enumerate(g.edges):
        g.edges[e]["rating"] = 0.0 if k % 7 == 3 else 30.0 + 5.0 * (k % 4)      # kVA; some lines unrated
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    rng = np.random.default_rng(4)
    T = 24
    all_homes = {h: rng.uniform(0.2, 1.5, T).astype(np.float32).astype(np.float64).tolist() for h in res}
    tariff = (0.1 + 0.05 * np.sin(np.arange(T) / T * 2 * np.pi)).astype(np.float32).astype(np.float64).tolist()
    com = res[5:35]
    grid = dict(adoptions=(50,), ratings=(4800,), seeds=(1, 2, 3), methods=("distributed",), group_by="adoption",
                max_iterations=2, mode="relaxed", arrays=True)
    fx = REVS()
    lab0, rep0 = fx.study(tariff, all_homes, g, com, ensemble=True, across=True, **grid)
    lab1, rep1 = fx.study(tariff, all_homes, g, com, ensemble=True, device_report=True, across=True, **grid)
    assert lab0 == lab1 and rep0.across is not None and rep1.across is not None
    nonsub = [n for n in g if g.nodes[n]["label"] != "S"]
    par, er, cons = feeder_of(g)[1]
    node_rating = line_nodes(g, None, par, nonsub)[0]
    nodes = [nonsub.index(h) for h in com]
    for rep in (rep0, rep1):
        ref = study.study_report(par, er, cons, rep.node_p, groups=rep.groups, rating=node_rating, nodes=nodes,
                                 arrays=True, across=True)
        assert ref.volt.tobytes() == rep.volt.tobytes() and ar.same_across(rep.across, ref.across)
        assert rep.across.group_sizes.tolist() == [3] and (rep.across.daily_volt["count"][0, nodes] == 3).all()
        assert rep.across.daily_loading["count"].sum() == 3 * int((node_rating > 0).sum())
    ar.check_report(rep1.across, rep1.volt, rep1.loading, rep1.groups, nodes, node_rating, (0.92, 0.95, 0.98), (0.8, 1.0),
                    0.95, 1.05)
