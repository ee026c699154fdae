"""The charging report on the GPU (csrc/charge_kernels.hip, revs_admm_amd/charging.py): every
output of revs_charge_report, through the C ABI and through the Python entries, against the numpy yard-stick
(tests/charge_ref.py) at the smallest shapes at which the mapping can go wrong -- one row, one short of and one more than
a workgroup's 256 rows, three workgroups, a slot count below, at and above the chunk, both load widths -- and end to end
from the state an engine and an ensemble hold."""
import numpy as np
import pytest

import bills_ref as br
import charge_ref as cr

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = F32(7e9)            # fills every gap of a padded layout: no record may see it
GUARD = 64                     # bytes of canary on either side of every output and of the scratch
OUTPUTS = ("row", "slot", "day", "hist", "val", "keep")
CHUNK = 32                     # revs_charge_report_chunk(): checked below


def native(lib, p, homes, tariff=None, on_frac=0.0, short_tol=1e-6, pad=0, off=0, layout="nst", want=OUTPUTS):
    """p (S, n, T) float32 and homes (S, n) on the host -> dict of what revs_charge_report wrote, through the C ABI.
    layout "nst": float[n][S][T + pad] (an ensemble's); "snt": float[S][n][T + pad] (a study's).  off: floats between a
    256-byte boundary and element 0.  Every gap holds SENTINEL; outputs and scratch sit between canaries; the inputs are
    compared before and after."""
    import torch
    from revs_admm_amd._lib import CHARGE_DAY_DTYPE, CHARGE_ROW_DTYPE, CHARGE_SLOT_DTYPE, check, ptr
    S, n, T = p.shape
    W = T + pad
    dev = torch.device("cuda:0")
    wide = np.full((n, S, W) if layout == "nst" else (S, n, W), SENTINEL, F32)
    if layout == "nst":
        wide[:, :, :T] = p.transpose(1, 0, 2)
        stride_s, stride_i = W, S * W
    else:
        wide[:, :, :T] = p
        stride_s, stride_i = n * W, W
    flat = np.concatenate([np.full(off, SENTINEL, F32), wide.reshape(-1), np.full(8, SENTINEL, F32)])
    d_all = torch.from_numpy(flat).to(dev)
    assert d_all.data_ptr() % 256 == 0
    d_p = d_all[off:]
    rec = np.ascontiguousarray(homes.T).view(np.uint8).reshape(-1)                 # records [n][S]
    d_homes = torch.from_numpy(rec).to(dev)
    d_tariff = None if tariff is None else torch.from_numpy(np.ascontiguousarray(tariff, np.float64)).to(dev)
    sizes = dict(row=S * n * 64, slot=S * T * 32, day=S * 64, hist=S * 3 * (T + 1) * 4, val=4 * S * n * 8, keep=S * n)
    nbytes = int(lib.revs_charge_report_scratch(S, n, T))
    assert nbytes > 0 and nbytes % 16 == 0
    sizes["scratch"] = nbytes
    guarded = lambda nb: torch.full((GUARD + nb + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    bufs = {k: guarded(sizes[k]) for k in sizes if k == "scratch" or k in want}
    q = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else None
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib.revs_charge_report(S, n, T, ptr(d_p), stride_s, stride_i, ptr(d_homes), ptr(d_tariff), float(on_frac),
                                 float(short_tol), q("row"), q("slot"), q("day"), q("hist"), q("val"), q("keep"),
                                 q("scratch"), st), "revs_charge_report")
    torch.cuda.synchronize()
    assert d_all.cpu().numpy().tobytes() == flat.tobytes() and d_homes.cpu().numpy().tobytes() == rec.tobytes()
    kinds = dict(row=(CHARGE_ROW_DTYPE, (S, n)), slot=(CHARGE_SLOT_DTYPE, (S, T)), day=(CHARGE_DAY_DTYPE, (S,)),
                 hist=(np.int32, (S, 3, T + 1)), val=(np.float64, (4, S, n)), keep=(np.uint8, (S, n)))
    out = {k: None for k in OUTPUTS}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xCD).all() and (h[GUARD + sizes[k]:] == 0xCD).all(), ("canary", k)
        if k != "scratch":
            out[k] = h[GUARD:GUARD + sizes[k]].copy().view(kinds[k][0]).reshape(kinds[k][1])
    return out


def layouts(T):
    """The ensemble's layout as it stands (16-byte loads where T is a multiple of 4); the study's, padded and off a
    16-byte boundary (4-byte loads); a view into a wider buffer whose strides are multiples of 4 (16-byte loads with a
    ragged end where T is none)."""
    return ((0, 0, "nst"), (3, 1, "snt"), ((-T) % 4 + 4, 4, "nst"))


# every n, S and T of the list, not their product; (600, 3) is three workgroups a scenario
SHAPES = [(1, 1, 1), (1, 3, 24), (255, 1, 5), (255, 3, CHUNK), (257, 1, 96), (257, 3, CHUNK - 1), (600, 1, CHUNK + 1),
          (600, 3, 24), (600, 1, 192), (257, 3, 1), (255, 1, 2 * CHUNK), (257, 1, 2 * CHUNK + 1)]


def test_the_shapes_cover_every_value(gpu_lib):
    assert int(gpu_lib.revs_charge_report_chunk()) == CHUNK
    assert {s[0] for s in SHAPES} == {1, 255, 257, 600} and {s[1] for s in SHAPES} == {1, 3}
    assert {s[2] for s in SHAPES} >= {1, 5, 24, 96, 192, CHUNK - 1, CHUNK, CHUNK + 1}


@pytest.mark.parametrize("n,S,T", SHAPES)
def test_outputs_at_every_shape(gpu_lib, n, S, T):
    rng = np.random.default_rng(1000 * n + 10 * T + S)
    on_frac, tol = (0.0, 1e-6) if (n + T) % 2 else (0.25, 1e-3)
    p, homes = cr.random_case(rng, S, n, T, on_frac, tol)
    tariff = rng.uniform(0.05, 0.4, T)
    ref = cr.report(p, homes, tariff, on_frac, tol)
    if n >= len(cr.AWKWARD):                       # every awkward row is there, and some rows are not kept
        assert (ref.row["flags"][0] & 4).any() and (ref.row["flags"][0] & 2).any() and not ref.keep[0].all()
    if S > 1:
        assert ref.day["n_ev"][1] == 0 and ref.day["n_ev"][0] > 0
    for pad, off, layout in layouts(T):
        out = native(gpu_lib, p, homes, tariff, on_frac, tol, pad, off, layout)
        cr.check(ref, **out, what=(n, S, T, pad, off, layout))


def test_without_a_tariff_every_cost_is_a_nan(gpu_lib):
    rng = np.random.default_rng(5)
    p, homes = cr.random_case(rng, 3, 300, 24)
    ref = cr.report(p, homes, None)
    out = native(gpu_lib, p, homes, None)
    cr.check(ref, **out, what="no tariff")
    ev = homes["ev"] != 0
    assert np.isnan(out["row"]["cost"][ev]).all() and (out["row"]["cost"][~ev] == 0).all()
    assert np.isnan(out["val"][1]).all() and np.isnan(out["day"]["cost"][[0, 2]]).all() and out["day"]["cost"][1] == 0


def test_each_output_alone_and_two_calls_give_the_same_bytes(gpu_lib):
    rng = np.random.default_rng(7)
    S, n, T = 3, 600, 33
    p, homes = cr.random_case(rng, S, n, T)
    tariff = rng.uniform(0.05, 0.4, T)
    full = native(gpu_lib, p, homes, tariff)
    again = native(gpu_lib, p, homes, tariff)
    for k in OUTPUTS:
        assert full[k].tobytes() == again[k].tobytes(), k
    for k in OUTPUTS:
        part = native(gpu_lib, p, homes, tariff, want=(k,))
        assert all((part[j] is None) == (j != k) for j in OUTPUTS)
        assert part[k].tobytes() == full[k].tobytes(), k
    # the other layout sums the same rows in the same order: the same bytes again
    other = native(gpu_lib, p, homes, tariff, pad=3, off=1, layout="snt")
    for k in OUTPUTS:
        assert other[k].tobytes() == full[k].tobytes(), k


def test_box_records_over_val_out(gpu_lib):
    """revs_bill_study (base = -1) over val_out under keep_out: bills_ref's record of the yard-stick's values, per
    scenario and pooled; through the Python entry, which also pools the integer records on the host."""
    from revs_admm_amd import charging as ch
    rng = np.random.default_rng(9)
    S, n, T = 3, 300, 24
    p, homes = cr.random_case(rng, S, n, T)
    homes["ev"][1] = rng.random(n) < 0.5           # (three scenarios with EVs: a pool of two and one alone)
    tariff = rng.uniform(0.05, 0.4, T)
    groups = [0, -1, 0]
    ref = cr.report(p, homes, tariff)
    rep = ch.charging_report(p, homes, tariff, groups=groups)
    cr.check(ref, rep.row, rep.slot, rep.day, rep.hist, what="python entry")
    assert rep.n_groups == 1 and rep.groups.tolist() == groups
    for q, name in enumerate(ch.QUANTITIES):
        for s in range(S):
            br.check_record(getattr(rep, name)[s], br.record(ref.val[q], ref.keep, [s]), (name, s))
        br.check_record(getattr(rep, "pooled_" + name)[0], br.record(ref.val[q], ref.keep, [0, 2]), (name, "pool"))
    # a charger that is never on is kept and has no wait: it counts in n_nan there
    never = ((ref.row["n_on"] == 0) & (ref.keep != 0)).sum(1)
    assert never.any() and (rep.wait["n_nan"] == never).all() and (rep.energy["n_nan"] == 0).all()
    for k in ("n_ev", "n_plugged", "n_on", "n_full", "n_starts"):
        assert (rep.pooled_slot[k][0] == ref.slot[k][0] + ref.slot[k][2]).all(), k
    assert (rep.pooled_hist[0] == ref.hist[0] + ref.hist[2]).all()
    assert rep.on_curve().tolist() == ref.slot["n_on"].tolist()
    d = rep.compare(rep)
    assert all(((d[k] == 0) | np.isnan(d[k])).all() for k in d)       # (scenario 0 holds rows of NaN and inf)
    assert (d["peak_on"] == 0).all()
    # rows=False / "device": the same records, the rows not read back
    lean = ch.charging_report(p, homes, tariff, groups=groups, rows=False)
    assert lean.row is None and lean.row_device is None and lean.slot.tobytes() == rep.slot.tobytes()
    assert lean.energy.tobytes() == rep.energy.tobytes() and lean.day.tobytes() == rep.day.tobytes()
    kept = ch.charging_report(p, homes, tariff, groups=groups, rows="device")
    assert kept.row is None and kept.row_device.is_cuda and kept.row_device.cpu().numpy().tobytes() == rep.row.tobytes()


def _same_but_sums(rep, free, what):
    """A method's report against the free function's on result()'s S in the caller's order: rows, counts, histograms and
    box records bit for bit; the sums over the rows of a scenario (another order) within their bound."""
    assert rep.row.tobytes() == free.row.tobytes(), what
    assert rep.hist.tobytes() == free.hist.tobytes() and rep.pooled_hist.tobytes() == free.pooled_hist.tobytes(), what
    assert rep.pooled_slot.tobytes() == free.pooled_slot.tobytes(), what
    for k in cr.SLOT_INT:
        assert rep.slot[k].tobytes() == free.slot[k].tobytes(), (what, k)
    for k in cr.DAY_INT[:2] + cr.DAY_INT[3:] + ("coincidence",):
        assert rep.day[k].tobytes() == free.day[k].tobytes(), (what, k)
    for name in ("energy", "cost", "soc_end", "wait"):
        assert getattr(rep, name).tobytes() == getattr(free, name).tobytes(), (what, name)
        assert getattr(rep, "pooled_" + name).tobytes() == getattr(free, "pooled_" + name).tobytes(), (what, name)


def test_engine_end_to_end(gpu_lib):
    from test_gpu_conv import _single
    import rules_ref as rr
    from revs_admm_amd import charging as ch
    w, make = _single()
    e, f = make(), make()
    for x in (e, f):
        x.run_steps(2)
    with pytest.raises(RuntimeError, match="did not write the charger power"):
        e.charging_report()
    for x in (e, f):
        x.step()
    power = e.result()[1]
    tariff = w.cost.astype(np.float64)
    rep = e.charging_report()
    free = ch.charging_report(power, w.homes, tariff)
    assert rep.row.shape == (1, 300) and rep.slot.shape == (1, 24) and rep.hist.shape == (1, 3, 25)
    _same_but_sums(rep, free, "engine")
    cr.check(cr.report(power[None], w.homes[None], tariff), rep.row, rep.slot, rep.day, rep.hist, what="engine")
    assert int(rep.day["n_ev"][0]) == int((w.homes["ev"] != 0).sum()) > 0 and rep.day["peak_on"][0] > 0
    # a policy name: the p of the rule schedule, as rules_ref gives it
    pol = e.charging_report("uncontrolled", tariff=None)
    p_ref = rr.rule_schedule(w.homes, w.load, rr.ASAP, rr.TARGET, 0)[0]
    cr.check(cr.report(p_ref[None], w.homes[None], None), pol.row, pol.slot, pol.day, pol.hist, what="uncontrolled")
    assert np.isnan(pol.day["cost"][0]) and (pol.row["wait"][pol.row["n_on"] > 0] == 0).all()
    # a tensor in the engine's order
    t = e.charging_report(e.S.clone(), tariff=tariff)
    assert t.row.tobytes() == rep.row.tobytes() and t.day.tobytes() == rep.day.tobytes()
    with pytest.raises(ValueError, match="profile must be"):
        e.charging_report("cheapest")
    with pytest.raises(ValueError, match="power tensor must be"):
        e.charging_report(e.S[:10])
    # the state is as it was: the run goes on bit for bit as one that was never asked
    e.step()
    f.step()
    for x, y in zip(e.get_state(), f.get_state()):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(e.result(), f.result()):
        assert x.tobytes() == y.tobytes()


def test_ensemble_end_to_end(gpu_lib):
    from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
    import rules_ref as rr
    from revs_admm_amd import charging as ch
    w = _workload(n=300, n_nodes=30)
    homes = _mixed_scenarios(w, 3)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for x in (a, b):
        x.run_steps(2)
    with pytest.raises(RuntimeError, match="did not write the charger power"):
        b.charging_report()
    for x in (a, b):
        x.step()
    rec = np.stack(homes)
    power = b.result()[1]
    tariff = w.cost.astype(np.float64)
    groups = [0, -1, 0]
    rep = b.charging_report(groups=groups, on_frac=0.05)
    free = ch.charging_report(power, rec, tariff, groups=groups, on_frac=0.05)
    assert rep.row.shape == (3, 300) and rep.slot.shape == (3, 24) and rep.pooled_slot.shape == (1, 24)
    _same_but_sums(rep, free, "ensemble")
    cr.check(cr.report(power, rec, tariff, 0.05), rep.row, rep.slot, rep.day, rep.hist, what="ensemble")
    assert (rep.day["n_ev"] == (rec["ev"] != 0).sum(1)).all()
    pol = b.charging_report("last_minute", groups=groups)
    p_ref = np.stack([rr.rule_schedule(h, w.load, rr.ALAP, rr.TARGET, 0)[0] for h in homes])
    cr.check(cr.report(p_ref, rec, tariff), pol.row, pol.slot, pol.day, pol.hist, what="last_minute")
    d = rep.compare(pol)
    assert set(d) == {"peak_on", "peak_power", "wait", "cost"} and all(v.shape == (3,) for v in d.values())
    a.step()
    b.step()
    for s in range(3):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()


def test_study_charging(gpu_lib, golden):
    """REVS.study(charging=True) on the 121144 feeder, 2 seeds x {distributed, individual}, the distributed scenarios as
    an ensemble: the individual rows against the yard-stick on the individual optimum of the same homes, the distributed
    rows (the ensemble's own S) against the schedules the study reports; without the flag the field stays None."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.lpsolver import homes_to_arrays
    from revs_admm_amd.revs_fixture import REVS, get_homes_ev_param
    z = golden[0]
    dist = golden_graph(golden)
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), group_by="method", max_iterations=3, v0=1.03,
                arrays=True, mode="relaxed")
    labels, rep = fx.study(tariff, all_homes, dist, com, ensemble=True, charging=True, **grid)
    ch = rep.charging
    assert [lab["method"] for lab in labels] == ["distributed", "individual"] * 2
    assert ch.row.shape == (4, len(res)) and ch.slot.shape == (4, 24) and ch.groups.tolist() == [0, 1, 0, 1] and ch.n_groups == 2
    load = np.array([all_homes[h] for h in res], np.float64)
    for s, lab in enumerate(labels):
        np.random.seed(int(lab["seed"]))
        ev_homes = np.random.choice(com, int(0.9 * len(com)), replace=False)
        homes = get_homes_ev_param(all_homes, dist, ev_homes, 4800 * 1e-3, 20, 0.2, 11, 23)
        rec = homes_to_arrays(homes, res)[1]
        assert int(ch.day["n_ev"][s]) == len(ev_homes) == int((rec["ev"] != 0).sum())
        if lab["method"] == "individual":
            p_ev = fx.get_individual_optimal(tariff, homes)[1]
            p = np.array([p_ev[h] for h in res], F32)
            cr.check(cr.report(p[None], rec[None], tariff.astype(np.float64)), ch.row[s:s + 1], ch.slot[s:s + 1],
                     ch.day[s:s + 1], ch.hist[s:s + 1], what=("study", s))
        else:                                      # g = load + p in float32: the energy is the schedule's less the load's
            assert np.allclose(ch.row["energy"][s], (rep.node_p[s] - load).sum(1), atol=1e-3)
            assert (ch.row["flags"][s] & 1 == (rec["ev"] != 0)).all()
        assert ch.slot["n_on"][s].sum() == ch.row["n_on"][s].sum()
    for k in ("n_on", "n_starts"):
        assert (ch.pooled_slot[k][1] == ch.slot[k][1].astype(np.int64) + ch.slot[k][3]).all()
    assert ch.pooled_energy[0]["count"] == ch.energy[0]["count"] + ch.energy[2]["count"]
    plain = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)[1]
    assert plain.charging is None
