"""The flexibility report on the GPU (csrc/flex_kernels.hip, revs_admm_amd/flexibility.py): every
output of revs_flex_report, through the C ABI and through the Python entries, against the numpy yard-stick
(tests/flex_ref.py) at the charging report's shapes -- one row, one short of and one more than a workgroup's 256 rows,
three workgroups, a slot count below, at and above the chunk, both load widths -- for both kinds of charger, under node
layouts of one node, a node a row, a random partition with empty nodes and a node across a workgroup boundary, and end to
end from the state an engine and an ensemble hold."""
import numpy as np
import pytest

import bills_ref as br
import charge_ref as cr
import flex_ref as fr
from test_gpu_charging import GUARD, SENTINEL, SHAPES, layouts

pytestmark = pytest.mark.gpu

F32 = np.float32
OUTPUTS = ("row", "slot", "day", "hist", "node_up", "node_down", "val", "keep")
CHUNK = 32                     # revs_flex_report_chunk(): checked below


def native(lib, p, homes, integral=0, on_frac=0.0, short_tol=1e-6, node_ptr=None, pad=0, off=0, layout="nst",
           want=OUTPUTS):
    """p (S, n, T) float32 and homes (S, n) on the host -> dict of what revs_flex_report wrote, through the C ABI.
    layout "nst": float[n][S][T + pad] (an ensemble's); "snt": float[S][n][T + pad] (a study's).  off: floats between a
    256-byte boundary and element 0.  Every gap holds SENTINEL; outputs and scratch sit between canaries; the inputs are
    compared before and after.  Without node_ptr the node outputs are not asked for."""
    import torch
    from revs_admm_amd._lib import FLEX_DAY_DTYPE, FLEX_ROW_DTYPE, FLEX_SLOT_DTYPE, check, ptr
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
    m = 0 if node_ptr is None else len(node_ptr) - 1
    h_ptr = None if node_ptr is None else np.ascontiguousarray(node_ptr, np.int64)
    d_ptr = None if node_ptr is None else torch.from_numpy(h_ptr).to(dev)
    if node_ptr is None:
        want = tuple(k for k in want if not k.startswith("node"))
    sizes = dict(row=S * n * 64, slot=S * T * 32, day=S * 64, hist=S * 2 * (T + 1) * 4, node_up=S * m * T * 8,
                 node_down=S * m * T * 8, val=4 * S * n * 8, keep=S * n)
    nbytes = int(lib.revs_flex_report_scratch(S, n, T))
    assert nbytes > 0 and nbytes % 16 == 0
    sizes["scratch"] = nbytes
    guarded = lambda nb: torch.full((GUARD + nb + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    bufs = {k: guarded(sizes[k]) for k in sizes if k == "scratch" or k in want}
    q = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else None
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib.revs_flex_report(S, n, T, ptr(d_p), stride_s, stride_i, ptr(d_homes), int(integral), float(on_frac),
                               float(short_tol), ptr(d_ptr), m, q("row"), q("slot"), q("day"), q("hist"), q("node_up"),
                               q("node_down"), q("val"), q("keep"), q("scratch"), st), "revs_flex_report")
    torch.cuda.synchronize()
    assert d_all.cpu().numpy().tobytes() == flat.tobytes() and d_homes.cpu().numpy().tobytes() == rec.tobytes()
    assert d_ptr is None or d_ptr.cpu().numpy().tobytes() == h_ptr.tobytes()
    kinds = dict(row=(FLEX_ROW_DTYPE, (S, n)), slot=(FLEX_SLOT_DTYPE, (S, T)), day=(FLEX_DAY_DTYPE, (S,)),
                 hist=(np.int32, (S, 2, T + 1)), node_up=(np.float64, (S, m, T)), node_down=(np.float64, (S, m, T)),
                 val=(np.float64, (4, S, n)), keep=(np.uint8, (S, n)))
    out = {k: None for k in OUTPUTS}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xCD).all() and (h[GUARD + sizes[k]:] == 0xCD).all(), ("canary", k)
        if k != "scratch":
            out[k] = h[GUARD:GUARD + sizes[k]].copy().view(kinds[k][0]).reshape(kinds[k][1])
    return out


def node_layouts(rng, n):
    """CSR offsets over n rows: one node owns every row; a node a row; a random partition with empty nodes; where the
    rows span more than a workgroup, a node over the rows 250..262 among nodes of a few rows."""
    out = [np.array([0, n]), np.arange(n + 1)]
    cuts = np.sort(rng.integers(0, n + 1, max(n // 5, 3)))
    out.append(np.concatenate([[0, 0], cuts, [n, n]]))
    if n > 256:
        out.append(np.concatenate([np.arange(0, 250, 7), [250], [263] if n > 263 else [], np.arange(270, n, 11), [n]]))
    return [np.asarray(a, np.int64) for a in out]


def test_the_shapes_cover_every_value(gpu_lib):
    assert int(gpu_lib.revs_flex_report_chunk()) == CHUNK == int(gpu_lib.revs_charge_report_chunk())
    assert {s[0] for s in SHAPES} == {1, 255, 257, 600} and {s[1] for s in SHAPES} == {1, 3}
    assert {s[2] for s in SHAPES} >= {1, 5, 24, 96, 192, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1}
    lay = node_layouts(np.random.default_rng(0), 600)
    assert len(lay) == 4 and (np.diff(lay[2]) == 0).any() and any(a <= 250 and b >= 263 for a, b in zip(lay[3], lay[3][1:]))
    assert all(a[0] == 0 and a[-1] == 600 and (np.diff(a) >= 0).all() for a in lay)


@pytest.mark.parametrize("integral", [0, 1])
@pytest.mark.parametrize("n,S,T", SHAPES)
def test_outputs_at_every_shape(gpu_lib, n, S, T, integral):
    rng = np.random.default_rng(1000 * n + 10 * T + S)
    on_frac, tol = (0.0, 1e-6) if (n + T) % 2 else (0.25, 1e-3)
    p, homes = cr.random_case(rng, S, n, T, on_frac, tol)
    ref = fr.report(p, homes, integral, on_frac, tol)
    if n >= len(cr.AWKWARD):                       # every awkward row is there, and some rows are not kept
        assert (ref.row["flags"][0] & 4).any() and not ref.keep[0].all()
    if n >= 255 and T > 1:
        assert (ref.up > 0).any() and (ref.down > 0).any() and (ref.row["flags"] & 2).any() and (ref.row["ready"] > 0).any()
    if S > 1:
        assert ref.day["n_ev"][1] == 0 and ref.day["n_ev"][0] > 0
    node_refs = [(ptr, fr.node_sums(ref.up, ptr), fr.node_sums(ref.down, ptr)) for ptr in node_layouts(rng, n)]
    for pad, off, layout in layouts(T):
        for ptr, nup, ndn in node_refs:
            out = native(gpu_lib, p, homes, integral, on_frac, tol, ptr, pad, off, layout)
            what = (n, S, T, integral, pad, off, layout, len(ptr) - 1)
            assert out["node_up"].tobytes() == nup.tobytes(), (what, "node_up")
            assert out["node_down"].tobytes() == ndn.tobytes(), (what, "node_down")
            fr.check(ref, out["row"], out["slot"], out["day"], out["hist"], out["val"], out["keep"], what=what)


def test_each_output_alone_and_two_calls_give_the_same_bytes(gpu_lib):
    rng = np.random.default_rng(7)
    S, n, T = 3, 600, 33
    p, homes = cr.random_case(rng, S, n, T)
    ptr = node_layouts(rng, n)[3]
    full = native(gpu_lib, p, homes, 0, node_ptr=ptr)
    again = native(gpu_lib, p, homes, 0, node_ptr=ptr)
    for k in OUTPUTS:
        assert full[k].tobytes() == again[k].tobytes(), k
    for k in ("row", "slot", "day", "hist", "val", "keep"):
        part = native(gpu_lib, p, homes, 0, want=(k,))
        assert all((part[j] is None) == (j != k) for j in OUTPUTS)
        assert part[k].tobytes() == full[k].tobytes(), k
    part = native(gpu_lib, p, homes, 0, node_ptr=ptr, want=("node_up", "node_down"))     # (the two come together)
    assert all((part[j] is None) == (not j.startswith("node")) for j in OUTPUTS)
    assert part["node_up"].tobytes() == full["node_up"].tobytes() and part["node_down"].tobytes() == full["node_down"].tobytes()
    # the other layout sums the same rows in the same order: the same bytes again
    other = native(gpu_lib, p, homes, 0, node_ptr=ptr, pad=3, off=1, layout="snt")
    for k in OUTPUTS:
        assert other[k].tobytes() == full[k].tobytes(), k


def test_box_records_over_val_out(gpu_lib):
    """revs_bill_study (base = -1) over val_out under keep_out: bills_ref's record of the yard-stick's values, per
    scenario and pooled; through the Python entry, which also pools the integer records on the host."""
    from revs_admm_amd import flexibility as fx
    rng = np.random.default_rng(9)
    S, n, T = 3, 300, 24
    p, homes = cr.random_case(rng, S, n, T)
    homes["ev"][1] = rng.random(n) < 0.5           # (three scenarios with EVs: a pool of two and one alone)
    groups = [0, -1, 0]
    ptr = node_layouts(rng, n)[2]
    ref = fr.report(p, homes, 1, 0.1)
    rep = fx.flexibility_report(p, homes, 1, ptr, groups=groups, on_frac=0.1)
    fr.check(ref, rep.row, rep.slot, rep.day, rep.hist, node_up=rep.node_up, node_down=rep.node_down, node_ptr=ptr,
             what="python entry")
    assert rep.n_groups == 1 and rep.groups.tolist() == groups and rep.integral == 1
    for q, name in enumerate(fx.QUANTITIES):
        for s in range(S):
            br.check_record(getattr(rep, name)[s], br.record(ref.val[q], ref.keep, [s]), (name, s))
        br.check_record(getattr(rep, "pooled_" + name)[0], br.record(ref.val[q], ref.keep, [0, 2]), (name, "pool"))
    never = ((ref.row["ready"] < 0) & (ref.keep != 0)).sum(1)
    assert never.any() and (rep.slack["n_nan"] == never).all() and (rep.up_energy["n_nan"] == 0).all()
    for k in ("n_plugged", "n_up", "n_down"):
        assert (rep.pooled_slot[k][0] == ref.slot[k][0] + ref.slot[k][2]).all(), k
    assert (rep.pooled_hist[0] == ref.hist[0] + ref.hist[2]).all()
    assert rep.up_curve().tobytes() == rep.slot["up"].tobytes()
    lean = fx.flexibility_report(p, homes, 1, ptr, groups=groups, on_frac=0.1, rows=False, nodes=False)
    assert lean.row is None and lean.row_device is None and lean.node_up is None and lean.node_down is None
    assert lean.slot.tobytes() == rep.slot.tobytes() and lean.day.tobytes() == rep.day.tobytes()
    assert lean.up_energy.tobytes() == rep.up_energy.tobytes()
    kept = fx.flexibility_report(p, homes, 1, ptr, groups=groups, on_frac=0.1, rows="device", nodes="device")
    assert kept.row is None and kept.row_device.is_cuda and kept.row_device.cpu().numpy().tobytes() == rep.row.tobytes()
    assert kept.node_up.is_cuda and kept.node_up.cpu().numpy().tobytes() == rep.node_up.tobytes()
    assert kept.node_down.cpu().numpy().tobytes() == rep.node_down.tobytes()
    with pytest.raises(ValueError, match="node_ptr must ascend"):
        fx.flexibility_report(p, homes, 1, [0, 10, 5, n])


def _same_but_sums(rep, free, what):
    """A method's report against the free function's on result()'s S in the caller's order: rows, counts, histograms and
    box records bit for bit; the sums over the rows of a scenario (another order) are left to the yard-stick's bound."""
    assert rep.row.tobytes() == free.row.tobytes(), what
    assert rep.hist.tobytes() == free.hist.tobytes() and rep.pooled_hist.tobytes() == free.pooled_hist.tobytes(), what
    assert rep.pooled_slot.tobytes() == free.pooled_slot.tobytes(), what
    for k in fr.SLOT_INT:
        assert rep.slot[k].tobytes() == free.slot[k].tobytes(), (what, k)
    for k in fr.DAY_INT:
        assert rep.day[k].tobytes() == free.day[k].tobytes(), (what, k)
    for name in fr.QUANTITIES:
        assert getattr(rep, name).tobytes() == getattr(free, name).tobytes(), (what, name)
        assert getattr(rep, "pooled_" + name).tobytes() == getattr(free, "pooled_" + name).tobytes(), (what, name)


def _anchors(report, homes_list, load, T):
    """The two anchors of test_flex_host.py on the device, from the engine's own rule schedules: with on/off chargers a
    last-minute schedule to the target leaves nothing to cut and an uncontrolled one to full nothing to add, exactly, on
    the rows the rule serves; with continuous chargers within rating 2^-23 a slot."""
    import rules_ref as rr
    for policy, fill, code, which in (("last_minute", "target", (rr.ALAP, rr.TARGET), "down"),
                                      ("uncontrolled", "full", (rr.ASAP, rr.FULL), "up")):
        rep = report(policy, fill=fill, charger="binary")
        assert rep.integral == 1
        for s, homes in enumerate(homes_list):
            ok = (rr.rule_schedule(homes, load, *code, 1)[3] == 0) & (homes["ev"] != 0)
            assert ok.sum() > 10 and (rep.row["n_" + which][s][ok] == 0).all(), (policy, s)
            assert (rep.row[which + "_energy"][s][ok] == 0).all(), (policy, s)
        other = "up" if which == "down" else "down"
        assert (rep.day[other + "_energy"] > 0).all(), policy
        rep = report(policy, fill=fill, charger="continuous")
        assert rep.integral == 0
        for s, homes in enumerate(homes_list):
            ok = (rr.rule_schedule(homes, load, *code, 0)[3] == 0) & (homes["ev"] != 0)
            bound = T * homes["rating"].astype(np.float64) * 2.0 ** -23
            assert ok.sum() > 10 and (rep.row[which + "_energy"][s][ok] <= bound[ok]).all(), (policy, s)


def test_engine_end_to_end(gpu_lib):
    from test_gpu_conv import _single
    import rules_ref as rr
    from revs_admm_amd import flexibility as fx
    w, make = _single()
    e, f = make(), make()
    for x in (e, f):
        x.run_steps(2)
    with pytest.raises(RuntimeError, match="did not write the charger power"):
        e.flexibility_report()
    for x in (e, f):
        x.step()
    power = e.result()[1]
    rep = e.flexibility_report()
    free = fx.flexibility_report(power, w.homes, 0)
    assert rep.row.shape == (1, 300) and rep.slot.shape == (1, 24) and rep.hist.shape == (1, 2, 25) and rep.integral == 0
    assert free.node_up is None
    _same_but_sums(rep, free, "engine")
    ref = fr.report(power[None], w.homes[None], 0)
    fr.check(ref, rep.row, rep.slot, rep.day, rep.hist, what="engine")
    # the node arrays: the engine's nodes, over the rows in the engine's order
    ptr = e.node_ptr.cpu().numpy()
    assert rep.node_up.shape == (1, e.M, 24) and len(ptr) == e.M + 1
    assert rep.node_up.tobytes() == fr.node_sums(ref.up[:, e.perm], ptr).tobytes()
    assert rep.node_down.tobytes() == fr.node_sums(ref.down[:, e.perm], ptr).tobytes()
    assert int(rep.day["n_ev"][0]) == int((w.homes["ev"] != 0).sum()) > 0 and rep.day["up_energy"][0] > 0
    # a policy name: the p of the rule schedule, as rules_ref gives it
    pol = e.flexibility_report("uncontrolled", nodes=False)
    p_ref = rr.rule_schedule(w.homes, w.load, rr.ASAP, rr.TARGET, 0)[0]
    fr.check(fr.report(p_ref[None], w.homes[None], 0), pol.row, pol.slot, pol.day, pol.hist, what="uncontrolled")
    assert pol.node_up is None
    _anchors(e.flexibility_report, [w.homes], w.load, 24)
    # a tensor in the engine's order
    t = e.flexibility_report(e.S.clone(), nodes="device")
    assert t.row.tobytes() == rep.row.tobytes() and t.day.tobytes() == rep.day.tobytes()
    assert t.node_up.is_cuda and t.node_up.cpu().numpy().tobytes() == rep.node_up.tobytes()
    with pytest.raises(ValueError, match="profile must be"):
        e.flexibility_report("cheapest")
    with pytest.raises(ValueError, match="power tensor must be"):
        e.flexibility_report(e.S[:10])
    # the state is as it was: the run goes on bit for bit as one that was never asked
    e.step()
    f.step()
    for x, y in zip(e.get_state(), f.get_state()):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(e.result(), f.result()):
        assert x.tobytes() == y.tobytes()


def test_ensemble_end_to_end(gpu_lib):
    from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
    from revs_admm_amd import flexibility as fx
    w = _workload(n=300, n_nodes=30)
    homes = _mixed_scenarios(w, 3)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for x in (a, b):
        x.run_steps(2)
    with pytest.raises(RuntimeError, match="did not write the charger power"):
        b.flexibility_report()
    for x in (a, b):
        x.step()
    rec = np.stack(homes)
    power = b.result()[1]
    groups = [0, -1, 0]
    rep = b.flexibility_report(groups=groups, short_tol=1e-4)
    free = fx.flexibility_report(power, rec, 0, groups=groups, short_tol=1e-4)
    assert rep.row.shape == (3, 300) and rep.slot.shape == (3, 24) and rep.pooled_slot.shape == (1, 24)
    _same_but_sums(rep, free, "ensemble")
    ref = fr.report(power, rec, 0, 0.0, 1e-4)
    fr.check(ref, rep.row, rep.slot, rep.day, rep.hist, what="ensemble")
    ptr = b.node_ptr.cpu().numpy()
    assert rep.node_up.shape == (3, b.M, 24)
    assert rep.node_up.tobytes() == fr.node_sums(ref.up[:, b.perm], ptr).tobytes()
    assert rep.node_down.tobytes() == fr.node_sums(ref.down[:, b.perm], ptr).tobytes()
    assert (rep.day["n_ev"] == (rec["ev"] != 0).sum(1)).all()
    _anchors(b.flexibility_report, homes, w.load, 24)
    a.step()
    b.step()
    for s in range(3):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()


def test_study_flexibility(gpu_lib, golden):
    """REVS.study(flexibility=True) on the 121144 feeder, 2 seeds x {distributed, individual}, the distributed scenarios
    as an ensemble: the individual rows against the yard-stick on the individual optimum of the same homes; without the
    flag the field stays None."""
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
    labels, rep = fx.study(tariff, all_homes, dist, com, ensemble=True, flexibility=True, **grid)
    fl = rep.flexibility
    assert [lab["method"] for lab in labels] == ["distributed", "individual"] * 2 and rep.charging is None
    assert fl.row.shape == (4, len(res)) and fl.slot.shape == (4, 24) and fl.groups.tolist() == [0, 1, 0, 1] and fl.n_groups == 2
    assert fl.integral == 0 and fl.node_up is None
    for s, lab in enumerate(labels):
        np.random.seed(int(lab["seed"]))
        ev_homes = np.random.choice(com, int(0.9 * len(com)), replace=False)
        homes = get_homes_ev_param(all_homes, dist, ev_homes, 4800 * 1e-3, 20, 0.2, 11, 23)
        rec = homes_to_arrays(homes, res)[1]
        assert int(fl.day["n_ev"][s]) == len(ev_homes) == int((rec["ev"] != 0).sum())
        if lab["method"] == "individual":
            p_ev = fx.get_individual_optimal(tariff, homes)[1]
            p = np.array([p_ev[h] for h in res], F32)
            fr.check(fr.report(p[None], rec[None], 0), fl.row[s:s + 1], fl.slot[s:s + 1], fl.day[s:s + 1],
                     fl.hist[s:s + 1], what=("study", s))
        else:
            assert (fl.row["flags"][s] & 1 == (rec["ev"] != 0)).all()
        assert fl.slot["n_up"][s].sum() == fl.row["n_up"][s].sum() and fl.slot["n_down"][s].sum() == fl.row["n_down"][s].sum()
    for k in ("n_up", "n_down"):
        assert (fl.pooled_slot[k][1] == fl.slot[k][1].astype(np.int64) + fl.slot[k][3]).all()
    assert fl.pooled_up_energy[0]["count"] == fl.up_energy[0]["count"] + fl.up_energy[2]["count"]
