"""The price report on the GPU (revs_net_prices; prices.report_for_tree, AdmmEngine.price_report,
AdmmEnsemble.price_reports) against tests/price_ref.py.

Kernel against the other entry points: line_y and (at s = 1) cong hold the bytes revs_net_report's scans give when fed
the multipliers -- its flow_out, and the drop_out of revs_net_losses, which carries those scans' drop --; flow and drop
those on the injections; lossp / cost, with powers of two as cost, the bytes of revs_net_losses' mlf_out.  Kernel against
restatement: every other array and every field of every record is bit for bit contract() fed the kernel's own scans
(flow, drop, line_y and -- from a second call with s = 1 and cost = 1 -- d and mlf); the summaries by the loss report's
rules (== for order statistics and counts, <= 2 ulp for the interpolated quartiles).  Loads are scaled so that the deepest
drop is 0.15 at vset = 1: no bad slot except those put in on purpose."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import headroom_ref as hr
import price_ref as pr
from test_gpu_losses import bits, same
from test_gpu_network import synthetic_forest, ulps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("price", "cong", "lossp", "line_y", "rent", "drop", "flow")
RECORDS = ("summary", "slot", "node_day", "line_day", "day")
SLOT_F = ("delivered", "energy_pay", "loss_pay", "cong_pay", "rent_total", "price_max", "price_min", "cong_max")
SLOT_I = ("price_max_index", "price_min_index", "cong_max_index", "n_priced", "n_rows", "n_bad")


def check_report(rep, par, er, cons, p, y, cost, scale=1.0, with_loss=True, lines=None, nodes=None, slot_hours=None,
                 price_cap=np.inf, vset=1.0):
    """One scenario's PriceReport against contract() on its own scans; d and mlf come from a call with s = 1, cost = 1."""
    from revs_admm_amd.feeder import feeder_tree
    from revs_admm_amd.prices import report_for_tree
    n, T = len(par), p.shape[1]
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    unit = report_for_tree(par, er, cons, p, y, cost=np.ones(T), with_loss=with_loss, vset=vset)
    for k in ("flow", "drop", "line_y"):
        assert getattr(unit, k).tobytes() == getattr(rep, k).tobytes(), k

    def mask(sel):
        if sel is None:
            return None
        mk = np.zeros(n, bool)
        mk[np.asarray(sel, np.int64)] = True
        return hr.to_pos(tree, mk, False)

    pos = lambda a: hr.to_pos(tree, a)
    hours = 24.0 / T if slot_hours is None else slot_hours
    b = pr.contract(tree, n, pos(rep.flow), pos(rep.drop), pos(rep.line_y), pos(unit.cong), pos(unit.lossp),
                    pr.gathered(tree, p), pr.gathered(tree, y), scale, cost, vset * vset, with_loss, mask(lines), mask(nodes),
                    hours, price_cap)
    for k in ("price", "cong", "lossp", "rent"):
        bits(getattr(rep, k), hr.to_nodes(tree, b[k], n), k)
    for k in SLOT_F:
        bits(rep.slot[k], b["slot"][k], k)
    for k in SLOT_I:
        assert same(rep.slot[k], b["slot"][k]), (k, rep.slot[k], b["slot"][k])
    for t, r in enumerate(b["summary"]):
        g = rep.summary[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"]), (t, g, r)
        if r["count"] == 0:
            assert np.isnan(g["min"]) and np.isnan(g["median"]) and np.isnan(g["worst_value"]) and g["n_fliers"] == 0
            continue
        box = r["box"]
        for k in ("min", "max", "whisker_lo", "whisker_hi"):
            assert g[k] == box[k], (t, k, g[k], box[k])
        assert g["worst_value"] == r["worst_value"]
        for k in ("q1", "median", "q3"):
            assert ulps(g[k], box[k]) <= 2, (t, k, g[k], box[k])
        assert g["n_fliers"] == box["n_fliers"], (t, g, box)
    for k in ("paid", "cong_paid", "peak_price"):
        bits(rep.node_day[k], b["node_day"][k], "node_day " + k)
    assert same(rep.node_day["peak_slot"], b["node_day"]["peak_slot"])
    for k in ("energy", "peak"):
        bits(rep.line_day[k], b["line_day"][k], "line_day " + k)
    assert same(rep.line_day["peak_slot"], b["line_day"]["peak_slot"])
    for k in ("energy_pay", "loss_pay", "cong_pay", "rent_total", "peak_price", "top_rent"):
        bits(rep.day[k], b["day"][k], "day " + k)
    assert same(rep.day["top_index"], b["day"]["top_index"]), (rep.day["top_index"], b["day"]["top_index"])
    for k in ("peak_slot", "peak_index", "n_bad_slots", "n_cong_slots"):
        assert rep.day[k] == b["day"][k], (k, rep.day[k], b["day"][k])
    return b


def run(par, er, cons, p, y, cost, **kw):
    from revs_admm_amd.prices import report_for_tree
    rep = report_for_tree(par, er, cons, p, y, cost=cost, **kw)
    check_report(rep, par, er, cons, p, y, cost, **kw)
    return rep


def scaled_loads(par, er, cons, p, deepest=0.15):
    """p scaled so that the deepest drop R p is `deepest` (numpy's scans: feeder.tree_report_host)."""
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    return p * (deepest / np.abs(tree_report_host(tree, p, len(par))[1]).max())


def multipliers(rng, M, T, frac=0.05):
    """Signed multipliers on about `frac` of the rows, at least one row."""
    y = np.where(rng.random((M, T)) < frac, rng.normal(0.0, 0.5, (M, T)), 0.0)
    y[rng.integers(M), :] = 0.25
    return y


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("M", [8, 2048, 4096, 8192, 8200, 16384])
def test_every_tree_shape_matches_the_restatements(gpu_lib, M, T):
    """One thread (8), 256 x 8, 512 x 8, 1024 x 8, the first 1024 x 16 size (8200 pads to 8208) and the largest, signed
    multipliers on about 5 % of the rows, a line mask, a node mask, a scale, a price cap and powers of two as tariff.
    T = 3 carries two bad slots: slot 1 a NaN multiplier, slot 2 the loads scaled to a deepest drop of 1.2 > vset^2."""
    from revs_admm_amd.losses import report_for_tree as loss_report
    from revs_admm_amd.network import report_for_tree as net_report
    from revs_admm_amd.prices import report_for_tree
    rng = np.random.default_rng(M + T)
    par, er, cons = synthetic_forest(M, M)
    er[rng.random(M) < 0.05] = 0.0
    p = scaled_loads(par, er, cons, rng.uniform(0.0, 4.0, (M, T)) * np.where(rng.random((M, 1)) < 0.1, -0.5, 1.0))
    y = multipliers(rng, M, T)
    if T == 3:
        y[M // 3, 1] = np.nan
        p[:, 2] *= 1.2 / 0.15
    lines, nodes = np.flatnonzero(rng.random(M) < 0.7), np.flatnonzero(rng.random(M) < 0.6)
    cost = 2.0 ** rng.integers(-4, 0, T).astype(np.float64)
    # ---- the scans: the other entry points' bytes
    unit = report_for_tree(par, er, cons, p, y, cost=cost)
    of_y, of_g = loss_report(par, er, cons, y), loss_report(par, er, cons, p)
    assert unit.line_y.tobytes() == of_y.flow.tobytes() == net_report(par, er, cons, y).flow.tobytes()
    assert unit.flow.tobytes() == of_g.flow.tobytes() == net_report(par, er, cons, p).flow.tobytes()
    assert unit.drop.tobytes() == of_g.drop.tobytes()
    good = unit.slot["n_bad"] == 0
    assert good.tolist() == ([True] if T == 1 else [True, False, False])
    assert unit.cong[:, good].tobytes() == of_y.drop[:, good].tobytes()
    assert (unit.lossp / cost)[:, good].tobytes() == of_g.mlf[:, good].tobytes()
    assert np.isnan(unit.cong[:, ~good]).all() and np.isnan(unit.lossp[:, ~good]).all()
    # ---- everything else: the restatement
    # (a tenth of the summarised nodes above the cap: the prices at s = 0.75 up to their rounding)
    cap = float(np.quantile((cost[0] + unit.lossp[nodes, 0]) + 0.75 * unit.cong[nodes, 0], 0.9)) if M > 8 else 0.1
    rep = run(par, er, cons, p, y, cost, scale=0.75, lines=lines, nodes=nodes, slot_hours=0.25, price_cap=cap)
    assert rep.slot["n_bad"].tolist() == ([0] if T == 1 else [0, 1, 1]) and rep.day["n_bad_slots"] == T - 1
    assert rep.slot["n_rows"][0] == (y[:, 0] != 0).sum() > 0 and rep.slot["n_priced"][0] > 0
    assert rep.summary["count"][0] == len(nodes) and (M == 8 or rep.summary["n_violations"][0] > 0)
    assert rep.scale == 0.75 and np.array_equal(rep.reinforcement_value(), 2.0 * 0.75 * rep.line_y * rep.flow, equal_nan=True)


def test_chain_of_depth_2048(gpu_lib):
    """One lateral of 2048 nodes with a positive multiplier at its end and one half-way: every line carries the last one,
    cong grows along the lateral, the largest price is at the end."""
    n = 2048
    rng = np.random.default_rng(4)
    par, er, cons = np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n)
    p = scaled_loads(par, er, cons, rng.uniform(0.0, 1.0, (n, 2)))
    y = np.zeros((n, 2))
    y[n - 1], y[n // 2] = 0.5, 0.25
    rep = run(par, er, cons, p, y, np.array([0.25, 0.5]))
    assert (rep.line_y[: n // 2 + 1] == 0.75).all() and (rep.line_y[n // 2 + 1:] == 0.5).all()
    assert (np.diff(rep.cong[:, 0]) > 0).all() and rep.slot["price_max_index"].tolist() == [n - 1, n - 1]
    assert rep.slot["n_rows"].tolist() == [2, 2] and rep.day["n_cong_slots"] == 2 and (rep.rent > 0).all()


def small_case(M=300, T=5, seed=300):
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed)
    p = scaled_loads(par, er, cons, rng.uniform(-0.3, 4.0, (M, T)))
    return par, er, cons, p, multipliers(rng, M, T, 0.08), rng


@pytest.mark.parametrize("with_loss", [True, False])
def test_scenario_grid_equals_single_calls(gpu_lib, with_loss):
    """S = 3 x T = 5 on 300 nodes, masks, one scale per scenario: every scenario against the restatement, its slice equal
    in bytes to the S = 1 call on that scenario with that scale."""
    from revs_admm_amd.prices import report_for_tree
    par, er, cons, p, y, rng = small_case()
    f = rng.uniform(0.5, 1.0, p.shape[1])
    ps, ys = np.stack([p, p * f, p[::-1].copy()]), np.stack([y, -y, y[::-1].copy()])
    scales, cost = np.array([1.0, 0.0, 2.5]), rng.uniform(0.1, 0.3, 5)
    kw = dict(lines=np.flatnonzero(rng.random(300) < 0.6), nodes=np.flatnonzero(rng.random(300) < 0.5), price_cap=0.15,
              with_loss=with_loss, slot_hours=0.5)
    reps = report_for_tree(par, er, cons, ps, ys, scale=scales, cost=cost, **kw)
    assert len(reps) == 3
    for s, rep in enumerate(reps):
        check_report(rep, par, er, cons, ps[s], ys[s], cost, scale=scales[s], **kw)
        one = report_for_tree(par, er, cons, ps[s], ys[s], scale=scales[s], cost=cost, **kw)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (s, k)
    assert (reps[1].cong == 0).all() and (reps[1].rent == 0).all() and reps[1].day["n_cong_slots"] == 5
    assert (reps[0].lossp == 0).all() == (not with_loss) and len(reps[0].top_lines) == 8
    assert reps[0].summary["n_violations"].max() > 0 and reps[0].slot_hours == 0.5
    sh = reps[0].shares()
    assert abs(sum(sh.values()) - 100.0) < 1e-9 and sh["energy"] > 0 and (sh["loss"] > 0) == with_loss


def _raw(lib, tree, th, g, yv, scale, cost, outs, scratch, lm=None, nm=None, nop=None, with_loss=1):
    import ctypes as C
    S, M, T = g.shape
    p = lambda t: None if t is None else t.data_ptr()
    return lib.revs_net_prices(S, M, T, C.byref(tree), p(g), p(yv), p(scale), p(cost), p(lm), p(nm), p(nop), M, 1.0, with_loss,
                               0.5, 0.2, *[p(o) for o in outs], p(scratch), None)


def test_every_output_alone_and_records_only(gpu_lib):
    """Each output with every other one NULL holds the bytes of the full call (the arrays without any scratch);
    arrays=False gives the same records."""
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.network import SUMMARY_DTYPE, side_arrays, tree_on_device
    from revs_admm_amd.prices import report_for_tree
    from revs_admm_amd.tree_reports import position_mask
    par, er, cons, p, y, rng = small_case(300, 4, 12)
    y[7, 2] = np.inf                                              # (a bad slot among them)
    lines, cost = np.flatnonzero(rng.random(300) < 0.6), rng.uniform(0.1, 0.3, 4)
    kw = dict(lines=lines, cost=cost, price_cap=0.2, slot_hours=0.5, scale=0.5)
    full = report_for_tree(par, er, cons, p, y, **kw)
    only = report_for_tree(par, er, cons, p, y, arrays=False, **kw)
    assert all(getattr(only, k) is None for k in ARRAYS) and full.slot["n_bad"].tolist() == [0, 0, 1, 0]
    for k in RECORDS:
        assert getattr(only, k).tobytes() == getattr(full, k).tobytes(), k
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    d_nop, _, _ = side_arrays(dev, th, 300, None, None)
    d_lm = position_mask(dev, th, 300, lines, "no array")
    g, yv = torch.from_numpy(p[None].copy()).to(dev), torch.from_numpy(y[None].copy()).to(dev)
    d_cost, d_scale = torch.from_numpy(cost).to(dev), torch.tensor([0.5], dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.revs_net_prices_scratch(1, 4, th["n"]) // 8, dtype=torch.float64, device=dev)
    wants = [getattr(full, k) for k in ARRAYS + RECORDS]
    sizes = [300 * 4 * 8] * 7 + [4 * SUMMARY_DTYPE.itemsize, 4 * 96, 300 * 32, 300 * 24, 160]
    for k in range(12):
        outs = [None] * 12
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = _raw(lib, tree, th, g, yv, d_scale, d_cost, outs, scratch if k in (7, 9, 10, 11) else None, lm=d_lm, nop=d_nop)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k
    assert _lib.PRICE_SLOT_DTYPE.itemsize == 96


def test_bad_slots(gpu_lib):
    """A NaN multiplier in slot 0, den <= 0 in slot 2 (only with the loss term), a negative and a NaN scale (the library's
    own test: the Python layer refuses them first): price, cong, lossp, rent and the records' doubles are NaN, the indices
    -1, the summary empty with n_nan = the nodes summarised; drop, flow and line_y are what the scans give."""
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.network import side_arrays, tree_on_device
    from revs_admm_amd.prices import report_for_tree
    par, er, cons, p, y, rng = small_case(300, 3, 7)
    cost = np.array([0.25, 0.5, 0.125])
    clean = report_for_tree(par, er, cons, p, y, cost=cost)
    y2, p2 = y.copy(), p.copy()
    y2[11, 0] = np.nan
    p2[:, 2] *= 1.2 / 0.15
    rep = run(par, er, cons, p2, y2, cost)
    assert rep.slot["n_bad"].tolist() == [1, 0, 1] and rep.day["n_bad_slots"] == 2 and rep.day["peak_slot"] == -1
    for k in ("price", "cong", "lossp", "rent"):
        a = getattr(rep, k)
        assert np.isnan(a[:, [0, 2]]).all() and a[:, 1].tobytes() == getattr(clean, k)[:, 1].tobytes(), k
    assert rep.flow[:, 0].tobytes() == clean.flow[:, 0].tobytes() and np.isfinite(rep.drop).all()
    assert np.isfinite(np.delete(rep.line_y[:, 0], np.flatnonzero(np.isnan(rep.line_y[:, 0])))).all()
    assert rep.summary["count"].tolist() == [0, 300, 0] and rep.summary["n_nan"].tolist() == [300, 0, 300]
    assert (rep.slot["price_max_index"][[0, 2]] == -1).all() and np.isnan(rep.slot["delivered"][[0, 2]]).all()
    assert np.isnan(rep.node_day["paid"]).all() and (rep.node_day["peak_slot"] == -1).all()
    no_loss = run(par, er, cons, p2, y2, cost, with_loss=False)      # (the collapse is the loss term's alone)
    assert no_loss.slot["n_bad"].tolist() == [1, 0, 0]
    # ---- the scales, on the library itself
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    d_nop, _, _ = side_arrays(dev, th, 300, None, None)
    g = torch.from_numpy(np.stack([p, p, p])).to(dev)
    yv = torch.from_numpy(np.stack([y, y, y])).to(dev)
    d_scale = torch.tensor([-1.0, float("nan"), 1.0], dtype=torch.float64, device=dev)
    price = torch.zeros(3, 300, 3, dtype=torch.float64, device=dev)
    slot = torch.zeros(9 * 96, dtype=torch.uint8, device=dev)
    outs = [price] + [None] * 7 + [slot] + [None] * 3
    assert _raw(lib, tree, th, g, yv, d_scale, torch.from_numpy(cost).to(dev), outs, None, nop=d_nop) == 0, lib.revs_last_error()
    torch.cuda.synchronize()
    rec = slot.cpu().numpy().view(_lib.PRICE_SLOT_DTYPE).reshape(3, 3)
    assert rec["n_bad"].tolist() == [[1] * 3, [1] * 3, [0] * 3] and np.isnan(price[:2].cpu().numpy()).all()
    assert np.isnan(rec["cong_pay"][:2]).all() and (rec["cong_max_index"][:2] == -1).all()
    assert price[2].cpu().numpy().tobytes() == clean.price.tobytes()


def test_ties_and_fewer_than_eight_lines(gpu_lib):
    """Twelve equal laterals of one line each under equal loads and multipliers: every price and rent ties -- the indices
    are 0, the top 8 are lines 0..7 in order (without the loss term: mlf is a block scan of inexact terms, whose last bits
    differ from position to position).  Five lines of which three carry a multiplier: the top 8 order the zero
    rents behind them by index and end in -1 / NaN."""
    eq = np.full(12, -1), np.full(12, 0.5), np.arange(12)
    rep = run(*eq, np.full((12, 2), 0.25), np.full((12, 2), 0.5), np.array([0.25, 0.25]), with_loss=False)
    assert (rep.summary["worst_index"] == 0).all() and rep.day["top_index"].tolist() == list(range(8))
    assert (rep.slot["price_max_index"] == 0).all() and (rep.slot["price_min_index"] == 0).all()
    assert len(set(rep.price.ravel().tolist())) == 1 and rep.day["peak_slot"] == 0 and rep.day["peak_index"] == 0
    assert (rep.node_day["peak_slot"] == 0).all() and (rep.line_day["peak_slot"] == 0).all()
    rep = run(*eq, np.full((12, 2), 0.25), np.full((12, 2), 0.5), np.array([0.25, 0.25]), lines=[11, 3, 5], nodes=[9, 4],
              with_loss=False)
    assert (rep.summary["worst_index"] == 4).all() and rep.day["top_index"].tolist() == [3, 5, 11, -1, -1, -1, -1, -1]
    par = np.array([-1, 0, 1, 0, 3])
    y = np.array([[0.0], [0.0], [0.5], [0.0], [0.5]])
    rep = run(par, np.array([0.25, 0.5, 0.5, 0.5, 0.5]), np.arange(5), np.array([[0.0], [0.03125], [0.0625], [0.03125], [0.0625]]),
              y, np.array([0.5]), with_loss=False)
    assert rep.day["top_index"].tolist() == [0, 1, 3, 2, 4, -1, -1, -1] and np.isnan(rep.day["top_rent"][5:]).all()
    assert rep.rent[1, 0] == rep.rent[3, 0] and rep.rent[2, 0] == rep.rent[4, 0] and rep.slot["cong_max_index"][0] == 2
    assert rep.slot["n_rows"][0] == 2 and rep.slot["n_priced"][0] == 5


def test_zero_multipliers_price_energy_and_loss_alone(gpu_lib):
    """y = 0: price == cost + lossp exactly, every cong and rent is +0.0, nothing is priced."""
    from revs_admm_amd.losses import report_for_tree as loss_report
    par, er, cons, p, y, rng = small_case(300, 3, 21)
    cost = np.array([0.25, 0.5, 0.125])
    rep = run(par, er, cons, p, np.zeros_like(p), cost, scale=3.0)
    assert rep.price.tobytes() == (cost[None, :] + rep.lossp).tobytes()
    zero = np.zeros_like(p).tobytes()
    assert rep.cong.tobytes() == zero and rep.rent.tobytes() == zero and rep.line_y.tobytes() == zero
    assert rep.slot["n_priced"].sum() == 0 and rep.slot["n_rows"].sum() == 0 and rep.day["n_cong_slots"] == 0
    assert rep.day["cong_pay"] == 0 and rep.day["rent_total"] == 0 and rep.shares()["congestion"] == 0
    assert (rep.lossp / cost).tobytes() == loss_report(par, er, cons, p).mlf.tobytes()
    assert rep.day["top_index"].tolist() == list(range(8)) and (rep.day["top_rent"] == 0).all()


def _binding_workload():
    from test_gpu_ensemble import _workload
    return _workload(stress=1.5)


def _node_sums(w, prof):
    g = np.zeros((w.M, prof.shape[1]))
    np.add.at(g, w.node_of, prof)
    return g


def test_engine_price_report(gpu_lib):
    """The workload on which test_gpu_ensemble.py sees multipliers (stress 1.5): after 8 iterations the operator holds a
    y with |y|.max() > 0; price_report() is the restatement on LOAD + P_sch and yd[0], the tariff the engine's own,
    slot_hours 24 / T; a given (M, T) array and the certificate's scale go the same way; the run's state keeps its bytes."""
    from revs_admm_amd.engine import AdmmEngine
    w = _binding_workload()
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="relaxed_exact", feeder=w.feeder)
    e.run(8)
    y = e.yd[0].cpu().numpy().copy()
    assert e.op.solver == "newton" and e._y_support and np.abs(y).max() > 0
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0])]
    cost = w.cost.astype(np.float64)
    g = _node_sums(w, w.load.astype(np.float64) + e.result()[0].astype(np.float64))
    feeder = (np.asarray(w.parent), np.asarray(w.edge_r, np.float64), np.arange(w.M))
    rep = e.price_report()
    assert (rep.vset, rep.slot_hours, rep.scale) == (w.vset, 1.0, 1.0)
    check_report(rep, *feeder, g, y, cost, vset=w.vset)
    assert rep.day["n_cong_slots"] > 0 and rep.day["n_bad_slots"] == 0 and rep.slot["n_priced"].max() > 0
    print(f"rows with a multiplier: {int((np.abs(y).max(axis=1) > 0).sum())}; shares {rep.shares()}; top lines {rep.top_lines[:3]}")
    s = e.certificate().scale
    scaled = e.price_report(scale=s, with_loss=False, price_cap=float(cost.max()), slot_hours=0.5)
    check_report(scaled, *feeder, g, y, cost, scale=s, with_loss=False, price_cap=float(cost.max()), slot_hours=0.5, vset=w.vset)
    given = e.price_report(profile=w.load, multipliers=-y, nodes=np.arange(0, w.M, 2), arrays=False)
    assert given.price is None
    full = e.price_report(profile=w.load, multipliers=-y, nodes=np.arange(0, w.M, 2))
    check_report(full, *feeder, _node_sums(w, w.load.astype(np.float64)), -y, cost, nodes=np.arange(0, w.M, 2), vset=w.vset)
    assert all(given.__dict__[k].tobytes() == full.__dict__[k].tobytes() for k in RECORDS)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G, e.yd[0])))
    e.run_steps(2)


def test_engine_without_multipliers_reports_zero_congestion(gpu_lib):
    """The ADMM forms' path, and the dual Newton path when its last solve left no row with a multiplier: y = 0 and zero
    congestion -- the correct answer for a run whose rows do not bind."""
    from revs_admm_amd.engine import AdmmEngine, OperatorOptions
    from test_gpu_ensemble import _workload
    w = _workload(stress=0.9)
    for op in (None, OperatorOptions(solver="admm")):
        e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                       mode="pdhg", feeder=w.feeder, op=op)
        e.run(3)
        rep = e.price_report()
        priced = op is None and e._y_support and bool((e.yd[0] != 0).any())
        assert priced == bool((rep.cong != 0).any()) == (rep.day["n_cong_slots"] > 0)
        if not priced:
            assert (rep.rent == 0).all() and rep.day["cong_pay"] == 0 and rep.day["rent_total"] == 0
            assert rep.price.tobytes() == (w.cost.astype(np.float64)[None, :] + rep.lossp).tobytes()
        assert op is None or not priced
    with pytest.raises(ValueError, match="multipliers"):
        e.price_report(multipliers=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="multipliers"):
        e.price_report(multipliers="other")


def test_ensemble_price_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.price_reports()[s] holds the bytes of a single engine's report on scenario s under the ensemble's
    multipliers of that scenario, which are not all zero."""
    from revs_admm_amd.engine import AdmmEngine
    from test_gpu_ensemble import _ensemble, _mixed_scenarios
    w = _binding_workload()
    homes = _mixed_scenarios(w, 3)
    ens = _ensemble(w, homes, "relaxed_exact")
    ens.run(8)
    before = (ens.P_sch.clone(), ens.yd[0].clone())
    assert ens._y_support and max(np.abs(ens.multipliers(s)).max() for s in range(3)) > 0
    scales = np.array([1.0, 0.5, 2.0])
    nodes = np.arange(0, w.M, 3)
    reps = ens.price_reports(scale=scales, nodes=nodes, price_cap=0.2)
    assert ens.P_sch.cpu().numpy().tobytes() == before[0].cpu().numpy().tobytes()
    assert ens.yd[0].cpu().numpy().tobytes() == before[1].cpu().numpy().tobytes()
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="relaxed_exact", feeder=w.feeder)
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], w.load, w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.price_report(multipliers=ens.multipliers(s), scale=scales[s], nodes=nodes, price_cap=0.2)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert reps[s].scale == scales[s]
    given = ens.price_reports(multipliers=np.stack([ens.multipliers(s) for s in range(3)]), scale=scales, nodes=nodes,
                              price_cap=0.2)
    assert all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for a, b in zip(given, reps) for k in ARRAYS + RECORDS)


SHARD_CASE = dict(name="price", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports --
    of the schedule after 4 iterations under the operator's multipliers and of a given profile under given ones -- hold
    the one-rank bytes."""
    sys.path.insert(0, HERE)
    from network_worker import engine
    from prices_worker import reports
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_price"]).all() and np.abs(ref["prof_cong"]).max() > 0
    port = 29900 + (os.getpid() + 1291) % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "prices_worker.py"), str(path)], stdout=log,
                                       stderr=subprocess.STDOUT, env=env), log))
    rcs = []
    for p, log in procs:
        try:
            rcs.append(p.wait(timeout=600))
        except subprocess.TimeoutExpired:
            p.kill()
            rcs.append(-9)
        log.close()
    logs = "\n".join((tmp_path / f"w{r}.log").read_text()[-3000:] for r in range(2))
    assert rcs == [0, 0], logs
    for r in range(2):
        got = np.load(tmp_path / f"price_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


@pytest.mark.parametrize("path", ["upload", "device"])
def test_study_fills_prices(gpu_lib, golden, path, monkeypatch):
    """REVS.study(prices=...) on the 121144 feeder, on the upload path (distributed, uncontrolled) and on the ensemble's
    device path (distributed, individual): StudyReport.prices[s] holds the bytes of report_for_tree on the report's own
    row s under the study's tariff and the multipliers the study took from the operator (recorded here where it takes
    them) -- zero for the methods that have none; the default leaves it None."""
    import revs_admm_amd.prices as prices
    from test_gpu_losses import _study_inputs
    from revs_admm_amd.revs_fixture import REVS
    tariff, all_homes, dist, com, (parent, edge_r, cons_of) = _study_inputs(golden)
    taken = []
    take = prices.operator_multipliers

    def recording(*a):
        y = take(*a)
        taken.append(y.cpu().numpy().copy())
        return y

    monkeypatch.setattr(prices, "operator_multipliers", recording)
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234,), arrays=True, max_iterations=2, v0=1.03, mode="relaxed")
    if path == "upload":
        grid.update(methods=("distributed", "uncontrolled"))
        assert REVS().study(tariff, all_homes, dist, com, **dict(grid, methods=("uncontrolled",)))[1].prices is None
    else:
        grid.update(methods=("distributed", "individual"), ensemble=True, device_report=True)
    opts = dict(price_cap=0.2, scale=0.5) if path == "upload" else True
    labels, rep = REVS().study(tariff, all_homes, dist, com, prices=opts, **grid)
    assert len(rep.prices) == len(labels) == 2 and len(taken) == 1
    y = taken[0] if path == "upload" else taken[0][:, 0, :]
    assert y.shape == rep.node_p[0].shape
    print(f"{path}: rows with a multiplier after 2 iterations: {int((np.abs(y).max(axis=1) > 0).sum())}")
    for s, got in enumerate(rep.prices):
        ys = y if labels[s]["method"] == "distributed" else np.zeros_like(y)
        one = prices.report_for_tree(parent, edge_r, cons_of, rep.node_p[s], ys, cost=np.asarray(tariff, np.float64),
                                     **(opts if isinstance(opts, dict) else {}))
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert got.day["n_bad_slots"] == 0 and got.slot_hours == 1.0 and got.scale == (0.5 if path == "upload" else 1.0)
        assert labels[s]["method"] == "distributed" or (got.day["n_cong_slots"] == 0 and (got.rent == 0).all())
