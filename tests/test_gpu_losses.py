"""The loss report on the GPU (revs_net_losses; losses.report_for_tree, AdmmEngine.loss_report, AdmmEnsemble.loss_reports,
REVS.study(losses=), drawing.compute_losses) against tests/losses_ref.py.

Kernel against restatement: loss, every field of the slot records, line_day and day are bit for bit contract() fed the
kernel's own flow_out / drop_out (and, for mlf_max alone, its own mlf_out: mlf is a block scan whose bits depend on the
launch shape); the summaries by check_summary's rules (== for order statistics and counts, <= 2 ulp for the interpolated
quartiles).  Against definition() from the dense F and R P: loss within the bounds that 1e-12 x the largest entry
propagates (losses_ref.propagated_bounds), mlf within 2 n 2^-53 sum |c|, which holds for any order of its sum; the
measured maxima are printed beside the bounds.  Loads are scaled so that the deepest drop is 0.15 at vset = 1: no bad slot
except the two put in on purpose (a NaN injection; a slot scaled so that a drop exceeds vset^2)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import headroom_ref as hr
import losses_ref as lr
from test_gpu_network import BOUND, dense_of_forest, golden_net, synthetic_forest, ulps  # noqa: F401  (golden_net: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDS = ("summary", "slot", "line_day", "day")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def bits(got, want, what):
    """Equal as doubles including the NaNs' places, and equal in bytes where they are no NaNs."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and same(got, want), (what, got, want)
    ok = ~np.isnan(want)
    assert got[ok].tobytes() == want[ok].tobytes(), what


def check_report(rep, par, er, cons, p, lines=None, nodes=None, classes=None, cost=None, slot_hours=None,
                 loss_max=np.inf, vset=1.0, dense=None):
    """One scenario's LossReport against contract() on its own flow / drop, and against definition() where the dense
    (F, R P) in the caller's node order are given."""
    from revs_admm_amd.feeder import feeder_tree
    n, T = len(par), p.shape[1]
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    src = tree["src"]
    inj = np.where((src >= 0)[:, None], p[np.maximum(src, 0)], 0.0)

    def mask(sel):
        if sel is None:
            return None
        mk = np.zeros(n, bool)
        mk[np.asarray(sel, np.int64)] = True
        return hr.to_pos(tree, mk, False)

    cls, C = None, 0
    if classes is not None:
        cls, C = hr.to_pos(tree, np.where(np.asarray(classes) < 0, 255, classes), 255), int(np.max(classes)) + 1
    hours = 24.0 / T if slot_hours is None else slot_hours
    b = lr.contract(tree, n, hr.to_pos(tree, rep.flow), hr.to_pos(tree, rep.drop), inj, vset * vset, mask(lines), mask(nodes),
                    cls, C, loss_max, cost, hours, mlf=hr.to_pos(tree, rep.mlf))
    bad = b["bad"]
    bits(rep.loss, hr.to_nodes(tree, b["loss"], n), "loss")
    assert np.isnan(rep.mlf[:, bad]).all() and not np.isnan(rep.mlf[:, ~bad]).any()
    # ---- the slot records, every field
    for k in ("total", "delivered", "class_total", "mlf_max"):
        bits(rep.slot[k], b["slot"][k], k)
    assert same(rep.slot["mlf_max_index"], b["slot"]["mlf_max_index"]) and same(rep.slot["n_bad"], b["slot"]["n_bad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        bits(rep.loss_percent, 100.0 * b["slot"]["total"] / b["slot"]["delivered"], "loss_percent")
    # ---- the box-plot records
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
    # ---- the day records
    for k in ("energy", "peak"):
        bits(rep.line_day[k], b["line_day"][k], "line_day " + k)
    assert same(rep.line_day["peak_slot"], b["line_day"]["peak_slot"])
    for k in ("energy", "delivered", "class_energy", "cost", "peak", "top_energy"):
        bits(rep.day[k], b["day"][k], "day " + k)
    assert same(rep.day["top_index"], b["day"]["top_index"]), (rep.day["top_index"], b["day"]["top_index"])
    assert (rep.day["peak_slot"], rep.day["n_bad_slots"]) == (b["day"]["peak_slot"], b["day"]["n_bad_slots"])
    # ---- against the definition
    if dense is not None:
        good = ~bad
        F, RP = hr.to_pos(tree, dense[0][:, good]), hr.to_pos(tree, dense[1][:, good])
        eF, eV = BOUND * np.abs(F).max(), BOUND * np.abs(RP).max()
        assert np.abs(hr.to_pos(tree, rep.flow)[:, good] - F).max() <= eF
        assert np.abs(hr.to_pos(tree, rep.drop)[:, good] - RP).max() <= eV
        paths = lr.root_paths(lr.parent_positions(tree))
        d = lr.definition(tree["w"], F, RP, vset * vset, paths)
        b_loss, _, _ = lr.propagated_bounds(tree["w"], F, RP, vset * vset, paths, BOUND)
        b_mlf = 2.0 * tree["n"] * 2.0 ** -53 * np.abs(d["c"]).sum(axis=0)[None, :]
        e_loss = np.abs(b["loss"][:, good] - d["loss"])
        e_mlf = np.abs(hr.to_pos(tree, rep.mlf)[:, good] - d["mlf"])
        print(f"n={n}: loss err {e_loss.max():.3e} (largest err/bound {(e_loss / np.maximum(b_loss, 1e-300)).max():.3e}), "
              f"mlf err {e_mlf.max():.3e} (bound {b_mlf.min():.3e})")
        assert (e_loss <= b_loss).all() and (e_mlf <= b_mlf).all()
    return b


def run(par, er, cons, p, dense=None, **kw):
    from revs_admm_amd.losses import report_for_tree
    rep = report_for_tree(par, er, cons, p, **kw)
    check_report(rep, par, er, cons, p, dense=dense, **kw)
    return rep


@functools.lru_cache(maxsize=None)
def forest_case(M):
    """A forest of M nodes, every node a row, three slots of loads (a tenth of them exporting) scaled so that the
    deepest drop is 0.15, with its dense reference (F, R P) -- computed once per size and shared by the cases (the
    factorisation of the 16 384-node matrix takes some twenty seconds, as in test_gpu_network.py)."""
    rng = np.random.default_rng(M)
    par, er, cons = synthetic_forest(M, M)
    er[rng.random(M) < 0.05] = 0.0
    p = rng.uniform(0.0, 4.0, (M, 3)) * np.where(rng.random((M, 1)) < 0.1, -0.5, 1.0)
    F, RP = dense_of_forest(par, er, p)
    s = 0.15 / np.abs(RP).max()
    return par, er, cons, p * s, F * s, RP * s


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("M", [8, 2048, 4096, 8192, 8200, 16384])
def test_every_tree_shape_matches_the_restatements(gpu_lib, M, T):
    """One thread (8), 256 x 8, 512 x 8, 1024 x 8, the first 1024 x 16 size (8200 pads to 8208) and the largest, with a
    line mask, a node mask, three classes, a finite loss_max and a tariff.  T = 3 carries the two bad slots: slot 1 a NaN
    injection, slot 2 the loads scaled to a deepest drop of 1.2 > vset^2."""
    from revs_admm_amd.network import report_for_tree as net_report
    par, er, cons, p, F, RP = forest_case(M)
    p, F, RP = p[:, :T].copy(), F[:, :T].copy(), RP[:, :T].copy()
    if T == 3:
        p[M // 3, 1] = np.nan
        p[:, 2] *= 1.2 / np.abs(RP[:, 2]).max()
    rng = np.random.default_rng(M + T)
    lines, nodes = np.flatnonzero(rng.random(M) < 0.7), np.flatnonzero(rng.random(M) < 0.6)
    classes = rng.integers(-1, 3, M)
    classes[0] = 2
    good = np.abs(0.5 * 2 * er[:, None] * F[:, :1] ** 2)
    rep = run(par, er, cons, p, dense=(F, RP), lines=lines, nodes=nodes, classes=classes, cost=rng.uniform(0.05, 0.3, T),
              slot_hours=0.25, loss_max=float(np.quantile(good, 0.9)) if M > 8 else 1e-3)
    assert rep.slot["n_bad"].tolist() == ([0] if T == 1 else [0, 1, 1])
    assert rep.slot["total"][0] > 0 and rep.summary["count"][0] == len(lines) and (M == 8 or rep.summary["n_violations"][0] > 0)
    if T == 1:
        assert net_report(par, er, cons, p).flow.tobytes() == rep.flow.tobytes()


def test_chain_of_depth_2048(gpu_lib):
    """One lateral of 2048 nodes: every root path is a prefix, mlf grows along it."""
    n = 2048
    rng = np.random.default_rng(4)
    par, er, cons = np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n)
    p = rng.uniform(0.0, 1.0, (n, 2))
    F, RP = dense_of_forest(par, er, p)
    s = 0.15 / np.abs(RP).max()
    rep = run(par, er, cons, p * s, dense=(F * s, RP * s))
    assert (np.diff(rep.mlf[:, 0]) >= 0).all() and rep.slot["mlf_max_index"].tolist() == [n - 1, n - 1]


@pytest.mark.parametrize("tag", ["dis_a90_r4800", "ind_a90_r4800", "LOAD"])
def test_stored_results_of_the_reference(gpu_lib, golden, golden_net, tag):
    """The 121144 feeder, T = 24, under the stored distributed and individual schedules and the base load alone, with
    the stored tariff: equal to the restatements.  (Which schedule loses less is not asserted.)"""
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    p = np.asarray(z["LOAD"] if tag == "LOAD" else z[tag + "_P_res"], np.float64)
    P = np.zeros((gn["n"], 24))
    P[gn["rows"]] = p
    dense = (gn["to_node"](gn["A_inv"] @ P), gn["R"] @ P)
    rep = run(par, er, cons, p, dense=dense, cost=np.asarray(z["tariff_shift6"], np.float64), slot_hours=1.0)
    assert rep.slot["n_bad"].sum() == 0 and rep.day["n_bad_slots"] == 0 and (rep.day["top_index"] >= 0).all()
    print(f"{tag}: day loss {rep.day['energy']:.1f}, {rep.day_loss_percent:.2f} % of delivered, peak slot {rep.day['peak_slot']}")
    assert 0.0 < rep.day_loss_percent < 5.0


def small_case(M=300, T=5, seed=300):
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed)
    p = rng.uniform(-0.3, 4.0, (M, T))
    F, RP = dense_of_forest(par, er, p)
    s = 0.15 / np.abs(RP).max()
    return par, er, cons, p * s, F * s, RP * s, rng


@pytest.mark.parametrize("C", [0, 3])
def test_scenario_grid_equals_single_calls(gpu_lib, C):
    """S = 3 x T = 5 on 300 nodes, masks, classes (or none), a tariff (or none): every scenario against the
    restatements, its slice equal in bytes to the S = 1 call on that scenario."""
    from revs_admm_amd.losses import report_for_tree
    par, er, cons, p, F, RP, rng = small_case()
    f = rng.uniform(0.5, 1.0, p.shape[1])
    ps = np.stack([p, p * f, p[::-1].copy()])
    loss_max = float(np.quantile(er[:, None] * F * F, 0.9))       # (r F^2: about a tenth of the lines lose more)
    kw = dict(lines=np.flatnonzero(rng.random(300) < 0.6), nodes=np.flatnonzero(rng.random(300) < 0.5), loss_max=loss_max,
              classes=rng.integers(0, 3, 300) if C else None, cost=rng.uniform(0.1, 0.3, 5) if C else None)
    reps = report_for_tree(par, er, cons, ps, **kw)
    assert len(reps) == 3
    dense = [(F, RP), (F * f, RP * f), None]
    for s, rep in enumerate(reps):
        check_report(rep, par, er, cons, ps[s], dense=dense[s], **kw)
        one = report_for_tree(par, er, cons, ps[s], **kw)
        for k in ("loss", "mlf", "drop", "flow") + RECORDS:
            assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (s, k)
    assert np.isnan(reps[0].day["cost"]) == (C == 0) and (reps[0].slot["class_total"][:, C:] == 0).all()
    assert reps[0].summary["n_violations"].max() > 0 and len(reps[0].top_lines) == 8


def test_ties_and_fewer_than_eight_lines(gpu_lib):
    """Twelve equal laterals of one line each: every loss ties -- worst_index 0, the top 8 are lines 0..7 in order.  Two
    equal laterals of two lines below a shared root, five lines in all: the top 8 end in -1 / NaN."""
    rep = run(np.full(12, -1), np.full(12, 0.5), np.arange(12), np.full((12, 2), 0.25))
    assert (rep.summary["worst_index"] == 0).all() and rep.day["top_index"].tolist() == list(range(8))
    assert len(set(rep.loss.ravel().tolist())) == 1 and (rep.summary["n_fliers"] == 0).all()
    rep = run(np.full(12, -1), np.full(12, 0.5), np.arange(12), np.full((12, 2), 0.25), lines=[11, 3, 5])
    assert (rep.summary["worst_index"] == 3).all() and rep.day["top_index"].tolist() == [3, 5, 11, -1, -1, -1, -1, -1]
    par = np.array([-1, 0, 1, 0, 3])
    rep = run(par, np.array([0.25, 0.5, 0.5, 0.5, 0.5]), np.arange(5), np.array([[0.0], [0.03125], [0.0625], [0.03125], [0.0625]]))
    assert rep.day["top_index"].tolist() == [0, 1, 3, 2, 4, -1, -1, -1] and np.isnan(rep.day["top_energy"][5:]).all()
    assert rep.loss[1, 0] == rep.loss[3, 0] and rep.loss[2, 0] == rep.loss[4, 0] and rep.slot["mlf_max_index"][0] == 2


def test_every_output_alone_and_records_only(gpu_lib):
    """Each output with every other one NULL holds the bytes of the full call (the arrays without any scratch);
    arrays=False gives the same records."""
    import ctypes as C
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.losses import _position_bytes, _position_classes, report_for_tree
    from revs_admm_amd.network import SUMMARY_DTYPE, side_arrays, tree_on_device
    par, er, cons, p, F, RP, rng = small_case(300, 4, 12)
    p[7, 2] = np.inf                                              # (a bad slot among them)
    lines, classes, cost = np.flatnonzero(rng.random(300) < 0.6), rng.integers(0, 2, 300), rng.uniform(0.1, 0.3, 4)
    kw = dict(lines=lines, classes=classes, cost=cost, loss_max=1e-4, slot_hours=0.5)
    full = report_for_tree(par, er, cons, p, **kw)
    only = report_for_tree(par, er, cons, p, arrays=False, **kw)
    assert only.loss is None and only.mlf is None and only.flow is None
    for k in RECORDS:
        assert getattr(only, k).tobytes() == getattr(full, k).tobytes(), k
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    d_nop, _, _ = side_arrays(dev, th, 300, None, None)
    d_lm = _position_bytes(dev, th, 300, lines, "lines")
    d_cls, n_cls = _position_classes(dev, th, 300, classes)
    g, d_cost = torch.from_numpy(p).to(dev), torch.from_numpy(cost).to(dev)
    scratch = torch.empty(lib.revs_net_losses_scratch(1, 4, th["n"]) // 8, dtype=torch.float64, device=dev)
    wants = [full.loss, full.mlf, full.drop, full.flow, full.summary, full.slot, full.line_day, full.day]
    sizes = [300 * 4 * 8] * 4 + [4 * SUMMARY_DTYPE.itemsize, 4 * 64, 300 * 24, 192]
    for k in range(8):
        outs = [None] * 8
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = lib.revs_net_losses(1, 300, 4, C.byref(tree), g.data_ptr(), d_lm.data_ptr(), None, d_cls.data_ptr(), n_cls,
                                 d_nop.data_ptr(), 300, 1.0, 0.5, 1e-4, d_cost.data_ptr(),
                                 *[None if o is None else o.data_ptr() for o in outs],
                                 scratch.data_ptr() if k in (4, 6, 7) else None, None)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k
    assert _lib.LOSS_SLOT_DTYPE.itemsize == 64


def _small_workload():
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(2000, 24, n_nodes=64, seed=3, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    return w


def test_engine_loss_report(gpu_lib):
    """After a short streaming run: loss_report() of the schedule, of a rule schedule and of the base load against the
    restatements; the tariff defaults to the engine's own, slot_hours to 24 / T; the run's state keeps its bytes."""
    from revs_admm_amd.engine import AdmmEngine
    w = _small_workload()
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run(3)
    e.run_steps(10)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    cost = w.cost.astype(np.float64)
    rep = e.loss_report()
    assert (rep.vset, rep.slot_hours) == (w.vset, 1.0)
    g = np.zeros((w.M, 24))
    np.add.at(g, w.node_of, w.load.astype(np.float64) + e.result()[0].astype(np.float64))
    F, RP = dense_of_forest(np.asarray(w.parent), np.asarray(w.edge_r, np.float64), g)
    check_report(rep, w.parent, w.edge_r, np.arange(w.M), g, cost=cost, vset=w.vset, dense=(F, RP))
    prof = e.rule_schedule("uncontrolled")
    rule = e.loss_report(profile=prof, loss_max=0.5, slot_hours=0.5)
    prof_h = (prof if isinstance(prof, np.ndarray) else prof.cpu().numpy()[e.inv_perm]).astype(np.float64)
    g2 = np.zeros((w.M, 24))
    np.add.at(g2, w.node_of, prof_h)
    check_report(rule, w.parent, w.edge_r, np.arange(w.M), g2, cost=cost, vset=w.vset, loss_max=0.5, slot_hours=0.5)
    base = e.loss_report(profile=w.load, arrays=False)
    assert base.loss is None and base.day["energy"] > 0 and base.day["energy"] != rep.day["energy"]
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    e.run_steps(2)


def test_ensemble_loss_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.loss_reports()[s] holds the bytes of a single engine's report on scenario s; the loss tensor can stay
    on the device."""
    import torch
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    classes = np.random.default_rng(6).integers(0, 4, w.M)
    out = torch.zeros(3, w.M, 24, dtype=torch.float64, device=ens.dev)
    reps = ens.loss_reports(classes=classes, loss_max=0.01, out=out)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.loss_report(profile=e.P_sch, classes=classes, loss_max=0.01)
        for k in ("loss", "mlf", "drop", "flow") + RECORDS:
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert out[s].cpu().numpy().tobytes() == one.loss.tobytes()
        assert np.isfinite(one.day["cost"]) and (one.day["class_energy"] > 0).all()


SHARD_CASE = dict(name="loss", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports --
    of the schedule after 4 iterations and of a given profile -- hold the one-rank bytes."""
    sys.path.insert(0, HERE)
    from losses_worker import reports
    from network_worker import engine
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_loss"]).all()
    port = 29900 + (os.getpid() + 977) % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "losses_worker.py"), str(path)], stdout=log,
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
        got = np.load(tmp_path / f"loss_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


def _study_inputs(golden):
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.lpsolver import feeder_of
    z = golden[0]
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    return f32(z["tariff_shift6"]), all_homes, dist, com, feeder_of(dist)[1]


@pytest.mark.parametrize("path", ["upload", "device"])
def test_study_fills_losses(gpu_lib, golden, path):
    """REVS.study(losses=...) on the 121144 feeder, on the upload path (individual, uncontrolled) and on the ensemble's
    device path (distributed, individual): StudyReport.losses[s] holds the bytes of report_for_tree on the report's own
    row s under the study's tariff; the default leaves it None."""
    from revs_admm_amd.losses import report_for_tree
    from revs_admm_amd.revs_fixture import REVS
    tariff, all_homes, dist, com, (parent, edge_r, cons_of) = _study_inputs(golden)
    if path == "upload":
        grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), methods=("individual", "uncontrolled"), arrays=True)
        assert REVS().study(tariff, all_homes, dist, com, **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].losses is None
    else:
        grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234,), methods=("distributed", "individual"), arrays=True,
                    ensemble=True, device_report=True, max_iterations=2, v0=1.03, mode="relaxed")
    labels, rep = REVS().study(tariff, all_homes, dist, com, losses=dict(loss_max=0.05) if path == "upload" else True, **grid)
    assert len(rep.losses) == len(labels) == (4 if path == "upload" else 2)
    for s, got in enumerate(rep.losses):
        one = report_for_tree(parent, edge_r, cons_of, rep.node_p[s], cost=np.asarray(tariff, np.float64),
                              loss_max=0.05 if path == "upload" else np.inf)
        for k in ("loss", "mlf") + RECORDS:
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert got.day["n_bad_slots"] == 0 and np.isfinite(got.day["cost"]) and got.slot_hours == 1.0


def test_compute_losses_on_the_golden_graph(gpu_lib, golden, golden_net):
    """drawing.compute_losses: {edge: kW per slot} in graph.edges order, the report's loss of the tree node below each
    edge; the edges' sum is the slot total up to the order of the sum."""
    from test_network_host import golden_graph
    from revs_admm_amd.drawing import compute_losses
    from revs_admm_amd.losses import report_for_tree
    z, gn = golden[0], golden_net
    dist = golden_graph(golden)
    p_sch = {int(h): row.tolist() for h, row in zip(z["res_id"], np.asarray(z["dis_a90_r4800_P_res"], np.float64))}
    out = compute_losses(dist, p_sch, vset=1.0)
    assert list(out) == list(dist.edges) and all(len(v) == 24 for v in out.values())
    par, er, cons = gn["feeder"]
    rep = report_for_tree(par, er, cons, np.asarray(z["dis_a90_r4800_P_res"], np.float64))
    got = np.array(list(out.values()))
    assert np.sort(got, axis=0).tobytes() == np.sort(rep.loss, axis=0).tobytes()
    assert np.allclose(got.sum(axis=0), rep.slot["total"], rtol=1e-12, atol=0.0)
