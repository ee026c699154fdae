"""The convergence report on the GPU (csrc/convergence_kernels.hip, revs_admm_amd/convergence.py, DESIGN.md section
3.11): every record of revs_conv_report, through the C ABI and through the Python entries, against the numpy yard-stick
(tests/conv_ref.py) at the smallest shapes at which the mapping can go wrong, and end to end from the histories that
run(history="device") leaves on the device."""
import numpy as np
import pytest

import conv_ref as cr

pytestmark = pytest.mark.gpu

F32 = np.float32


class Rep:
    """What revs_conv_report wrote, as numpy arrays (None: that output was NULL)."""


def native(lib, hist, eps, patience=8, keep=None, index=None, groups=None, pad=0, res=True, run=True, settle=True):
    """hist (S, K, n) float32 on the host -> Rep through the C ABI.  pad: extra elements per row (a sliced tensor),
    filled with a value no record may see."""
    import torch
    from revs_admm_amd._lib import BILL_DTYPE, CONV_RES_DTYPE, CONV_RUN_DTYPE, check, ptr
    S, K, n = hist.shape
    dev = torch.device("cuda:0")
    wide = np.full((K, n * S + pad), 7e9, F32)
    wide[:, :n * S] = hist.transpose(1, 2, 0).reshape(K, n * S)
    d_hist = torch.from_numpy(wide).to(dev)
    d_keep = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)
    d_index = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
    G = 0 if groups is None else int(max(groups)) + 1
    hg = None if groups is None else np.ascontiguousarray(groups, np.int32)
    junk = lambda nbytes: torch.full((max(nbytes, 1),), 0xCD, dtype=torch.uint8, device=dev)
    rec = BILL_DTYPE.itemsize
    d_iter, d_pool = junk(S * K * rec), junk(G * K * rec) if G else None
    d_res = junk(S * n * CONV_RES_DTYPE.itemsize) if res else None
    d_run = junk(S * CONV_RUN_DTYPE.itemsize) if run else None
    d_settle = junk(S * rec) if settle else None
    nbytes = int(lib.revs_conv_report_scratch(S, n, K, G))
    assert nbytes > 0
    d_scratch = torch.full((nbytes // 8 + 1,), -1.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib.revs_conv_report(S, n, K, ptr(d_hist), n * S + pad, ptr(d_keep), ptr(d_index),
                               hg.ctypes.data if G else None, G, float(eps), patience, ptr(d_iter), ptr(d_pool), ptr(d_res),
                               ptr(d_run), ptr(d_settle), ptr(d_scratch), st), "revs_conv_report")
    out = Rep()
    out.iterations = d_iter.cpu().numpy()[:S * K * rec].view(BILL_DTYPE).reshape(S, K)
    out.pooled = d_pool.cpu().numpy()[:G * K * rec].view(BILL_DTYPE).reshape(G, K) if G else np.zeros((0, K), BILL_DTYPE)
    out.residences = d_res.cpu().numpy().view(CONV_RES_DTYPE).reshape(S, n) if res else None
    out.run = d_run.cpu().numpy().view(CONV_RUN_DTYPE).reshape(S) if run else None
    out.settle = d_settle.cpu().numpy().view(BILL_DTYPE).reshape(S) if settle else None
    return out


def history(S, K, n, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "mixed":                            # 90 % exact zeros among random positives
        h = rng.uniform(0.0, 2.0, (S, K, n)) * (rng.random((S, K, n)) < 0.1)
    elif kind == "dense":
        h = rng.lognormal(-3.0, 2.0, (S, K, n))
    elif kind == "equal":
        h = np.full((S, K, n), 0.37)
    elif kind == "zero":
        h = np.zeros((S, K, n))
    elif kind == "two":
        h = np.where(rng.random((S, K, n)) < 0.6, 0.25, 1.5)
    elif kind == "awkward":
        # -0.0, denormals, infinities, a negative, and values that share the upper three bytes of their keys
        close = (0.5 + np.arange(256) * 2.0 ** -24).astype(F32)
        assert len(set((close.view(np.uint32) >> 8).tolist())) == 1 and len(set(close.tolist())) == 256
        pool = np.concatenate([close[rng.integers(0, 256, 40)], F32([-0.0, 0.0, 1e-45, 1e-40, -1e-42, np.inf, -np.inf,
                                                                        -1.5, 0.5, 0.5, 3e38])])
        h = pool[rng.integers(0, len(pool), (S, K, n))]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(h, F32)


SIZES = [(1, 1, 1, "dense"), (63, 2, 3, "mixed"), (64, 15, 1, "mixed"), (65, 40, 5, "mixed"), (257, 15, 3, "dense"),
         (1000, 2, 5, "awkward"), (1000, 40, 1, "mixed"), (65, 2, 11, "dense"), (3, 2, 1030, "mixed")]


@pytest.mark.parametrize("n,K,S,kind", SIZES)
def test_records_at_every_shape(gpu_lib, n, K, S, kind):
    h = history(S, K, n, kind, seed=n + K + S)
    groups = None
    if S == 3:
        groups = [0, -1, 0]
    elif S == 5:
        groups = [1, 0, 1, -1, 1]
    elif S == 11:
        groups = [0, 1, 2, 3, 4, 5, 5, -1, 2, 0, 0]           # more groups than one pool launch holds
    elif S == 1030:
        groups = [0] * S                                      # more columns than the workgroup has threads
    eps = 0.5 if kind == "awkward" else float(np.median(h[h > 0])) if (h > 0).any() else 0.0
    assert kind != "awkward" or (h == F32(0.5)).any()          # (eps equal to a value that is there: `>` is strict)
    for pad in (0, 5):
        rep = native(gpu_lib, h, eps, patience=2, groups=groups, pad=pad)
        cr.check_report(rep, h, eps, 2, groups=groups, what=(n, K, S, kind, pad))


@pytest.mark.parametrize("kind", ["equal", "zero", "two", "mixed", "awkward"])
def test_ties_and_awkward_values(gpu_lib, kind):
    h = history(3, 4, 257, kind, seed=3)
    for eps in (0.0, 0.37, 0.25):
        rep = native(gpu_lib, h, eps, patience=1, groups=[0, 0, 1])
        cr.check_report(rep, h, eps, 1, groups=[0, 0, 1], what=(kind, eps))


def test_nan_keep_and_index(gpu_lib):
    S, K, n = 3, 6, 130
    h = history(S, K, n, "mixed", seed=8)
    rng = np.random.default_rng(9)
    h[rng.random(h.shape) < 0.05] = np.nan                   # scattered
    h[1, 2, :] = np.nan                                       # a whole row of a scenario
    h[:, 4, :] = np.nan                                       # a row of the history
    h[0, 5, :7] = 5.0                                         # a tie for the largest value
    keep = rng.random((S, n)) < 0.7
    keep[2] = False                                           # a scenario with nothing kept
    index = rng.permutation(n)
    groups = [0, 0, 1]
    rep = native(gpu_lib, h, 0.3, patience=1, keep=keep, index=index, groups=groups)
    cr.check_report(rep, h, 0.3, 1, keep=keep, index=index, groups=groups, what="nan/keep/index")
    # the tie goes to the lowest caller-side index among the kept
    tied = [i for i in range(7) if keep[0, i]]
    assert tied and int(rep.iterations[0, 5]["worst_index"]) == min(index[i] for i in tied)
    assert (rep.iterations[2]["count"] == 0).all() and (rep.iterations[2]["worst_index"] == -1).all()
    assert int(rep.settle[2]["count"]) == 0 and np.isnan(rep.settle[2]["median"])
    assert (rep.iterations[:, 4]["count"] == 0).all() and (rep.iterations[:2, 4]["n_nan"] == keep[:2].sum(1)).all()
    assert int(rep.pooled[1, 0]["count"]) == 0 and int(rep.pooled[1, 0]["worst_scenario"]) == -1
    # a NaN row is above eps for every residence: nobody has settled before it
    assert (rep.residences["settle"] >= 5).all()
    # without an index the rows are their own
    rep0 = native(gpu_lib, h, 0.3, patience=1, keep=keep, groups=groups)
    cr.check_report(rep0, h, 0.3, 1, keep=keep, groups=groups, what="nan/keep")


def _rows_with_maxima(maxima, n=5):
    """(1, K, n): row k holds maxima[k] once and smaller values."""
    h = np.zeros((1, len(maxima), n), F32)
    for k, m in enumerate(maxima):
        h[0, k, (3 * k) % n] = m
        h[0, k, (3 * k + 1) % n] = 0.5 * m
    return h


def test_patience(gpu_lib):
    lo, hi = 0.1, 0.9
    cases = [
        ([lo] * 10, {1: 0, 8: 0, 10: 0, 11: -1}),                               # from the first row on
        ([hi, hi] + [lo] * 8, {1: 2, 8: 2, 9: -1}),                             # the last possible row
        ([hi] + [lo] * 7 + [hi] + [lo], {1: 1, 7: 1, 8: -1}),                   # broken one row short
        ([lo, hi, lo, lo, hi, lo, lo, lo, hi, lo], {1: 0, 2: 2, 3: 5, 4: -1}),
        ([hi] * 10, {1: -1, 8: -1}),
        ([0.5] * 3, {1: 0, 3: 0, 4: -1}),                                       # eps itself is within
    ]
    for maxima, want in cases:
        h = _rows_with_maxima(maxima)
        for patience, at in want.items():
            rep = native(gpu_lib, h, 0.5, patience=patience)
            assert int(rep.run[0]["converged_at"]) == at, (maxima, patience, rep.run)
            cr.check_report(rep, h, 0.5, patience, what=("patience", maxima, patience))
    # more rows than the final workgroup has threads: stretches that cross its threads' pieces
    rng = np.random.default_rng(2)
    maxima = np.where(rng.random(700) < 0.1, hi, lo).tolist()
    h = _rows_with_maxima(maxima, n=2)
    for patience in (1, 8, 40, 50, 701):
        rep = native(gpu_lib, h, 0.5, patience=patience, res=True)
        want = cr.run_record(maxima, 0.5, patience)
        assert (int(rep.run[0]["converged_at"]), int(rep.run[0]["last_above"])) == (want["converged_at"], want["last_above"])
    assert [cr.run_record(maxima, 0.5, p)["converged_at"] for p in (1, 8, 40, 50, 701)] == [0, 8, 8, 615, -1]


def test_pools_and_repeatability(gpu_lib):
    S, K, n = 5, 7, 300
    h = history(S, K, n, "mixed", seed=21)
    h[3] = history(1, K, n, "dense", seed=22)[0]
    keep = np.random.default_rng(23).random((S, n)) < 0.8
    groups = [0, 1, 0, 2, -1]                                 # several members, one member (twice), in no group
    a = native(gpu_lib, h, 0.2, keep=keep, groups=groups)
    b = native(gpu_lib, h, 0.2, keep=keep, groups=groups, pad=3)
    cr.check_report(a, h, 0.2, 8, keep=keep, groups=groups, what="pools")
    for k in ("iterations", "pooled", "residences", "run", "settle"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k          # two calls, the same bytes
    # a pool of one scenario repeats that scenario's record byte for byte, total included
    assert a.pooled[1].tobytes() == a.iterations[1].tobytes() and a.pooled[2].tobytes() == a.iterations[3].tobytes()
    assert a.pooled[0].tobytes() != a.iterations[0].tobytes()
    assert (a.pooled[0]["count"] == a.iterations[0]["count"] + a.iterations[2]["count"]).all()


def test_null_outputs(gpu_lib):
    S, K, n = 3, 9, 140
    h = history(S, K, n, "mixed", seed=31)
    groups = [0, 0, 1]
    full = native(gpu_lib, h, 0.4, groups=groups)
    for res, run, settle in ((False, True, True), (True, False, True), (True, True, False), (False, False, False),
                             (False, True, False), (False, False, True)):
        part = native(gpu_lib, h, 0.4, groups=groups, res=res, run=run, settle=settle)
        assert part.iterations.tobytes() == full.iterations.tobytes() and part.pooled.tobytes() == full.pooled.tobytes()
        if res:
            assert part.residences.tobytes() == full.residences.tobytes()
        if settle:
            assert part.settle.tobytes() == full.settle.tobytes()
        if run and res:
            assert part.run.tobytes() == full.run.tobytes()
        if run and not res:                                   # the two counts need the per-residence walk's output
            for k in ("converged_at", "last_above"):
                assert part.run[k].tolist() == full.run[k].tolist()
            assert (part.run["n_unsettled"] == -1).all() and (part.run["n_never"] == -1).all()


def test_reference_trajectory_through_the_python_entries(gpu_lib, golden):
    import torch
    from revs_admm_amd import convergence
    from test_conv_host import golden_history
    h = golden_history(golden[0])                             # (1, 15, 267)
    rep = convergence.convergence_report(h[0], 0.5)
    cr.check_report(rep, h, 0.5, 8, what="golden")
    assert rep.run[0].tolist() == (-1, 12, 0, 111) and rep.iterations[0]["n_above"][:4].tolist() == [156, 4, 33, 33]
    assert rep.iterations[0]["worst_index"][[0, 1, 14]].tolist() == [112, 179, 223]
    assert (rep.settle[0]["count"], rep.settle[0]["total"], rep.settle[0]["worst_index"]) == (267, 302.0, 6)
    assert rep.pooled.shape == (0, 15) and rep.n_groups == 0 and rep.keep is None
    assert convergence.convergence_report(h[0], 0.5, patience=2).run[0]["converged_at"] == 13
    # the device entry on a slice of a wider tensor, three copies as three scenarios, a keep mask, records only
    wide = torch.zeros(15, 267 * 3 + 9, device="cuda:0")
    wide[:, :267 * 3] = torch.from_numpy(np.repeat(h[0], 3, axis=1)).to("cuda:0")
    keep = np.ones((3, 267), bool)
    keep[1, ::2] = False
    r3 = convergence.convergence_report_device(wide[:, :267 * 3], 0.5, S=3, keep=keep, groups=[0, 1, 0], arrays=False)
    h3 = np.repeat(h, 3, axis=0)
    cr.check_report(r3, h3, 0.5, 8, keep=keep, groups=[0, 1, 0], what="golden x 3")
    assert r3.residences is None
    for k in ("median", "max", "n_above", "worst_index", "n_fliers"):          # (scenario 0 keeps everybody)
        assert r3.iterations[0][k].tobytes() == rep.iterations[0][k].tobytes(), k
    assert (r3.run["n_unsettled"] == -1).all() and r3.keep.tobytes() == keep.tobytes()
    with pytest.raises(ValueError, match="negative or a NaN"):
        convergence.convergence_report_device(wide[:, :801], -0.5, S=3)


def _single(seed=4, n=300):
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(n, 24, n_nodes=30, seed=seed, stress=1.02)
    w.load, w.cost = f32(w.load), f32(w.cost)
    shuffle = np.random.default_rng(seed).permutation(n)      # (the sweep order is then not the caller's)
    w.node_of, w.load, w.homes = w.node_of[shuffle], w.load[shuffle], w.homes[shuffle]
    return w, lambda: AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow,
                                 vhigh=w.vhigh, mode="relaxed", feeder=w.feeder)


def test_engine_end_to_end(gpu_lib):
    w, make = _single()
    e, f = make(), make()
    with pytest.raises(ValueError, match="no history on the device"):
        e.convergence_report(1e-3)
    assert e.run(iter_max=40, history="device") == 40
    assert e.diff_history.is_cuda and tuple(e.diff_history.shape) == (40, 300)
    d = f.run(iter_max=40, history=True)
    assert d.shape == (40, 300) and d.dtype == np.float32
    assert e.diff_history.cpu().numpy()[:, e.inv_perm].tobytes() == d.tobytes()
    mx = d.max(axis=1)
    eps = float(np.sort(mx)[len(mx) // 3])
    ev = w.homes["ev"] != 0
    for keep in (None, ev):
        rep = e.convergence_report(eps, patience=3, keep=keep)
        cr.check_report(rep, d[None], eps, 3, keep=None if keep is None else keep[None], what="engine")
    assert rep.keep.tobytes() == ev[None].tobytes() and rep.residences.shape == (1, 300)
    assert (rep.residences["last"][0] == d[-1]).all()         # the caller's order
    # a run that stops on eps: the history's verdict is the engine's
    tail = float(mx[25:].max())
    g = make()
    it0 = g.iteration
    k = g.run(iter_max=200, eps=tail, patience=3, history="device")
    assert g.converged_at is not None and k < 200 and tuple(g.diff_history.shape) == (k, 300)
    r = g.convergence_report(tail, patience=3, arrays=False)
    print(f"run(eps={tail:.3e}) stopped after {k} iterations, converged_at {g.converged_at}; the report's row "
          f"{int(r.run['converged_at'][0])}, last_above {int(r.run['last_above'][0])}")
    assert int(r.run["converged_at"][0]) + it0 + 1 == g.converged_at
    # the folded maxima the run judged are the history rows' maxima
    for it, v in g.max_diff.items():
        if it0 < it <= it0 + k:
            assert v == float(r.iterations[0, it - it0 - 1]["max"]), (it, v)


def test_ensemble_end_to_end(gpu_lib):
    from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
    w = _workload()
    homes = _mixed_scenarios(w, 3)
    e, f = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    with pytest.raises(ValueError, match='True or "device"'):
        e.run(3, history=False)
    assert e.run(8, history="device") == 8 and tuple(e.diff_history.shape) == (8, 600 * 3)
    d = f.run(8)
    assert d.shape == (3, 8, 600)
    got = e.diff_history.view(8, 600, 3).permute(2, 0, 1).cpu().numpy()[:, :, e.inv_perm]
    assert got.tobytes() == d.tobytes()
    eps = float(np.median(d.max(axis=2)))
    ev = np.stack([h["ev"] != 0 for h in homes])
    groups = [0, -1, 0]
    rep = e.convergence_report(eps, patience=2, groups=groups, keep=ev)
    cr.check_report(rep, d, eps, 2, keep=ev, groups=groups, what="ensemble")
    assert rep.keep.tobytes() == ev.tobytes() and rep.n_groups == 1 and rep.groups.tolist() == groups
    every = e.convergence_report(eps, patience=2, arrays=False)
    assert every.residences is None and (every.iterations["count"] == 600).all()


def test_solve_many_with_convergence(gpu_lib):
    """Six scenarios at T = 192: two ensembles, one report over both, pooled across them."""
    from test_gpu_ensemble_report import _small_graph
    from revs_admm_amd.extract import get_homes_ev_param
    from revs_admm_amd.lpsolver import solve_ADMM_many
    T = 192
    g = _small_graph()
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    rng = np.random.default_rng(4)
    base = {h: rng.uniform(0.2, 1.5, T).astype(F32).astype(np.float64).tolist() for h in res}
    tariff = (0.1 + 0.05 * np.sin(np.arange(T) / T * 2 * np.pi)).astype(F32).astype(np.float64).tolist()
    scen = [get_homes_ev_param(base, g, rng.choice(res, 8 + 4 * s, replace=False), (3.6, 4.8, 7.2)[s % 3], 160.0, 0.2,
                               88, 184) for s in range(6)]
    groups = [0, 1, 0, 1, -1, 0]
    out, rep = solve_ADMM_many(scen, g, tariff, None, kappa=5.0, iter_max=3, vset=1.03, vlow=0.95, vhigh=1.05,
                               mode="relaxed", return_convergence=0.05, convergence_groups=groups, convergence_patience=1)
    assert len(out) == 6 and rep.iterations.shape == (6, 3) and rep.pooled.shape == (2, 3)
    d = np.array([[[sol[0][k + 1][h] for h in res] for k in range(3)] for sol in out], F32)
    cr.check_report(rep, d, 0.05, 1, groups=groups, what="solve_ADMM_many")
    plain = solve_ADMM_many(scen[:2], g, tariff, None, kappa=5.0, iter_max=3, vset=1.03, vlow=0.95, vhigh=1.05,
                            mode="relaxed")
    assert isinstance(plain, list) and len(plain) == 2
    empty = solve_ADMM_many([], g, tariff, return_convergence=0.05)
    assert empty == ([], None)


def test_study_with_convergence(gpu_lib, golden):
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    labels, rep = REVS().study(tariff, all_homes, dist, com, adoptions=(90,), ratings=(4800,), seeds=(1234, 56),
                               group_by="method", max_iterations=3, v0=1.03, mode="relaxed", ensemble=True,
                               convergence=0.5, patience=1)
    c = rep.convergence
    n = len(z["res_id"])
    assert [l["method"] for l in labels] == ["distributed", "individual"] * 2
    assert c.iterations.shape == (2, 3) and c.pooled.shape == (1, 3) and c.groups.tolist() == [0, 0]
    assert c.residences.shape == (2, n) and (c.iterations["count"] == n).all() and (c.pooled["count"] == 2 * n).all()
    assert (c.pooled[0]["max"] == c.iterations["max"].max(axis=0)).all()
    assert (c.pooled[0]["n_above"] == c.iterations["n_above"].sum(axis=0)).all()
    assert (c.residences["n_above"].sum(axis=1) == c.iterations["n_above"].sum(axis=1)).all()
    assert (c.run["n_never"] == (c.residences["settle"] == 0).sum(axis=1)).all() and c.patience == 1 and c.eps == 0.5
