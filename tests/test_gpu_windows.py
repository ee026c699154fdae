"""The sweep kernels at every window placement per lane shape.

tests/window_cases.py lists, per horizon, the residences at which a kernel that spreads a residence's slots over lanes is
most likely to be wrong: one-slot windows on both sides of every lane boundary, windows of exactly one lane, inside one
lane, over the ragged last lane, reaching outside the horizon, each needing no slot, one slot, half the window, the
whole window, one slot more than the window, or fewer slots than the least that reaches 90 %.  Here revs_agent_step,
revs_agent_step_multi and revs_dual_bound run on that atlas at one horizon per shape (and the full horizons 24, 64 and
192) and are held to oracle/revs_oracle.py, tests/sweep_ref.py and tests/bound_ref.py at the bars the project already
uses for the same quantities; the engine's streaming loop runs on the feasible part of it.  A miss names the residence:
its category, need class, window and slot counts (window_cases.describe)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_shapes import MAX_INNER, RAGGED, _bits, _ids, _note, _same_bits, shape_of  # noqa: E402
import window_cases as wc  # noqa: E402

HORIZONS = RAGGED + [24, 64, 192]
_ATLAS, _ORACLE, _LINKS = {}, {}, {}


def _case(T):
    """-> (atlas, workload, oracle homes) of horizon T, built once."""
    from helpers import oracle_homes
    if T not in _ATLAS:
        a = wc.atlas_of(T)
        w = wc.workload(a)
        _ATLAS[T] = (a, w, oracle_homes(w))
    return _ATLAS[T]


def _start(w, T, zero):
    from test_gpu_agent import _state
    n = len(w.homes)
    return (np.zeros((n, T)),) * 4 if zero else _state(w, T)


def _oracle(T, zero, kind):
    """ro.home_solve_binary / ro.home_solve_relaxed of the atlas from the zero or the mid-run state, once."""
    from oracle import revs_oracle as ro
    key = (T, zero, kind)
    if key not in _ORACLE:
        a, w, oh = _case(T)
        pe_old, _, ps, gm = _start(w, T, zero)
        solve = ro.home_solve_binary if kind == "binary" else ro.home_solve_relaxed
        _ORACLE[key] = solve(w.cost, oh, pe_old, ps, gm, w.kappa)
    return _ORACLE[key]


def _held(a, what, got, ref, rows=None, rtol=0.0, atol=0.0):
    """|got - ref| <= atol + rtol |ref| on the residences `rows` (numpy's assert_allclose rule); a miss names the worst
    residence.  Returns the largest |got - ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rows = np.arange(len(a.homes)) if rows is None else np.flatnonzero(rows) if rows.dtype == bool else rows
    if not len(rows):
        return 0.0
    err = np.abs(got - ref)[rows].reshape(len(rows), -1)
    over = (err - (atol + rtol * np.abs(ref[rows]).reshape(len(rows), -1))).max(axis=1)
    i = int(np.argmax(over))
    assert over[i] <= 0, f"{what}: off by {err[i].max():.3e} (bar {atol:.1e} + {rtol:.1e} |ref|) at {wc.describe(a, rows[i])}"
    return float(err.max())


def _same_rows(a, what, ok):
    """`ok` (per residence) holds everywhere; a miss names the first residence where it does not."""
    bad = np.flatnonzero(~ok)
    assert not len(bad), f"{what}: {len(bad)} residences, first {wc.describe(a, bad[0])}"


def _capped(lib, a, w, oh, pe, ps, gm, x0=None, y0=None):
    """The one place where the low status byte of a PDHG residence is not the oracle's.  A residence of class nmin_W has
    one feasible schedule (every slot at full rating, to float rounding): PDHG's multiplier has to grow until the worst
    slot saturates, in steps that shrink with the row's residual, and on the longest windows the default cap of 4000
    passes comes first.  Measured at T = 192, window [0, 192), from the mid-run state: 4000 passes and status bit 1, "the
    iteration cap was reached before the tolerance"; 5144 passes with the cap lifted; from the zero state 3112.  The KKT
    steps behind PDHG settle the residence all the same (bit 2 clear, schedule 1.1e-6 kW off the oracle's, inside the
    1e-4 bar that is kept).  It is the stopping rule and not the kernel: ro.home_solve_relaxed_pdhg in float32 with the
    kernel's own cap, tolerance and starting point takes the same 3112 and 4000 passes on that residence.  So on nmin_W
    residences, and only there, bit 1 is expected exactly where that restatement reaches the cap.
    -> (n,) bool."""
    import ctypes as C
    from oracle import revs_oracle as ro
    from revs_admm_amd._lib import PDHG
    pd = PDHG()
    lib.revs_pdhg_defaults(C.byref(pd))
    assert pd.polish == 1 and pd.tol == 0.0 and not pd.full_rows       # (automatic tolerance: 1e-4 in front of the polish)
    rows = a.tags["nmin_W"]
    sub = ro.Homes(*(getattr(oh, k)[rows] for k in ("LOAD", "ev", "rating", "capacity", "initial", "start", "end")))
    n_it = ro.home_solve_relaxed_pdhg(w.cost, sub, pe[rows], ps[rows], gm[rows], w.kappa, iters=pd.max_iter, tol=1e-4,
                                      check=pd.check, dtype=np.float32, full_rows=False,
                                      x0=None if x0 is None else x0[rows], y0=None if y0 is None else y0[rows])[3]
    out = np.zeros(len(a.homes), bool)
    out[rows] = n_it >= pd.max_iter
    return out


# ---- a. one iteration per launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["binary", "relaxed_exact", "pdhg", "pdhg_presolve"])
@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_one_iteration_on_the_atlas(gpu_lib, T, mode):
    """revs_agent_step from the zero state and from a mid-run state, at tests/test_gpu_agent.py::test_edge_parameters'
    bars: the oracle's status for every residence (PDHG: with the iteration cap's bit where _capped expects it); on/off
    chargers (keys64 = 1) the oracle's schedule on every feasible residence, objective within 2e-5 and identical slot
    counts; continuous chargers (closed form, PDHG, PDHG behind the
    KKT steps: polish = 3) |S - oracle| < 1e-4 kW; nothing outside the window, nothing on flagged residences,
    C[:, 0] = initial.  The epilogue on the feasible residences at the bars of tests/test_gpu_shapes.py::
    test_one_iteration_*_at_band_edges: P_sch and C within 2e-6, G 1e-5, diff 1e-5 (on/off); C 2e-4, G 2e-3, diff 1e-4,
    dsq 2e-3 relative (continuous)."""
    from oracle import revs_oracle as ro
    from test_gpu_agent import _run_agent
    a, w, oh = _case(T)
    n = len(a.homes)
    binary = mode == "binary"
    for zero in (True, False):
        pe_old, pe_new, ps, gm = _start(w, T, zero)
        if mode == "pdhg_presolve":
            r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", dict(polish=3))
        else:
            r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode, dict(keys64=1) if binary else None)
        p, s, g, st = _oracle(T, zero, "binary" if binary else "relaxed")
        ok = st == 0
        chk = pe_new - g
        S_err = np.abs(r["S"] - p).max(axis=1)
        worst = int(np.argmax(np.where(ok, S_err, -1.0)))
        note = dict(T=T, shape=shape_of(T), mode=mode, zero=int(zero), n=n, flagged=int((~ok).sum()), S=float(S_err[worst]),
                    S_at=wc.describe(a, worst).split("]")[0].split("[")[1].replace(" ", "+"),
                    C=float(np.abs(r["C"] - s)[ok].max()), G=float(np.abs(r["G"] - (gm + 0.5 * w.kappa * chk))[ok].max()),
                    diff=float(np.abs(r["diff"] - np.linalg.norm(chk, axis=1) / T)[ok].max()))
        if binary:
            obj_g = ro.home_objective(w.cost, oh, r["S"], pe_old, ps, gm, w.kappa)
            obj_r = ro.home_objective(w.cost, oh, p, pe_old, ps, gm, w.kappa)
            note["obj"] = float(np.max(np.abs(obj_g - obj_r)[ok] / np.maximum(1, np.abs(obj_r[ok]))))
        want = st | 2 * _capped(gpu_lib, a, w, oh, pe_old, ps, gm) if mode == "pdhg" else st
        note["capped"] = int((want & 2).sum() // 2)
        _note("w-a", **note)
        _same_rows(a, f"status ({mode}, zero={zero})", (r["status"] & 0xFF) == want)
        if binary:
            assert note["obj"] < 2e-5
            _same_rows(a, "slot count", ((r["S"] > 0).sum(1) == (p > 0).sum(1)) | ~ok)
            _same_rows(a, "on/off schedule", (S_err == 0) | ~ok)
        else:
            _held(a, f"S ({mode}, zero={zero})", r["S"], p, ok, atol=1e-4 * (1 - 1e-12))
        _same_rows(a, "charging outside the window", (np.where(oh.window(), 0.0, r["S"]) == 0).all(axis=1))
        _same_rows(a, "a schedule on a flagged residence", (r["S"] == 0).all(axis=1) | ok)
        _held(a, "C[:, 0]", r["C"][:, 0], np.where(oh.ev, oh.initial, 0), ok, atol=1e-6)
        G = gm + 0.5 * w.kappa * chk
        dref = np.linalg.norm(chk, axis=1) / T
        if binary:
            _held(a, "P_sch", r["P_sch"], g, ok, rtol=2e-6, atol=2e-6)
            _held(a, "C", r["C"], s, ok, rtol=2e-6, atol=2e-6)
            _held(a, "G", r["G"], G, ok, rtol=1e-5, atol=1e-5)
            _held(a, "diff", r["diff"], dref, ok, rtol=1e-5, atol=1e-6)
        else:
            _held(a, "C", r["C"], s, ok, atol=2e-4)
            _held(a, "G", r["G"], G, ok, atol=2e-3, rtol=1e-5)
            _held(a, "diff", r["diff"], dref, ok, atol=1e-4, rtol=1e-4)
            _held(a, "dsq", r["dsq"], ((g - ps) ** 2).sum(axis=1), ok, rtol=2e-3, atol=1e-6)


# ---- b. several iterations per launch -------------------------------------------------------------------------------
def _ordered(a, layout):
    """by_class: the residences sorted by need class (those without EV first), so that workgroups hold like residences
    -- all flagged, all without EV; shuffled: a random order, workgroups mixed."""
    n = len(a.homes)
    if layout == "dense_shuffled":
        return wc.reordered(a, np.random.default_rng(n).permutation(n))
    cls = np.zeros(n, np.int64)
    for k, name in enumerate(wc.NEEDS):
        cls[a.tags[name]] = k + 1
    return wc.reordered(a, np.argsort(cls, kind="stable"))


@pytest.mark.parametrize("layout", ["dense", "dense_shuffled", "sparse"])
@pytest.mark.parametrize("mode", ["binary", "relaxed_exact", "pdhg"])
@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_multi_iteration_launch_on_the_atlas(gpu_lib, T, mode, layout):
    """revs_agent_step_multi with kin = 3 and then kin = revs_agent_max_inner(T, 0), against the same iterations as
    launches of kin = 1: bit for bit on the state, the carried multipliers, pen2, dsq, the status words (a launch ORs the
    low three bits of its inner iterations), every diff row and every ring slice (node sums and partial maxima of diff);
    and every link of the chain against tests/sweep_ref.py at the bars of tests/test_gpu_shapes.py::
    test_multi_iteration_launch_equals_a_chain_of_single_launches (PDHG: the status with the iteration cap's bit where
    _capped expects it from the link's own warm start, the state's schedule and the carried multiplier).

    dense: all residences on 16 nodes, sorted by need class (workgroups of like residences); dense_shuffled: the same in
    a random order (mixed workgroups); sparse: one residence per node.  The residences are sorted by node in each, as
    the entry point demands."""
    _atlas_chain(gpu_lib, T, mode, layout, 5.0)


@pytest.mark.parametrize("kappa", [0.8, 3.3, 7.0])
@pytest.mark.parametrize("mode", ["binary", "relaxed_exact", "pdhg"])
@pytest.mark.parametrize("T", _ids([24, 96]))
def test_multi_iteration_launch_on_the_atlas_at_other_penalties(gpu_lib, T, mode, kappa):
    """test_multi_iteration_launch_on_the_atlas (dense layout), every check and bar as there, at the two bench lane
    shapes and the ADMM penalties of tests/param_cases.py other than 5: 1 / kappa and kappa / 2 rounded floats."""
    from param_cases import OFF_KAPPAS
    assert kappa in OFF_KAPPAS and len(OFF_KAPPAS) == 3
    _atlas_chain(gpu_lib, T, mode, "dense", kappa)


def _atlas_chain(lib, T, mode, layout, kappa):
    from helpers import oracle_homes
    from sweep_ref import link, node_sums
    from test_gpu_agent import _state
    from test_gpu_shapes import _Sweep
    shape = shape_of(T)
    kmax = int(lib.revs_agent_max_inner(T, 0))
    assert kmax == MAX_INNER[shape], (T, shape, kmax)
    a = _ordered(_case(T)[0], layout)
    w = wc.workload(a, kappa)
    oh = oracle_homes(w)
    n = len(a.homes)
    node_of, M = (np.arange(n), n) if layout == "sparse" else (np.arange(n) * 16 // n, 16)
    assert (np.diff(node_of) >= 0).all() and node_of.max() == M - 1
    pe_old, _, ps, gm = _state(w, T + 2)
    state = (pe_old, ps, gm)
    sw = _Sweep(lib, w, node_of, M, mode)
    mt, tot = sw.mt, 3 + kmax
    multi, m_diff, m_ring = sw.run(state, [3, kmax], rotate_y=True)
    chain, c_diff, c_ring = sw.run(state, [1] * tot, rotate_y=False)

    # ---- bit for bit ----
    for snap, at in ((multi[0], 2), (multi[1], tot - 1)):
        for k in ("P_est", "P_sch", "G", "pen2", "dsq") + (("y",) if mode == "pdhg" else ()):
            x, y = snap[k], chain[at][k]
            _same_rows(a, f"{k} after {at + 1} iterations, multi against chain",
                       (_bits(x) == _bits(y)).reshape(n, -1).all(axis=1))
    cst = np.stack([s["status"] for s in chain])
    for snap, lo, hi in ((multi[0], 0, 3), (multi[1], 3, tot)):
        want = cst[hi - 1] | np.bitwise_or.reduce(cst[lo:hi] & 7, axis=0)
        _same_rows(a, f"status word of iterations {lo}..{hi}", snap["status"] == want)
    assert _same_bits(m_diff, c_diff)
    for i in range(tot - 1):
        assert _same_bits(chain[i]["pen2"], chain[i + 1]["P_est"]), i
    for name, ring, diff in (("multi", m_ring, m_diff), ("chain", c_ring, c_diff)):
        assert _same_bits(ring[:, mt:].max(axis=1), diff.max(axis=1).astype(np.float64)), name
        assert (ring[:, mt:] >= 0).all()
    slice_err = 0.0
    for i in range(tot):
        ref = node_sums(node_of, M, chain[i]["pen2"]).ravel()
        big = max(np.abs(ref).max(), np.finfo(np.float64).tiny)
        assert _same_bits(m_ring[i, :mt], c_ring[i, :mt]), i
        err = float(np.abs(c_ring[i, :mt] - ref).max() / big)
        slice_err = max(slice_err, err)
        assert err <= 1e-12, (i, err)

    # ---- every link of the chain against float64 ----
    key = (T, mode, layout != "dense_shuffled", kappa)    # (the state does not depend on the node layout)
    if key in _LINKS and all(_same_bits(x[k], y[k]) for x, y in zip(_LINKS[key][0], chain) for k in ("P_est", "P_sch", "G")):
        links = _LINKS[key][1]
    else:
        links, st = [], tuple(np.asarray(x, np.float64) for x in state)
        for s in chain:
            links.append(link(w.cost, oh, st[0], st[1], st[2], w.kappa, "binary" if mode == "binary" else "relaxed"))
            st = tuple(s[k].astype(np.float64) for k in ("P_est", "P_sch", "G"))
        _LINKS.clear()
        _LINKS[key] = (chain, links)
    rate = max(1.0, float(w.homes["rating"].max()))
    st = tuple(np.asarray(x, np.float64) for x in state)
    worst = dict(pen=0.0, sch=0.0, G=0.0, diff=0.0)
    flagged = capped = 0
    for i, (s, lk) in enumerate(zip(chain, links)):
        pe, p_s, G0 = st
        pen_gpu, sch, Gn = (s[k].astype(np.float64) for k in ("P_est", "P_sch", "G"))
        bar = 2.0 ** -22 * (0.5 * (np.abs(pe) + np.abs(p_s)) + np.abs(G0) / w.kappa)
        worst["pen"] = max(worst["pen"], float((np.abs(pen_gpu - lk.pen) / np.maximum(bar, 1e-300)).max()))
        _same_rows(a, f"P_est of link {i}", (np.abs(pen_gpu - lk.pen) <= bar).all(axis=1))
        want = lk.status
        if mode == "pdhg":
            y0 = np.zeros(n) if i == 0 else chain[i - 1]["y"].astype(np.float64)
            cap = _capped(lib, a, w, oh, pe, p_s, G0, x0=(p_s - oh.LOAD) / np.where(oh.ev, oh.rating, 1.0)[:, None], y0=y0)
            want, capped = want | 2 * cap, capped + int(cap.sum())
        _same_rows(a, f"status of link {i}", (cst[i] & 0xFF) == want)
        flagged = int((lk.status != 0).sum())
        chk = pen_gpu - lk.g
        Gref = G0 + 0.5 * w.kappa * chk
        dref = np.linalg.norm(chk, axis=1) / T
        if mode == "binary":
            on = ((sch - oh.LOAD) > 0.5 * oh.rating[:, None]) & oh.ev[:, None]
            _same_rows(a, f"on/off schedule of link {i}", (on == (lk.p > 0)).all(axis=1))
            worst["sch"] = max(worst["sch"], _held(a, f"P_sch of link {i}", sch, lk.g, rtol=2e-6, atol=2e-6))
            worst["G"] = max(worst["G"], _held(a, f"G of link {i}", Gn, Gref, rtol=1e-5, atol=1e-5))
            worst["diff"] = max(worst["diff"], _held(a, f"diff of link {i}", c_diff[i], dref, rtol=1e-5, atol=1e-6))
        else:
            worst["sch"] = max(worst["sch"], _held(a, f"P_sch of link {i}", sch, lk.g, atol=5e-5 * rate * (1 - 1e-12)))
            worst["G"] = max(worst["G"], _held(a, f"G of link {i}", Gn, Gref, atol=2e-3, rtol=1e-5))
            worst["diff"] = max(worst["diff"], _held(a, f"diff of link {i}", c_diff[i], dref, atol=1e-4, rtol=1e-4))
            _held(a, f"dsq of link {i}", s["dsq"], ((lk.g - p_s) ** 2).sum(axis=1), rtol=2e-3, atol=1e-6)
        st = (pen_gpu, sch, Gn)
    _note("w-b", T=T, shape=shape, mode=mode, layout=layout, kappa=kappa, n=n, kin=f"3+{kmax}", flagged=flagged, capped=capped, slice=slice_err,
          pen_over_bar=worst["pen"], sch=worst["sch"], G=worst["G"], diff=worst["diff"])


# ---- c. dual bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_dual_bound_on_the_atlas(gpu_lib, T):
    """revs_dual_bound against tests/bound_ref.py with the cases and bars of tests/test_gpu_shapes.py::
    test_dual_bound_equals_the_float64_restatement (relaxed and on/off, s in {0, 0.5, 1, 3}, random signed y; 1e-11
    relative per part and on p_node, bit-identical from call to call) on the atlas, spread over the 60 nodes of a
    make_workload feeder.  The residences whose own rows are empty are counted exactly, and they are the ones the atlas
    says: on/off, the classes nmin_W1 and nmax_lt_nmin; relaxed, nmin_W1 and the nmax_lt_nmin residences on one-slot
    windows (1.33 slots' energy fits every longer one).  Residences without EV and those charged past 90 % have rows
    that hold (p = 0) and are not among them."""
    import torch
    from bound_ref import dual_bound
    from revs_admm_amd._lib import check, ptr
    from revs_admm_amd.synthetic import make_workload
    from test_gpu_bound import _sparse_y
    lib = gpu_lib
    a, wa, oh = _case(T)
    n = len(a.homes)
    f = make_workload(n, T, n_nodes=60, seed=7, binary_feasible=False, stress=1.0)      # the feeder and the residences' nodes
    cost, load, homes, node_np = a.cost, a.load, a.homes, f.node_of
    vlo, vhi = f.vlow ** 2 - f.vset ** 2, f.vhigh ** 2 - f.vset ** 2
    y = _sparse_y(np.random.default_rng(T), f.M, T)
    d = f.Rn.T @ y
    W = oh.window().sum(1)
    n_bad = {True: len(a.tags["infeasible"]),
             False: len(a.tags["nmin_W1"]) + int((W[a.tags["nmax_lt_nmin"]] < 2).sum())}
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_cost, hd, d_node = up(cost.astype(np.float32)), up(homes.view(np.uint8).reshape(n, 32)), up(node_np.astype(np.int32))
    lsum = np.zeros((f.M, T))
    np.add.at(lsum, node_np, load)
    d_d, y_d, l_d = up(d), up(y), up(lsum)
    scratch = torch.zeros(int(lib.revs_dual_bound_scratch(n, T)), dtype=torch.float64, device=dev)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    pn = torch.zeros(f.M, T, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    worst = dict(total=0.0, per_part=0.0, p_node=0.0)
    for integral in (False, True):
        for s in (0.0, 0.5, 1.0, 3.0):
            got = []
            for rep in range(2):
                pn.zero_()
                check(lib.revs_dual_bound(n, T, ptr(d_cost), ptr(hd), ptr(d_node), f.M, ptr(d_d), ptr(y_d), ptr(l_d),
                                          s, vlo, vhi, int(integral), ptr(scratch), ptr(pn), ptr(out), st), "revs_dual_bound")
                got.append((out.cpu().numpy().copy(), pn.cpu().numpy()))
            (o1, p1), (o2, p2) = got
            assert np.array_equal(o1, o2), (integral, s, o1, o2)
            ref, parts, empty, _, pref = dual_bound(cost, homes, load, node_np, f.Rn, y, s, vlo, vhi, integral=integral, d=d)
            tot = (o1[0] + o1[1]) + o1[2]
            worst["total"] = max(worst["total"], abs(tot - ref) / abs(ref))
            for k, v in zip(("home", "load", "row"), o1[:3]):
                worst["per_part"] = max(worst["per_part"], abs(v - parts[k]) / max(abs(parts[k]), abs(ref)))
            worst["p_node"] = max(worst["p_node"], float(np.abs(p1 - pref).max() / max(1.0, np.abs(pref).max())))
            assert o1[3] == empty == n_bad[integral], (integral, s, o1[3], empty, n_bad[integral])
            assert abs(tot - ref) <= 1e-11 * abs(ref), (integral, s, tot, ref)
            for k, v in zip(("home", "load", "row"), o1[:3]):
                assert abs(v - parts[k]) <= 1e-11 * max(abs(parts[k]), abs(ref)), (integral, s, k, v, parts[k])
            assert np.abs(p1 - pref).max() <= 1e-11 * max(1.0, np.abs(pref).max()), (integral, s)
            assert pref.max() > 0
    _note("w-c", T=T, shape=shape_of(T), kernel="dual_bound", n=n, empty_onoff=n_bad[True], empty_relaxed=n_bad[False],
          **worst)


# ---- d. the engine's streaming loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", _ids([41, 113]))
def test_closed_loop_on_the_feasible_atlas(gpu_lib, T):
    """AdmmEngine (PDHG residences) on the feeder of make_workload(n, T, n_nodes=60, stress=1.02) with the atlas'
    feasible residences and their load in place of the generator's: run_steps(59) and a last step, against
    ro.solve_ADMM (relaxed residences, dual operator) at tests/test_gpu_agent.py::test_wide_lane_shapes_in_the_engine's
    bars -- S within 5e-4 kW, the last diff within 1e-3 x max(1, max diff) -- and the streaming loop is what ran
    (more than 20 iterations kept).

    The generator scales the resistances against ITS residences' coordinated profile.  The atlas' load (uniform in
    (0.2, 5) kW) is about three times the generator's: on the feeder as it comes, the base load alone sits at 1.49
    (T = 41) and 1.69 (T = 113) times the voltage limit, and with the resistances scaled by the generator's own rule to
    a stress of 1.02 for the atlas, the oracle's rows still bind through iteration 45 and through all 60 -- the
    streaming loop, which runs while the rows rest, would not be what ran.  So the resistances are scaled by that rule
    to a stress of 0.9: in the oracle's run (on the CPU) the rows bind through iteration 8 (T = 41) and 9 (T = 113) and
    then rest with 10 to 13 % to spare, which leaves the transient, the hand-over and 50 streaming iterations."""
    from helpers import f32, oracle_homes
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    a = wc.atlas_of(T, feasible_only=True)
    n = len(a.homes)
    w = make_workload(n, T, n_nodes=60, stress=1.02)
    w.homes, w.load, w.cost = a.homes, a.load, f32(w.cost)
    oh = oracle_homes(w)
    win = oh.window()
    peak = np.zeros((w.M, T))            # make_workload's rule: every EV's need spread evenly over its window
    np.add.at(peak, w.node_of, w.load + win * (ro.energy_bounds(oh)[0] / np.maximum(win.sum(1), 1))[:, None])
    k = 0.9 * ro.voltage_limits(w.vset, w.vlow, w.vhigh)[1] / (w.Rn @ peak).max()
    w.Rn, w.edge_r = w.Rn * k, w.edge_r * k
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run_steps(59)
    e.step(write_sc=True)
    d_ref, P_ref, S_ref, C_ref = ro.solve_ADMM(oracle_homes(w), w.Rn, w.node_of, w.cost, w.kappa, 60, w.vset, w.vlow,
                                               w.vhigh, mode="relaxed", util_method="dual")
    P, S, Cs = e.result()
    S_err = np.abs(S - S_ref).max(axis=1)
    d_err = np.abs(e.diff.cpu().numpy()[e.inv_perm] - d_ref[59])
    d_bar = 1e-3 * max(1.0, d_ref.max())
    _note("w-d", T=T, shape=shape_of(T), n=n, spec=f"{e.spec_hist[0]}/{e.spec_hist[1]}", S=float(S_err.max()),
          S_at=wc.describe(a, int(np.argmax(S_err))).split("]")[0].split("[")[1].replace(" ", "+"),
          diff=float(d_err.max()), diff_bar=d_bar)
    assert e.spec_hist[0] > 20, e.spec_hist
    _held(a, "S", S, S_ref, atol=5e-4 * (1 - 1e-12))
    _held(a, "last diff", d_err, np.zeros(n), atol=d_bar * (1 - 1e-12))
