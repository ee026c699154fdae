"""The full-rows PDHG sweep -- revs_pdhg_t::full_rows = 1, agent_step_kernel<LPA, SPL, REVS_MODE_RELAXED_PDHG, FULL_ROWS,
MULTI> -- at every lane shape, in both launch forms and in the engine.

It is the one place that runs group_excl_suffix (K^T y) next to group_excl_prefix (K xbar): cross-lane scans with
per-group masks that can go wrong at a group's first and last lane, at the ragged last lane and at the dead lanes, and it
carries a float[n][T] multiplier from call to call.  Here:

  a. 64 fixed passes, cold and from a carried multiplier, against ro.home_solve_relaxed_pdhg(dtype=float32) -- the
     kernel's step-for-step restatement -- on the atlas of tests/window_cases.py: the schedule and the multiplier rows;
  b. the converged solve against ro.home_solve_relaxed, on the generator's windows and on the atlas (which residences
     must settle and which must report the iteration cap: tests/full_rows_cases.py), with the epilogue held to the
     float64 formulas on the kernel's own schedule;
  c. revs_agent_step_multi with kin = 3 and kin = max against launches of kin = 1, bit for bit, (n, T) multipliers
     included, and every link against tests/sweep_ref.py;
  d. AdmmEngine(mode="pdhg", pdhg=dict(full_rows=1)) against ro.solve_ADMM, and against itself with one iteration per
     streaming launch.

tests/test_full_rows_cases.py holds the conditions these rest on, on the host."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_shapes import EDGES, FULL, MAX_INNER, RAGGED, _bits, _ids, _same_bits, shape_of  # noqa: E402
from test_gpu_windows import _held, _same_rows  # noqa: E402
import full_rows_cases as fr  # noqa: E402
import window_cases as wc  # noqa: E402

HORIZONS = RAGGED + FULL
FIXED = dict(max_iter=64, check=64, tol=-1.0, polish=0, full_rows=1)
# (lanes, T): revs_pdhg_t::lanes -- 16 lanes x 2 slots and 32 lanes x 1 slot per residence at T <= 32
WIDE = [(16, 24), (32, 24), (16, 17), (32, 17), (16, 32), (32, 32)]


def _note(part, **kw):
    """One line per case with the largest error against each bar."""
    print(f"FULLROWS part={part} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _x0(P_sch, oh):
    """The kernel's primal warm start before the clip to the window's box: (P_sch - LOAD) / rating in float."""
    F = np.float32
    return (P_sch.astype(F) - oh.LOAD.astype(F)) * (F(1.0) / np.where(oh.ev, oh.rating, 1.0).astype(F))[:, None]


# ---- a. step for step -----------------------------------------------------------------------------------------------
def _follow(lib, a, w, oh, T, lanes, shape):
    """64 passes cold (no carried multiplier: x = 0, y = 0), then two calls that carry a float[n][T] multiplier: the
    first from zero rows and the state's own P_sch, the second from the rows the first left and the P_sch it wrote."""
    import torch
    from oracle import revs_oracle as ro
    from test_gpu_agent import _run_agent
    n = len(a.homes)
    ev, before = oh.ev, np.arange(T)[None, :] < oh.start[:, None]
    opts = dict(FIXED, lanes=lanes)
    rs = lambda st, dt, x0, y0: ro.home_solve_relaxed_pdhg(w.cost, oh, st[0], st[2], st[3], w.kappa, iters=64, tol=-1.0,
                                                           check=64, dtype=dt, full_rows=True, x0=x0, y0=y0)
    for zero in (True, False):
        st = fr.start(w, T, zero)
        flagged = fr.classify(T, zero)["ref"][3] == 1 if lanes == 0 else _flagged(w, oh, st)
        ok = ev & ~flagged
        want = np.where(ok, 2 | (64 << 8), np.where(flagged, 1, 0))       # 64 passes, "not settled": tol < 0 never is
        yd = torch.zeros(n, T, dtype=torch.float32, device="cuda:0")
        worst = {}
        for call in ("cold", "warm1", "warm2"):
            if call == "cold":
                r = _run_agent(lib, w, *st, "pdhg", opts)
                x0 = y0 = None
            else:
                y0 = yd.cpu().numpy()
                x0 = _x0(st[2], oh)
                r = _run_agent(lib, w, *st, "pdhg", opts, ydual=yd)
            p32, _, _, _, y32 = rs(st, np.float32, x0, y0)
            _same_rows(a, f"status after 64 passes ({call}, zero={zero})", r["status"] == want)
            worst[f"S_{call}"] = _held(a, f"S after 64 passes ({call}, zero={zero})", r["S"], p32, ok, atol=5e-4 * (1 - 1e-12))
            _same_rows(a, "charging outside the window", (np.where(oh.window(), 0.0, r["S"]) == 0).all(axis=1))
            if call != "cold":
                y_gpu = yd.cpu().numpy()
                y64 = rs(st, np.float64, x0, y0)[4]
                gap = float(np.abs(y32 - y64)[ok].max())
                # the restatement's own float32 error on these rows, x 8: the kernel's scans add in another order
                worst[f"y_{call}"] = _held(a, f"multiplier rows ({call}, zero={zero})", y_gpu, y32, ok, atol=8 * gap)
                worst[f"gap_{call}"] = gap
                assert gap > 0 and np.abs(y64[ok]).max() > 1e3 * gap, (gap, np.abs(y64[ok]).max())
                _same_rows(a, "a multiplier on a residence without EV", (y_gpu == 0).all(axis=1) | ev)
                _same_rows(a, "a multiplier on a row in front of the window", (np.where(before, y_gpu, 0.0) == 0).all(axis=1) | ~ok)
                st = (st[0], st[1], r["P_sch"], st[3])              # the next call starts from this one's schedule
        _note("a", T=T, shape=shape, zero=int(zero), n=n, flagged=int(flagged.sum()), **worst)


def _flagged(w, oh, st):
    from oracle import revs_oracle as ro
    return ro.home_solve_relaxed(w.cost, oh, st[0], st[2], st[3], w.kappa)[3] == 1


@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_fixed_passes_follow_the_restatement(gpu_lib, T):
    """64 passes (tol = -1, check = 64, polish = 0) on the atlas, from the zero and the mid-run state, cold and warm
    (`ydual` a float[n][T] filled by a first call, P_sch that call's output): the schedule within 5e-4 kW of the
    float32 restatement, every feasible EV residence with a status of 64 passes (flagged ones: the oracle's status, no
    pass), and the carried multiplier rows within 8 x the restatement's own float32-against-float64 gap on them
    (computed here and printed) -- exactly 0 on residences without EV and on the rows in front of the window, whose
    prefix sums are empty."""
    a, w, oh = fr.case(T)
    _follow(gpu_lib, a, w, oh, T, 0, shape_of(T))


@pytest.mark.parametrize("lanes,T", WIDE, ids=[f"T{T}-{lanes}x{32 // lanes}" for lanes, T in WIDE])
def test_fixed_passes_on_the_wide_shapes(gpu_lib, lanes, T):
    """The same with revs_pdhg_t::lanes = 16 and 32 (shapes 16x2 and 32x1) at T = 24, 17 and 32, on the atlas built for
    that shape's lane boundaries."""
    from helpers import oracle_homes
    a = wc.atlas(T, lanes, 32 // lanes, T)
    w = wc.workload(a)
    _follow(gpu_lib, a, w, oracle_homes(w), T, lanes, f"{lanes}x{32 // lanes}")


# ---- b. converged ---------------------------------------------------------------------------------------------------
def _epilogue(a, r, w, oh, st, what):
    """P_sch = S + LOAD, C the prefix sum, G, diff and dsq from the float64 formulas (lpsolver.py:275-284) on the
    kernel's own S, at tests/test_gpu_windows.py::test_one_iteration_on_the_atlas' continuous bars (P_sch: one float
    addition, its on/off bar) -- the solver's tolerance stays out of it.  -> the largest errors."""
    pe_old, pe_new, ps, gm = st
    n, T = w.load.shape
    S = r["S"]
    g = S + oh.LOAD
    soc = np.where(oh.ev[:, None], np.concatenate([np.zeros((n, 1)), np.cumsum(S, axis=1)], axis=1)
                   / oh.capacity[:, None] + oh.initial[:, None], 0.0)
    chk = pe_new - g
    return dict(P_sch=_held(a, f"P_sch ({what})", r["P_sch"], g, rtol=2e-6, atol=2e-6),
                C=_held(a, f"C ({what})", r["C"], soc, atol=2e-4),
                G=_held(a, f"G ({what})", r["G"], gm + 0.5 * w.kappa * chk, atol=2e-3, rtol=1e-5),
                diff=_held(a, f"diff ({what})", r["diff"], np.linalg.norm(chk, axis=1) / T, atol=1e-4, rtol=1e-4),
                dsq=_held(a, f"dsq ({what})", r["dsq"], ((g - ps) ** 2).sum(axis=1), rtol=2e-3, atol=1e-6))


class _Rows:
    """What _held and _same_rows need of an atlas, for a generator workload: a residence is named by its record."""

    def __init__(self, w):
        self.homes, self.tags = w.homes, {}


@pytest.mark.parametrize("T", _ids(EDGES))
def test_generator_windows_converge(gpu_lib, T):
    """Default options plus full_rows = 1 on make_workload's windows at every band edge: status low byte 0 everywhere
    (tests/test_full_rows_cases.py: the restatement needs fewer than 3000 of the 4000 passes there), S within
    2e-4 x 7.2 kW of ro.home_solve_relaxed, nothing outside the window, the epilogue on the kernel's own S."""
    from test_gpu_agent import _run_agent
    w, oh, st, ref, n_it = fr.generator_case(T)
    assert n_it.max() < fr.SURE and (ref[3] == 0).all()
    a = _Rows(w)
    r = _run_agent(gpu_lib, w, *st, "pdhg", dict(full_rows=1))
    _same_rows(a, "status", (r["status"] & 0xFF) == 0)
    S = _held(a, "S", r["S"], ref[0], atol=fr.BAR * (1 - 1e-12))
    _same_rows(a, "charging outside the window", (np.where(oh.window(), 0.0, r["S"]) == 0).all(axis=1))
    ep = _epilogue(a, r, w, oh, st, "generator")
    _note("b-generator", T=T, shape=shape_of(T), n=len(w.homes), passes=int((r["status"] >> 8).max()),
          passes_restated=int(n_it.max()), S=S, **ep)


@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_atlas_converges_or_reports_the_cap(gpu_lib, T):
    """Default options plus full_rows = 1 on the atlas, from the zero and the mid-run state.  A residence the float32
    restatement settles in fewer than 3000 passes: status bit 1 clear and S within 2e-4 x 7.2 kW of
    ro.home_solve_relaxed; one it has not settled after 5000: bit 1 set, "the iteration cap was reached before the
    tolerance"; between the two, nothing is asked (tests/test_full_rows_cases.py caps their share).  Flagged residences
    keep the oracle's status and get no schedule, residences without EV status 0; nothing outside the window; the
    epilogue on the kernel's own S."""
    from test_gpu_agent import _run_agent
    a, w, oh = fr.case(T)
    for zero in (True, False):
        c = fr.classify(T, zero)
        st = fr.start(w, T, zero)
        p, _, _, status = c["ref"]
        r = _run_agent(gpu_lib, w, *st, "pdhg", dict(full_rows=1))
        low = r["status"] & 0xFF
        _same_rows(a, f"status of a residence that settles (zero={zero})", (low == 0) | ~c["sure"])
        _same_rows(a, f"status of a residence at the cap (zero={zero})", (low == 2) | ~c["capped"])
        _same_rows(a, "status of a flagged residence", (low == 1) | (status != 1))
        _same_rows(a, "status of a residence without EV", (r["status"] == 0) | oh.ev)
        _same_rows(a, "status of a residence in between", np.isin(low, (0, 2)) | ~c["between"])
        S = _held(a, f"S (zero={zero})", r["S"], p, c["sure"], atol=fr.BAR * (1 - 1e-12))
        _same_rows(a, "a schedule on a flagged residence or one without EV", (r["S"] == 0).all(axis=1) | c["feasible"])
        _same_rows(a, "charging outside the window", (np.where(oh.window(), 0.0, r["S"]) == 0).all(axis=1))
        ep = _epilogue(a, r, w, oh, st, f"zero={zero}")
        _note("b-atlas", T=T, shape=shape_of(T), zero=int(zero), n=len(a.homes), sure=int(c["sure"].sum()),
              between=int(c["between"].sum()), capped=int(c["capped"].sum()), flagged=int((status == 1).sum()),
              passes_sure=int((r["status"] >> 8)[c["sure"]].max()), passes_sure_restated=int(c["passes"][c["sure"]].max()),
              S=S, **ep)


# ---- c. several iterations per launch -------------------------------------------------------------------------------
_LINKS = {}


@pytest.mark.parametrize("layout", ["dense", "sparse"])
@pytest.mark.parametrize("T", _ids(HORIZONS))
def test_multi_iteration_launch_with_full_rows(gpu_lib, T, layout):
    """revs_agent_step_multi with full_rows = 1 -- the MULTI x FULL_ROWS instantiation the engine streams with -- kin = 3
    and then kin = revs_agent_max_inner(T, 0), against the same iterations as launches of kin = 1: bit for bit on the
    state, the (n, T) multipliers, the prepared estimate, dsq, the status words, every diff row and every ring slice.
    Every link of the chain against tests/sweep_ref.py: the oracle's status, and P_sch within 2e-4 x 7.2 kW where the
    float32 restatement, from the link's own warm start (the schedule and the multiplier rows the link before it
    left), settles in fewer than 3000 passes -- there status bit 1 is clear too.

    300 residences with the generator's windows; dense: 16 nodes, the workgroups' LDS accumulators; sparse: one
    residence per node."""
    from oracle import revs_oracle as ro
    from sweep_ref import link, node_sums
    from test_gpu_agent import _prep, _state
    from test_gpu_shapes import _Sweep
    lib, n = gpu_lib, 300
    shape = shape_of(T)
    kmax = int(lib.revs_agent_max_inner(T, 0))
    assert kmax == MAX_INNER[shape], (T, shape, kmax)
    w, oh = _prep(n, T, seed=200 + T, binary_feasible=False)
    a = _Rows(w)
    node_of, M = (w.node_of, 16) if layout == "dense" else (np.arange(n), n)
    pe_old, _, ps, gm = _state(w, T + 2)
    state = (pe_old, ps, gm)
    sw = _Sweep(lib, w, node_of, M, "pdhg", dict(full_rows=1))
    assert sw.pd.full_rows == 1 and sw.pd.polish == 1            # (the polish is the presolved form's: not run here)
    mt, tot = sw.mt, 3 + kmax
    multi, m_diff, m_ring = sw.run(state, [3, kmax], rotate_y=True)
    chain, c_diff, c_ring = sw.run(state, [1] * tot, rotate_y=False)
    assert multi[0]["y"].shape == (n, T) and np.abs(chain[-1]["y"]).max() > 0

    # ---- bit for bit ----
    for snap, at in ((multi[0], 2), (multi[1], tot - 1)):
        for k in ("P_est", "P_sch", "G", "pen2", "dsq", "y"):
            _same_rows(a, f"{k} after {at + 1} iterations, multi against chain",
                       (_bits(snap[k]) == _bits(chain[at][k])).reshape(n, -1).all(axis=1))
    cst = np.stack([s["status"] for s in chain])
    for snap, lo, hi in ((multi[0], 0, 3), (multi[1], 3, tot)):
        want = cst[hi - 1] | np.bitwise_or.reduce(cst[lo:hi] & 7, axis=0)
        _same_rows(a, f"status word of iterations {lo}..{hi}", snap["status"] == want)
    assert _same_bits(m_diff, c_diff)
    for i in range(tot - 1):
        assert _same_bits(chain[i]["pen2"], chain[i + 1]["P_est"]), i
    for name, ring, diff in (("multi", m_ring, m_diff), ("chain", c_ring, c_diff)):
        assert _same_bits(ring[:, mt:].max(axis=1), diff.max(axis=1).astype(np.float64)), name
    for i in range(tot):
        ref = node_sums(node_of, M, chain[i]["pen2"]).ravel()
        assert _same_bits(m_ring[i, :mt], c_ring[i, :mt]), i
        assert np.abs(c_ring[i, :mt] - ref).max() <= 1e-12 * max(np.abs(ref).max(), np.finfo(np.float64).tiny), i

    # ---- every link of the chain against float64 ----
    key = (T,)                      # (the state does not depend on the node layout)
    if key in _LINKS and all(_same_bits(x[k], y[k]) for x, y in zip(_LINKS[key][0], chain) for k in ("P_est", "P_sch", "G", "y")):
        links = _LINKS[key][1]
    else:
        links, st = [], tuple(np.asarray(x, np.float64) for x in state)
        y0 = np.zeros((n, T), np.float32)
        for s in chain:
            lk = link(w.cost, oh, st[0], st[1], st[2], w.kappa, "relaxed")
            n_it = ro.home_solve_relaxed_pdhg(w.cost, oh, st[0], st[1], st[2], w.kappa, iters=fr.SURE, tol=fr.TOL,
                                              check=fr.CHECK, dtype=np.float32, full_rows=True, x0=_x0(st[1], oh), y0=y0)[3]
            links.append((lk, oh.ev & (lk.status == 0) & (n_it < fr.SURE)))
            st, y0 = tuple(s[k].astype(np.float64) for k in ("P_est", "P_sch", "G")), s["y"]
        _LINKS.clear()
        _LINKS[key] = (chain, links)
    st = tuple(np.asarray(x, np.float64) for x in state)
    worst, left_out = dict(pen=0.0, sch=0.0, G=0.0, diff=0.0), 0
    for i, (s, (lk, sure)) in enumerate(zip(chain, links)):
        pe, p_s, G0 = st
        pen_gpu, sch, Gn = (s[k].astype(np.float64) for k in ("P_est", "P_sch", "G"))
        bar = 2.0 ** -22 * (0.5 * (np.abs(pe) + np.abs(p_s)) + np.abs(G0) / w.kappa)
        worst["pen"] = max(worst["pen"], float((np.abs(pen_gpu - lk.pen) / np.maximum(bar, 1e-300)).max()))
        _same_rows(a, f"P_est of link {i}", (np.abs(pen_gpu - lk.pen) <= bar).all(axis=1))
        rows = sure | ~oh.ev
        left_out += int((~rows).sum())
        _same_rows(a, f"status of link {i}", ((cst[i] & 0xFF) == lk.status) | ~rows)
        _same_rows(a, f"status of link {i}, left-out residences", np.isin(cst[i] & 0xFF, (0, 2)) | rows)
        worst["sch"] = max(worst["sch"], _held(a, f"P_sch of link {i}", sch, lk.g, rows, atol=fr.BAR * (1 - 1e-12)))
        # the epilogue of the link on the kernel's own schedule
        chk = pen_gpu - sch
        worst["G"] = max(worst["G"], _held(a, f"G of link {i}", Gn, G0 + 0.5 * w.kappa * chk, atol=2e-3, rtol=1e-5))
        worst["diff"] = max(worst["diff"], _held(a, f"diff of link {i}", c_diff[i], np.linalg.norm(chk, axis=1) / T, atol=1e-4, rtol=1e-4))
        _held(a, f"dsq of link {i}", s["dsq"], ((sch - p_s) ** 2).sum(axis=1), rtol=2e-3, atol=1e-6)
        st = (pen_gpu, sch, Gn)
    assert left_out <= 0.08 * tot * int(oh.ev.sum()), left_out
    _note("c", T=T, shape=shape, layout=layout, n=n, kin=f"3+{kmax}", left_out=left_out, pen_over_bar=worst["pen"],
          sch=worst["sch"], G=worst["G"], diff=worst["diff"])


# ---- d. the engine --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stress", [0.9, 1.5])
def test_engine_with_full_rows(gpu_lib, stress):
    """tests/test_gpu_admm.py::test_relaxed_trajectory's workload with pdhg = dict(full_rows = 1) and the Newton operator,
    eight iterations against ro.solve_ADMM(mode = "relaxed"): diff within 1e-3 relative, S and P_sch within 2e-3 kW --
    that test's bar for PDHG without the KKT polish, which the full-rows form does not have (the
    first-order tail is 1e-3 kW in the closed loop) -- and C within that bar x the window length / the smallest
    capacity; check_status() is clean; the carried multipliers are (n, T) and the buffer the plan works on: a further
    iteration of the general driver moves them.  Then the same run, and 30 more iterations through run_steps, with
    OperatorOptions(stream_inner = 1): the residences' state and multipliers are the same bit for bit -- part c inside
    the engine."""
    import torch
    from helpers import f32, oracle_homes
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import OperatorOptions
    from revs_admm_amd.synthetic import make_workload
    from test_gpu_admm import _engine
    w = make_workload(600, 24, n_nodes=60, seed=11, binary_feasible=False, stress=stress)
    w.load, w.cost = f32(w.load), f32(w.cost)
    oh = oracle_homes(w)
    iters, n, T = 8, 600, 24
    e = _engine(w, "pdhg", op=OperatorOptions(solver="newton"), pdhg=dict(full_rows=1))
    diffs = e.run(iters)
    P_sch, S, Cs = e.result()
    e.check_status()
    d_ref, P_ref, S_ref, C_ref = ro.solve_ADMM(oh, w.Rn, w.node_of, w.cost, w.kappa, iters, w.vset, w.vlow, w.vhigh,
                                               mode="relaxed", util_eps=1e-10)
    tol = 2e-3
    c_tol = tol * (oh.end - oh.start)[oh.ev].max() / oh.capacity[oh.ev].min()
    err = dict(diff=float(np.abs(diffs - d_ref).max()), S=float(np.abs(S - S_ref).max()),
               P_sch=float(np.abs(P_sch - P_ref).max()), C=float(np.abs(Cs - C_ref).max()))
    assert e.pdhg_dual.shape == (n, T) and e.pdhg_dual.dtype == torch.float32
    assert float(e.pdhg_dual.abs().max()) > 0 and float(e.pdhg_dual[torch.from_numpy(~oh.ev[e.perm]).to(e.pdhg_dual.device)].abs().max()) == 0

    b = _engine(w, "pdhg", op=OperatorOptions(solver="newton", stream_inner=1), pdhg=dict(full_rows=1))
    b.run(iters)
    assert b._inner == 1 and e._inner == MAX_INNER[shape_of(T)]
    names = ("P_est", "P_sch", "G", "diff", "pdhg_dual")
    same = lambda: [k for k in names if not torch.equal(getattr(e, k), getattr(b, k))]
    assert not same(), same()
    for eng in (e, b):
        eng.run_steps(30)
    assert e.iteration == b.iteration == iters + 30 and not same(), same()
    # the general driver's sweep reads and writes the plan's multipliers: they are the engine's tensor
    before = e.pdhg_dual.clone()
    for eng in (e, b):
        eng.step(write_sc=True)
        eng.check_status()
    assert e.pdhg_dual.shape == (n, T) and not torch.equal(before, e.pdhg_dual)
    assert not same(), same()
    for x, y in zip(e.result(), b.result()):
        np.testing.assert_array_equal(x, y)
    _note("d", stress=stress, T=T, shape=shape_of(T), spec=f"{e.spec_hist[0]}/{e.spec_hist[1]}", stream_calls=len(e.stream_calls),
          C_bar=float(c_tol), **err)
    assert err["diff"] < 1e-3 * max(1.0, d_ref.max())
    assert err["S"] < tol and err["P_sch"] < tol and err["C"] < c_tol
    if stress < 1.0:            # the rows rest: the streaming loop, several iterations per launch, is what ran
        assert e.spec_hist[0] > 0 and e.stream_calls, (e.spec_hist, e.stream_calls)
