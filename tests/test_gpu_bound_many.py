"""Every scenario's dual bound in one launch (revs_dual_bound_many, AdmmEnsemble.lower_bounds / certificates, DESIGN.md
sections 3.6 and 3.9): the kernel bit for bit against revs_dual_bound on contiguous copies of each scenario and against
the float64 restatement (tests/bound_ref.py) in every lane shape and past 256 columns; the ensemble's methods against one
AdmmEngine per scenario and against HiGHS (oracle.solve_central_lp); a run left untouched; the call surface."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# (S, T): lane shapes 8x3, 8x1, 16x6, 64x3; 288, 260, 384 and 264 columns lie past one tile of 256
SHAPES = [(1, 24), (3, 24), (5, 7), (3, 96), (2, 130), (2, 192), (11, 24)]
N_RES, N_NODES, N_EMPTY = 203, 23, 5          # 203 residences: a ragged last workgroup in every lane shape


def _scenario_records(rng, n, T, s):
    """EV ownership, rating and windows of scenario s's own (test_ensemble_host.py's draw, the windows scaled to T).
    Every record has a level in 0.9 .. 1 within reach (rating / capacity < 0.1, the window wide enough): no residence
    has empty rows until _with_empty_rows makes some."""
    from revs_admm_amd.engine import pack_homes
    rating = (3.6, 2.4, 3.0)[s % 3]
    capacity = rng.choice([40.0, 60.0, 80.0], n)
    start = (rng.integers(10, 14, n) * T) // 24
    end = np.minimum((rng.integers(21, 25, n) * T) // 24, T)
    ev = rng.random(n) < (0.5, 0.3, 0.7)[s % 3]
    initial = np.maximum(np.clip(0.9 - rng.uniform(0.3, 0.7, n), 0.05, 0.85), 0.9 - 0.9 * rating / capacity * (end - start - 1))
    return pack_homes(ev, rating, capacity, initial, start, end)


def _with_empty_rows(homes):
    """test_gpu_bound.py's edits: a window of no slot (three residences) and an initial state of charge of 1.2 (two)."""
    h = homes.copy()
    ev = np.flatnonzero(h["ev"] != 0)
    for i in ev[[3, 17, 40]]:
        h["end"][i] = h["start"][i]
    for i in ev[[5, 41]]:
        h["initial"][i] = 1.2
        h["nmin"][i], h["nmax"][i] = 0, -1
    return h


def _sparse_y(rng, M, T, frac=0.05):
    y = np.zeros((M, T))
    mask = rng.random((M, T)) < frac
    y[mask] = rng.choice([-1.0, 1.0], mask.sum()) * rng.uniform(0.05, 3.0, mask.sum())
    return y


def _kernel_case(S, T):
    """Host arrays of one parity case: scenario 0 has the residences with empty rows, scenario 1 a load of its own and
    scale 0, scenario 2 all-zero multipliers; every scenario its own records, multipliers and scale."""
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(N_RES, T, n_nodes=N_NODES, seed=7, binary_feasible=False, stress=1.0)
    w.load, w.cost = f32(w.load), f32(w.cost)
    rng = np.random.default_rng(1000 * S + T)
    homes = [_scenario_records(rng, N_RES, T, s) for s in range(S)]
    homes[0] = _with_empty_rows(homes[0])
    load = np.stack([w.load] * S)
    y = np.stack([_sparse_y(rng, w.M, T) for _ in range(S)])
    scale = np.array([0.5, 0.0, 1.0, 3.0, 0.25, 2.0, 0.75, 1.5, 4.0, 0.125, 1.25][:S])
    if S > 1:
        load[1] = f32(w.load * rng.uniform(0.8, 1.2, w.load.shape))
    if S > 2:
        y[2] = 0.0
    d = np.stack([w.Rn.T @ y[s] for s in range(S)])
    lsum = np.zeros((S, w.M, T))
    for s in range(S):
        np.add.at(lsum[s], w.node_of, load[s])
    vlo, vhi = w.vlow ** 2 - w.vset ** 2, w.vhigh ** 2 - w.vset ** 2
    return w, homes, load, y, d, lsum, scale, vlo, vhi


def _restatements(case, integral):
    from bound_ref import dual_bound
    w, homes, load, y, d, lsum, scale, vlo, vhi = case
    return [dual_bound(w.cost, homes[s], load[s], w.node_of, w.Rn, y[s], scale[s], vlo, vhi, integral=integral, d=d[s])[:3]
            for s in range(len(homes))]


@pytest.mark.parametrize("S,T", SHAPES)
def test_kernel_equals_the_single_call_bit_for_bit(gpu_lib, S, T):
    import torch
    from revs_admm_amd._lib import check, ptr
    lib = gpu_lib
    case = _kernel_case(S, T)
    w, homes, load, y, d, lsum, scale, vlo, vhi = case
    n, M = N_RES, w.M
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    cost, node_of = up(w.cost.astype(np.float32)), up(w.node_of.astype(np.int32))
    bytes_of = lambda h: h.view(np.uint8).reshape(len(h), 32)
    # the ensemble's layout: records [n][S], columns s T + t of double[M][S T]
    cols = lambda a: up(a.transpose(1, 0, 2).reshape(M, S * T))
    hd = up(np.stack([bytes_of(h) for h in homes], axis=1).reshape(n * S, 32))
    d_d, y_d, l_d, sc_d = cols(d), cols(y), cols(lsum), up(scale)
    assert int(lib.revs_dual_bound_many_scratch(n, S, T)) == S * int(lib.revs_dual_bound_scratch(n, T))
    scratch = torch.zeros(int(lib.revs_dual_bound_many_scratch(n, S, T)), **f64)
    out = torch.zeros(S, 4, **f64)
    # contiguous copies of each scenario for the single call
    one = [(up(bytes_of(homes[s])), up(d[s]), up(y[s]), up(lsum[s])) for s in range(S)]
    scratch1 = torch.zeros(int(lib.revs_dual_bound_scratch(n, T)), **f64)
    out1 = torch.zeros(4, **f64)
    st = torch.cuda.current_stream(dev).cuda_stream
    for integral in (0, 1):
        got = []
        for rep in range(2):
            out.fill_(float("nan"))
            check(lib.revs_dual_bound_many(n, S, T, ptr(cost), ptr(hd), ptr(node_of), M, ptr(d_d), ptr(y_d), ptr(l_d),
                                           ptr(sc_d), vlo, vhi, integral, ptr(scratch), ptr(out), st), "revs_dual_bound_many")
            got.append(out.cpu().numpy().copy())
        assert got[0].tobytes() == got[1].tobytes(), (integral, got)            # bit-identical from call to call
        refs = _restatements(case, bool(integral))
        for s in range(S):
            h_s, d_s, y_s, l_s = one[s]
            check(lib.revs_dual_bound(n, T, ptr(cost), ptr(h_s), ptr(node_of), M, ptr(d_s), ptr(y_s), ptr(l_s),
                                      float(scale[s]), vlo, vhi, integral, ptr(scratch1), None, ptr(out1), st),
                  "revs_dual_bound")
            single = out1.cpu().numpy()
            assert np.array_equal(got[0][s], single), (integral, s, got[0][s], single)
            ref, parts, empty = refs[s]
            o = got[0][s]
            tot = (o[0] + o[1]) + o[2]
            print(f"S={S} T={T} integral={integral} scenario {s}: relative distance to the restatement {abs(tot - ref) / abs(ref):.2e}")
            assert abs(tot - ref) <= 1e-11 * abs(ref), (integral, s, tot, ref)
            for k, v in zip(("home", "load", "row"), o[:3]):
                assert abs(v - parts[k]) <= 1e-11 * max(abs(parts[k]), abs(ref)), (integral, s, k, v, parts[k])
            assert o[3] == empty == (N_EMPTY if s == 0 else 0), (integral, s, o[3], empty)
    # n_res = 0: the slot-wise terms only -- c . x_s, as the single entry's own n = 0 form gives it
    x = np.random.default_rng(T).uniform(0.0, 5.0, (S, M, T))
    x_d, zero = cols(x), torch.zeros(S, **f64)
    out.fill_(float("nan"))
    check(lib.revs_dual_bound_many(0, S, T, ptr(cost), None, None, M, None, None, ptr(x_d), ptr(zero), vlo, vhi, 0,
                                   ptr(scratch), ptr(out), st), "revs_dual_bound_many")
    many0 = out.cpu().numpy()
    for s in range(S):
        x_s = up(x[s])
        check(lib.revs_dual_bound(0, T, ptr(cost), None, None, M, None, None, ptr(x_s), 0.0, vlo, vhi, 0, ptr(scratch1),
                                  None, ptr(out1), st), "revs_dual_bound")
        single = out1.cpu().numpy()
        assert np.array_equal(many0[s], single), (s, many0[s], single)
        cx = float((w.cost[None, :] * x[s]).sum())
        assert abs(many0[s][1] - cx) <= 1e-12 * cx and many0[s][0] == many0[s][2] == many0[s][3] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------
def _engine_case(S):
    """150 residences on 15 nodes, T = 24, S scenarios of their own EV ownership and rating (scenario 1: its own load),
    explicit sparse multipliers -- zero on scenarios 2, 5, 8 when S = 9 -- and one scale per scenario."""
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    n, T = 150, 24
    # (stress 0.85: every scenario's centralized LP has a solution, with rows binding in the 70 % scenarios)
    w = make_workload(n, T, n_nodes=15, seed=11, binary_feasible=False, stress=0.85)
    w.load, w.cost = f32(w.load), f32(w.cost)
    rng = np.random.default_rng(40 + S)
    homes = [_scenario_records(rng, n, T, s) for s in range(S)]
    load = np.stack([w.load] * S)
    load[1] = f32(w.load * rng.uniform(0.8, 1.2, w.load.shape))
    y = np.stack([_sparse_y(rng, w.M, T, frac=0.08) for _ in range(S)])
    if S == 9:
        y[[2, 5, 8]] = 0.0
    scale = rng.uniform(0.1, 3.0, S)
    scale[0] = 0.0
    return w, homes, load, y, scale


def _central_optima(w, homes, load):
    from oracle import revs_oracle as ro
    return [ro.solve_central_lp(w.cost, ro.homes_from_records(load[s], homes[s]), w.Rn, w.node_of, w.vset, w.vlow,
                                w.vhigh)[3] for s in range(len(homes))]


@pytest.mark.parametrize("S", [3, 9])
def test_ensemble_bounds_and_certificates_equal_one_engine_per_scenario(gpu_lib, S):
    """S = 3: 72 columns.  S = 9: 216 columns, past the 192 of one dense product (the schedules' voltages go through
    column slices of whole scenarios), the multipliers zero on three scenarios."""
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    w, homes, load, y, scale = _engine_case(S)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    assert ens.T == S * 24
    ens.run(3)
    engines = []
    for s in range(S):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        engines.append(e)
    scale_v = max(abs(ens.vlo), abs(ens.vhi))
    lbs = ens.lower_bounds(y, scale)
    at0, at1 = ens.lower_bounds(y, 0.0), ens.lower_bounds(y, 1.0)
    assert lbs.shape == (S,) and lbs.dtype == np.float64
    certs = ens.certificates(multipliers=y, search=False)
    assert len(certs) == S
    for s, e in enumerate(engines):
        one = e.lower_bound(y[s], float(scale[s]))
        print(f"S={S} scenario {s}: lower_bounds {lbs[s]:.12f}, its own engine {one:.12f} ({abs(lbs[s] - one) / abs(one):.2e} relative)")
        assert abs(lbs[s] - one) <= 1e-12 * abs(one), (s, lbs[s], one)
        c, r = certs[s], e.certificate(multipliers=y[s], search=False)
        assert abs(c.lower - r.lower) <= 1e-12 * abs(r.lower), (s, c.lower, r.lower)
        assert abs(c.upper - r.upper) <= 1e-12 * abs(r.upper), (s, c.upper, r.upper)
        assert abs(c.max_violation - r.max_violation) <= 1e-9 * scale_v, (s, c.max_violation, r.max_violation)
        assert (c.empty, c.integral, c.scale) == (r.empty, r.integral, r.scale), (s, c, r)
        assert c.evaluations == 1 and c.ascent_steps == 0
    # ---- the search, in lock-step: weak duality against HiGHS (the data are f32-rounded as the engine holds them)
    opt = _central_optima(w, homes, load)
    searched = ens.certificates(multipliers=y, search=True)
    for s, c in enumerate(searched):
        print(f"S={S} scenario {s}: searched lower {c.lower:.9f} at s = {c.scale:.4f} (L(0) {at0[s]:.9f}, L(1) {at1[s]:.9f}), "
              f"HiGHS {opt[s]:.9f}, upper {c.upper:.9f}, {c.evaluations} batched evaluations")
        assert c.lower >= max(at0[s], at1[s]), (s, c.lower, at0[s], at1[s])
        assert c.lower <= opt[s] * (1 + 1e-9), (s, c.lower, opt[s])
        assert c.evaluations == searched[0].evaluations and c.seconds == searched[0].seconds
        assert c.upper == certs[s].upper and c.max_violation == certs[s].max_violation
        if not y[s].any():
            assert c.scale == 0.0 and c.lower == at0[s]
    # at most 2 + the longest doubling phase (60 at the most) + 48 -- and fewer launches than the scalar searches together
    assert searched[0].evaluations <= 2 + 60 + 48
    scalar = [e.certificate(multipliers=y[s], search=True).evaluations for s, e in enumerate(engines)]
    print(f"S={S}: {searched[0].evaluations} batched evaluations; the scalar searches take {scalar}")
    assert searched[0].evaluations < sum(scalar)


def test_certificates_leave_the_run_untouched(gpu_lib):
    import torch
    from revs_admm_amd.ensemble import AdmmEnsemble
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    state = lambda e: [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)]
    runs = []
    for certify in (False, True):
        e = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
        e.run(5)
        before = state(e)
        if certify:
            certs, lbs = e.certificates(), e.lower_bounds()
            assert len(certs) == 3 and lbs.shape == (3,)
            torch.cuda.synchronize()
            for a, b in zip(before, state(e)):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        e.step()
        torch.cuda.synchronize()
        runs.append(state(e) + [e.iteration])
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert runs[0][5] == runs[1][5] == 6


def test_call_surface_returns_one_certificate_per_scenario(gpu_lib, golden):
    """lpsolver.solve_ADMM_many(return_certificates=True) on the 121144 feeder: the solutions are those of the call
    without the flag, one Certificate per scenario in homes_list order, lower <= upper wherever the schedules are
    feasible."""
    from test_gpu_ensemble import _nx_graph
    from revs_admm_amd.engine import Certificate
    from revs_admm_amd.extract import get_homes_ev_param
    from revs_admm_amd.lpsolver import solve_ADMM_many
    z, fd = golden
    g = _nx_graph(fd, z)
    res = z["res_id"].tolist()
    all_homes = {h: z["LOAD"][i].tolist() for i, h in enumerate(res)}
    ev = z["dis_a90_r4800_ev_homes"]
    com = z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]
    np.random.seed(56)
    other = np.random.choice(com, int(0.3 * len(com)), replace=False)
    scen = [get_homes_ev_param(all_homes, g, other, 3.6, 20, 0.2, 11, 23),
            get_homes_ev_param(all_homes, g, ev, 4.8, 20, 0.2, 11, 23),
            get_homes_ev_param(all_homes, g, other, 7.2, 20, 0.2, 11, 23)]
    kw = dict(kappa=5.0, iter_max=5, vset=1.03, vlow=0.95, vhigh=1.05)
    plain = solve_ADMM_many(scen, g, z["tariff_shift6"].tolist(), None, **kw)
    sols, certs = solve_ADMM_many(scen, g, z["tariff_shift6"].tolist(), None, return_certificates=True, **kw)
    assert sols == plain and len(sols) == 3
    assert len(certs) == 3 and all(isinstance(c, Certificate) for c in certs)
    for s, c in enumerate(certs):
        print(f"121144 scenario {s}: lower {c.lower:.6f} upper {c.upper:.6f} gap {c.gap:.3e}, max violation "
              f"{c.max_violation:.2e} feasible {c.feasible}, s = {c.scale:.4f}, {c.evaluations} batched evaluations, "
              f"{1e3 * c.seconds:.1f} ms for the three")
        assert c.integral and c.ascent_steps == 0 and c.evaluations == certs[0].evaluations
        tariff = z["tariff_shift6"].astype(np.float32).astype(np.float64)          # (the engine holds it as float)
        cost_s = sum(float(np.dot(tariff, sols[s][1][h])) for h in res)
        assert abs(c.upper - cost_s) <= 1e-9 * cost_s
        if c.feasible:
            assert c.lower <= c.upper
