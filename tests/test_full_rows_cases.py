"""The full-rows PDHG (revs_pdhg_t::full_rows = 1) on the host: the step sizes of ro.pdhg_steps -- the expression the
kernel forms in float -- against the norm of the operator the iteration applies, on every EV residence of the atlas of
tests/window_cases.py; and the conditions tests/test_gpu_full_rows.py rests on, from the float32 restatement alone."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_shapes import EDGES, FULL, RAGGED, shape_of  # noqa: E402
import full_rows_cases as fr  # noqa: E402

HORIZONS = RAGGED + FULL
_IDS = [f"T{T}-{shape_of(T)}" for T in HORIZONS]


def _old_steps(oh):
    """The bound this replaces: the window's triangle alone, the window not clipped to the horizon."""
    Tw = np.maximum(oh.end - oh.start, 1).astype(float)
    nK = np.where(oh.ev, oh.rating / oh.capacity, 1.0) * (2.0 / np.pi) * (Tw + 1.0)
    return 0.25 / nK, 4.0 / nK


@pytest.mark.parametrize("T", HORIZONS, ids=_IDS)
def test_step_sizes_cover_the_operator(T):
    """tau sigma ||K||^2 <= 1 for the K the iteration applies -- delta x (the window's triangle and one row of ones per
    slot behind the window) -- with ||K|| from numpy.linalg.norm(K, 2), on every EV residence, in float64 and in the
    float32 the kernel uses (rounding moves the product by 1e-6; the bound leaves 3e-3).  The triangle's norm alone,
    the earlier bound, does not cover it: most of the atlas' residences sit above 1 there."""
    from oracle import revs_oracle as ro
    a, w, oh = fr.case(T)
    tau, sig, delta = ro.pdhg_steps(oh)
    tau32, sig32, _ = ro.pdhg_steps(oh, dtype=np.float32)
    assert tau32.dtype == np.float32 and np.allclose(tau32, tau, rtol=1e-6) and np.allclose(sig32, sig, rtol=1e-6)
    tau_o, sig_o = _old_steps(oh)
    ev = np.flatnonzero(oh.ev)
    prod, prod32, old = np.zeros(len(ev)), np.zeros(len(ev)), np.zeros(len(ev))
    for k, i in enumerate(ev):
        K = ro.soc_operator(oh, i)
        assert K.shape == (T, fr.wc.clipped(oh.start[i], oh.end[i], T))
        # (the rows the iteration sees: s_{t+1} - initial over the window's slots)
        x = np.random.default_rng(i).uniform(0, 1, T) * oh.window()[i]
        assert np.allclose(K @ x[oh.window()[i]], delta[i] * np.cumsum(x))
        n2 = np.linalg.norm(K, 2) ** 2
        prod[k], prod32[k], old[k] = tau[i] * sig[i] * n2, float(tau32[i]) * float(sig32[i]) * n2, tau_o[i] * sig_o[i] * n2
    print(f"FULLROWS part=steps T={T} shape={shape_of(T)} n_ev={len(ev)} max_product={prod.max():.4f} "
          f"old_bound_max={old.max():.1f} old_bound_above_1={np.mean(old > 1):.2f}")
    assert prod.max() <= 1.0 and prod32.max() <= 1.0
    assert prod.max() > 0.9                   # ... and it is no loose bound: the steps stay as long as the operator allows
    assert np.mean(old > 1) > 0.5 and old.max() > T / 2


@pytest.mark.parametrize("zero", [True, False], ids=["zero", "midrun"])
@pytest.mark.parametrize("T", HORIZONS, ids=_IDS)
def test_restatement_meets_the_gpu_tests_conditions(T, zero):
    """The float32 restatement with the kernel's tolerance (1e-6) and check interval (4), capped at 5000 passes: every
    residence it settles in fewer than 3000 passes lies within 2e-4 x 7.2 kW of ro.home_solve_relaxed
    (tests/test_gpu_agent.py::test_pdhg_full_rows_matches_oracle's bar), and the others are at most 8 % of the
    feasible EV residences (the residences with a single feasible schedule, as tests/test_gpu_windows.py::_capped
    describes them for the presolved form)."""
    a, w, oh = fr.case(T)
    c = fr.classify(T, zero)
    err = np.abs(c["p"] - c["ref"][0]).max(axis=1)
    n_ok, rest = int(c["feasible"].sum()), int((c["between"] | c["capped"]).sum())
    sure = c["sure"]
    print(f"FULLROWS part=classes T={T} shape={shape_of(T)} zero={int(zero)} feasible={n_ok} sure={int(sure.sum())} "
          f"between={int(c['between'].sum())} capped={int(c['capped'].sum())} S_sure={err[sure].max():.3e} "
          f"passes_sure={int(c['passes'][sure].max())}")
    assert n_ok > 100 and np.array_equal(c["feasible"], sure | c["between"] | c["capped"])
    i = int(np.argmax(np.where(sure, err, -1.0)))
    assert err[i] < fr.BAR, f"off by {err[i]:.3e} kW after {c['passes'][i]} passes at {fr.wc.describe(a, i)}"
    assert rest <= 0.08 * n_ok, (rest, n_ok)
    # a flagged residence and one without EV get no schedule from ro.home_solve_relaxed: nothing to compare there
    assert (c["ref"][0][~c["feasible"]] == 0).all()


@pytest.mark.parametrize("T", EDGES, ids=[f"T{T}-{shape_of(T)}" for T in EDGES])
def test_generator_windows_settle(T):
    """make_workload's windows (short tails behind the window, rows that rarely bind): no residence needs 3000 passes,
    and every one ends within the bar."""
    w, oh, st, ref, n_it = fr.generator_case(T)
    print(f"FULLROWS part=generator T={T} shape={shape_of(T)} n={len(n_it)} passes={int(n_it.max())}")
    assert (ref[3] == 0).all() and oh.ev.sum() > 50
    assert n_it.max() < fr.SURE, int(n_it.max())


def test_warm_start_continues_the_cold_run():
    """x0 and y0 in the kernel's units: 64 passes, then 64 more from the schedule and the multiplier rows they left
    are the 128 passes of one run to float32 rounding (x0 goes through p = x rating and back)."""
    from oracle import revs_oracle as ro
    T = 29
    a, w, oh = fr.case(T)
    pe_old, _, ps, gm = fr.start(w, T, False)
    kw = dict(tol=-1.0, check=64, dtype=np.float32, full_rows=True)
    p1, _, g1, n1, y1 = ro.home_solve_relaxed_pdhg(w.cost, oh, pe_old, ps, gm, w.kappa, iters=64, **kw)
    p2, _, _, n2, y2 = ro.home_solve_relaxed_pdhg(w.cost, oh, pe_old, ps, gm, w.kappa, iters=128, **kw)
    assert y1.dtype == np.float32 and y1.shape == (len(a.homes), T) and (y1[~oh.ev] == 0).all()
    assert (n1[oh.ev] == 64).all() and (n2[oh.ev] == 128).all() and np.abs(y1).max() > 0
    x0 = (p1 / np.where(oh.ev, oh.rating, 1.0)[:, None]).astype(np.float32)
    p3, _, _, n3, y3 = ro.home_solve_relaxed_pdhg(w.cost, oh, pe_old, ps, gm, w.kappa, iters=64, x0=x0, y0=y1, **kw)
    ok = np.flatnonzero(oh.ev)
    # (p = x rating in double: dividing it back gives x to the last bit or one off; the bar is float32's)
    assert np.abs(p3 - p2)[ok].max() <= 1e-5 and np.abs(y3 - y2)[ok].max() <= 1e-5
    assert not np.array_equal(p1, p2)
