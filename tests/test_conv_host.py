"""The convergence report without a GPU: the numpy yard-stick (tests/conv_ref.py) on the reference's own stored
trajectory of the 121144 feeder, every check of the Python entries raising before the library is loaded, and
run(history="device") on engines over the numpy stand-in of the kernels (tests/fake_kernels.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conv_ref as cr


def golden_history(z):
    """(1, 15, 267) float32: scenario, row, EV residence."""
    d = z["dis_a90_r4800_diff"]
    assert d.shape == (267, 15) and d.dtype == np.float64
    return np.ascontiguousarray(d.T[None], np.float32)


def test_golden_trajectory(golden):
    z, _ = golden
    h = golden_history(z)
    mx = h[0].max(axis=1)
    assert np.allclose(mx[[0, 1, 2, 14]], [1.7224, 0.5425, 0.8573, 0.4966], rtol=0, atol=5e-5)
    eps = 0.5
    it = cr.iteration_records(h, eps)
    assert [r["count"] for r in it[0]] == [267] * 15 and not any(r["n_nan"] for r in it[0])
    # read off the array itself: the residences above 0.5 per row, the residence that holds each row's maximum
    assert [int((h[0, k] > 0.5).sum()) for k in range(15)] == [156, 4, 33, 33, 5, 3, 1, 1, 1, 0, 3, 2, 3, 0, 0]
    assert [r["n_above"] for r in it[0]] == [156, 4, 33, 33, 5, 3, 1, 1, 1, 0, 3, 2, 3, 0, 0]
    assert [r["worst_index"] for r in it[0]] == [int(np.argmax(h[0, k])) for k in range(15)]
    assert [it[0][k]["worst_index"] for k in (0, 1, 14)] == [112, 179, 223]
    assert abs(it[0][0]["box"]["median"] - 0.54684) < 1e-5 and abs(it[0][13]["box"]["median"] - 0.00572) < 1e-5
    maxima = [r["box"]["max"] for r in it[0]]
    # rows 9, 13 and 14 are the only ones within 0.5 (0.4938, 0.4999, 0.4966): the last row above is 12
    assert [k for k in range(15) if maxima[k] <= eps] == [9, 13, 14]
    res = [cr.residence(h[0, :, i], eps) for i in range(267)]
    settles = [r["settle"] for r in res]
    assert cr.run_record(maxima, eps, 8, settles) == dict(converged_at=-1, last_above=12, n_unsettled=0, n_never=111)
    assert cr.run_record(maxima, eps, 1)["converged_at"] == 9 and cr.run_record(maxima, eps, 2)["converged_at"] == 13
    assert cr.run_record(maxima, eps, 3)["converged_at"] == -1
    assert np.bincount(settles, minlength=16).tolist() == [111, 120, 0, 0, 29, 2, 1, 0, 0, 0, 0, 1, 0, 3, 0, 0]
    sr = cr.settle_record(settles, np.arange(267))
    assert (sr["count"], sr["n_above"], sr["total"], sr["worst_index"]) == (267, 156, 302.0, 6)
    assert (sr["box"]["median"], sr["box"]["max"], sr["box"]["n_fliers"]) == (1.0, 13.0, 36)
    assert res[6]["settle"] == 13 and res[6]["n_above"] == int((h[0, :, 6] > 0.5).sum())


def test_yardstick_rules():
    nan, inf = np.nan, np.inf
    h = np.array([[[0.0, 2.0, nan, -0.0], [0.5, 0.5, inf, 0.25], [0.0, 0.5, 0.0, nan]]], np.float32)   # (1, 3, 4)
    it = cr.iteration_records(h, 0.5, index=[3, 2, 1, 0])
    assert [(r["count"], r["n_nan"], r["n_above"]) for r in it[0]] == [(3, 1, 1), (3, 1, 0), (3, 1, 0)]
    assert it[0][1]["worst_index"] == 2 and it[0][0]["worst_index"] == 2      # ties: the lowest caller-side index
    assert not np.signbit(it[0][0]["box"]["min"])
    r = [cr.residence(h[0, :, i], 0.5) for i in range(4)]
    assert [x["settle"] for x in r] == [0, 1, 2, 3] and [x["n_above"] for x in r] == [0, 1, 2, 1]
    assert [x["worst_iteration"] for x in r] == [1, 0, 1, 1] and r[2]["max"] == np.float32(inf)
    assert np.isnan(r[3]["last"]) and r[3]["max"] == np.float32(0.25)
    assert np.isnan(cr.residence(np.array([nan, nan], np.float32), 0.0)["max"])
    # eps is a strict bound for `above`; an empty row is not within eps
    assert cr.run_record([0.5, nan, 0.5, 0.5], 0.5, 2) == dict(converged_at=2, last_above=1, n_unsettled=-1, n_never=-1)
    assert cr.run_record([0.5, 0.5, 0.6], 0.5, 2, [3, 0, 0, 1]) == dict(converged_at=0, last_above=2, n_unsettled=1, n_never=2)
    assert cr.run_record([0.1, 0.6, 0.1], 0.5, 2)["converged_at"] == -1       # broken one row short
    assert cr.run_record([0.1] * 3, 0.5, 4)["converged_at"] == -1             # patience beyond the history
    keep = np.array([[0, 0, 0, 0]], bool)
    e = cr.iteration_records(h, 0.5, keep)[0][0]
    assert (e["count"], e["n_nan"], e["worst_index"]) == (0, 0, -1) and e["box"] is None
    assert cr.settle_record([], [])["count"] == 0


def test_value_errors_before_the_library_is_loaded(monkeypatch):
    import torch
    from revs_admm_amd import _lib, convergence

    def no_load():
        raise AssertionError("the library is loaded before the arguments are checked")
    monkeypatch.setattr(_lib, "load", no_load)
    h = torch.zeros(5, 6)
    bad = [
        (dict(hist=h.double()), "float32 tensor"),
        (dict(hist=h[0]), "float32 tensor"),
        (dict(hist=np.zeros((5, 6), np.float32)), "float32 tensor"),
        (dict(hist=h.t()), "contiguous"),
        (dict(hist=torch.zeros(0, 6)), "empty"),
        (dict(S=4), "no multiple"),
        (dict(S=0), "no multiple"),
        (dict(S=4097, hist=torch.zeros(1, 4097)), "scenarios outside"),
        (dict(eps=-1e-9), "negative or a NaN"),
        (dict(eps=float("nan")), "negative or a NaN"),
        (dict(patience=0), "patience"),
        (dict(patience=1.5), "patience"),
        (dict(S=2, groups=[0]), "groups must be 2 integers"),
        (dict(S=2, groups=[-2, 0]), "groups must be 2 integers"),
        (dict(S=2, groups=[0.5, 0]), "groups must be 2 integers"),
        (dict(S=2, groups=[0, 5000]), "pools"),
        (dict(S=2, keep=np.ones((3, 2))), "keep must be"),
        (dict(keep=np.ones(6)), "keep must be"),
        (dict(index=[0, 1, 2]), "index must be 6 integers"),
        (dict(index=[0, 1, 2, 3, 4, -1]), "index must be 6 integers"),
        (dict(index=np.arange(6.0)), "index must be 6 integers"),
    ]
    for kw, msg in bad:
        args = dict(hist=h, eps=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            convergence.convergence_report_device(**args)
    with pytest.raises(ValueError, match="runs on the GPU"):          # (checked arguments, a tensor on the host)
        convergence.convergence_report_device(h, 0.5, S=2, keep=np.ones((2, 3)), groups=[0, -1], index=None)
    with pytest.raises(ValueError, match=r"\(iterations, residences\)"):
        convergence.convergence_report(np.zeros(4), 0.5)
    with pytest.raises(ValueError, match="negative or a NaN"):
        convergence.convergence_report(np.zeros((4, 3)), -1.0)
    with pytest.raises(ValueError, match="keep must be"):
        convergence.convergence_report(np.zeros((2, 4, 3)), 0.1, keep=np.ones(3))
    with pytest.raises(ValueError, match="scenarios outside"):
        convergence.convergence_report(np.zeros((4097, 1, 1)), 0.1)


def _engine():
    from fake_kernels import FakeKernels
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(60, 12, n_nodes=8, seed=6, stress=1.02)
    w.load, w.cost = f32(w.load), f32(w.cost)
    shuffle = np.random.default_rng(3).permutation(60)               # (so that the sweep order is not the caller's)
    w.node_of, w.load, w.homes = w.node_of[shuffle], w.load[shuffle], w.homes[shuffle]
    return AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                      mode="relaxed_exact", device="cpu", _kernels=FakeKernels())


def test_run_history_device_on_the_stand_in(monkeypatch):
    e, f = _engine(), _engine()
    with pytest.raises(ValueError, match="no history on the device"):
        e.convergence_report(0.1)
    with pytest.raises(ValueError, match='True, False or "device"'):
        e.run(3, history="host")
    with pytest.raises(ValueError, match="2 GB"):
        e.run(10 ** 7, history="device")
    assert e.iteration == 0                                          # (nothing ran)
    k = e.run(6, history="device")
    d = f.run(6)
    assert k == 6 and tuple(e.diff_history.shape) == (6, 60) and e.diff_history.dtype.is_floating_point
    assert not np.array_equal(e.perm, np.arange(60))
    np.testing.assert_array_equal(e.diff_history.numpy()[:, e.inv_perm], d)           # sweep order on the device
    with pytest.raises(ValueError, match="one boolean per residence"):
        e.convergence_report(0.1, keep=np.ones(3))
    with pytest.raises(ValueError, match="runs on the GPU"):         # (the stand-in's tensors live on the host)
        e.convergence_report(0.1)
    assert e.run(2, history=False) == 2 and e.diff_history is None
    assert e.run(2).shape == (2, 60) and e.diff_history is None


def test_entries_exist():
    import inspect
    from revs_admm_amd import lpsolver
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.revs_fixture import REVS
    from revs_admm_amd.study import StudyReport
    assert inspect.signature(AdmmEnsemble.run).parameters["history"].default is True
    assert inspect.signature(AdmmEnsemble.convergence_report).parameters["groups"].default is None
    assert inspect.signature(AdmmEngine.convergence_report).parameters["patience"].default == 8
    assert inspect.signature(lpsolver.solve_ADMM_many).parameters["return_convergence"].default is None
    assert inspect.signature(REVS.study).parameters["convergence"].default is None
    assert StudyReport.__dataclass_fields__["convergence"].default is None
    with pytest.raises(ValueError, match="pass ensemble=True"):
        REVS.study(None, None, None, None, None, (), (), (), convergence=0.1)
