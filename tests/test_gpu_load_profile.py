"""The load-profile report on the GPU (csrc/load_profile_kernels.hip, revs_admm_amd/load_profile.py, DESIGN.md section
3.13): every record of revs_load_profile, through the C ABI and through the Python entries, against the numpy yard-stick
(tests/profile_ref.py) at the smallest shapes at which the mapping can go wrong -- one residence, fewer residences than a
wavefront, more than one chunk, every tile width, both load widths -- against revs_conv_report on the same buffer, and
end to end from the state an engine and an ensemble hold."""
import itertools

import numpy as np
import pytest

import bills_ref as br
import profile_ref as pr

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = F32(7e9)            # fills every gap of a padded layout: no record may see it
GUARD = 64                     # bytes of canary on either side of every output and of the scratch
OUTPUTS = ("slot", "peak", "day", "pooled_slot", "pooled_peak")


class Rep:
    """What revs_load_profile wrote, as numpy arrays (None: that output was NULL)."""


def native(lib, g, classes=None, C=0, above=0.0, index=None, groups=None, pad=0, off=0, layout="nst", want=OUTPUTS):
    """g (S, n, T) float32 on the host -> Rep through the C ABI.  layout "nst": float[n][S][T + pad] (an ensemble's);
    "snt": float[S][n][T + pad].  off: floats between a 256-byte boundary and element 0.  Every gap holds SENTINEL;
    outputs and scratch sit between canaries; the input is compared before and after."""
    import torch
    from revs_admm_amd._lib import BILL_DTYPE, PROFILE_DAY_DTYPE, check, ptr
    S, n, T = g.shape
    W = T + pad
    dev = torch.device("cuda:0")
    wide = np.full((n, S, W) if layout == "nst" else (S, n, W), SENTINEL, F32)
    if layout == "nst":
        wide[:, :, :T] = g.transpose(1, 0, 2)
        stride_s, stride_i = W, S * W
    else:
        wide[:, :, :T] = g
        stride_s, stride_i = n * W, W
    flat = np.concatenate([np.full(off, SENTINEL, F32), wide.reshape(-1), np.full(8, SENTINEL, F32)])
    d_all = torch.from_numpy(flat).to(dev)
    assert d_all.data_ptr() % 256 == 0
    d_g = d_all[off:]
    d_cls = None if classes is None else torch.from_numpy(np.ascontiguousarray(classes, np.uint8)).to(dev)
    d_index = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
    G = 0 if groups is None else int(max(groups)) + 1
    hg = None if groups is None else np.ascontiguousarray(groups, np.int32)
    Q, rec, day = C + 1, BILL_DTYPE.itemsize, PROFILE_DAY_DTYPE.itemsize
    sizes = dict(slot=S * Q * T * rec, peak=S * Q * rec, day=S * Q * day, pooled_slot=G * Q * T * rec, pooled_peak=G * Q * rec)
    nbytes = int(lib.revs_load_profile_scratch(S, n, T, C, G))
    assert nbytes > 0 and nbytes % 16 == 0
    sizes["scratch"] = nbytes
    guarded = lambda nb: torch.full((GUARD + nb + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    bufs = {k: guarded(sizes[k]) for k in sizes if k == "scratch" or (k in want and sizes[k])}
    p = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else None
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib.revs_load_profile(S, n, T, ptr(d_g), stride_s, stride_i, ptr(d_cls), C, ptr(d_index),
                                hg.ctypes.data if G else None, G, float(above), p("slot"), p("peak"), p("day"),
                                p("pooled_slot"), p("pooled_peak"), p("scratch"), st), "revs_load_profile")
    torch.cuda.synchronize()
    assert d_all.cpu().numpy().tobytes() == flat.tobytes()                        # the input is as it was
    out = Rep()
    shapes = dict(slot=(S, Q, T), peak=(S, Q), day=(S, Q), pooled_slot=(G, Q, T), pooled_peak=(G, Q))
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xCD).all() and (h[GUARD + sizes[k]:] == 0xCD).all(), ("canary", k)
        if k != "scratch":
            setattr(out, k, h[GUARD:GUARD + sizes[k]].copy().view(PROFILE_DAY_DTYPE if k == "day" else BILL_DTYPE).reshape(shapes[k]))
    for k in OUTPUTS:
        if k not in bufs:
            setattr(out, k, None)
    return out


def profile(S, n, T, kind, seed=0):
    rng = np.random.default_rng(seed)
    sh = (S, n, T)
    if kind == "mixed":                            # 90 % exact zeros among random positives
        h = rng.uniform(0.0, 2.0, sh) * (rng.random(sh) < 0.1)
    elif kind == "dense":
        h = rng.lognormal(-1.0, 1.0, sh)
    elif kind == "equal":
        h = np.full(sh, 0.37)
    elif kind == "zero":
        h = np.zeros(sh)
    elif kind == "two":
        h = np.where(rng.random(sh) < 0.6, 0.25, 1.5)
    elif kind == "negative":                       # exporting residences: loads of either sign, some exact zeros
        h = rng.normal(0.3, 1.0, sh) * (rng.random(sh) < 0.9)
    elif kind == "awkward":
        # -0.0, denormals, infinities, a negative, and values that share the upper three bytes of their keys
        close = (0.5 + np.arange(256) * 2.0 ** -24).astype(F32)
        assert len(set((close.view(np.uint32) >> 8).tolist())) == 1 and len(set(close.tolist())) == 256
        pool = np.concatenate([close[rng.integers(0, 256, 40)], F32([-0.0, 0.0, 1e-45, 1e-40, -1e-42, np.inf, -np.inf,
                                                                        -1.5, 0.5, 0.5, 3e38])])
        h = pool[rng.integers(0, len(pool), sh)]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(h, F32)


def class_bytes(S, n, C, seed):
    """Random classes with bytes >= C sprinkled in (C itself and 255); with S > 1, class 0 is empty in scenario 1."""
    if C == 0:
        return None
    rng = np.random.default_rng(seed)
    c = rng.integers(0, C, (S, n))
    out = rng.random((S, n)) < 0.1
    c[out] = np.where(rng.random(int(out.sum())) < 0.5, C, 255)
    if S > 1:
        c[1][c[1] == 0] = C - 1 if C > 1 else 255
    return c.astype(np.uint8)


def groups_for(S):
    return {1: None, 3: [0, -1, 0], 9: [0, 0, 1, 1, 2, 2, -1, 3, 3]}[S]


# every n, T, S, C and kind of the issue, not their product; n = 1600 spans four chunks, (5000, 96) chunks and tiles
SHAPES = [(1, 1, 1, 0, "dense"), (2, 5, 3, 1, "mixed"), (63, 24, 1, 2, "mixed"), (257, 96, 1, 2, "dense"),
          (4099, 24, 1, 2, "awkward"), (1600, 24, 3, 2, "mixed"), (257, 192, 1, 4, "dense"), (63, 5, 9, 4, "two"),
          (4099, 1, 1, 0, "negative"), (2, 192, 3, 0, "equal"), (257, 24, 9, 1, "zero"), (63, 96, 3, 4, "negative"),
          (1, 24, 9, 2, "dense"), (4099, 5, 3, 1, "awkward"), (257, 1, 3, 2, "mixed"), (63, 192, 1, 1, "two"),
          (2, 1, 9, 0, "dense"), (1, 96, 1, 4, "mixed"), (257, 5, 1, 0, "negative"), (5000, 96, 1, 2, "dense"),
          (257, 24, 3, 4, "equal")]


def test_the_shapes_cover_every_value_and_three_chunks(gpu_lib):
    chunk = int(gpu_lib.revs_load_profile_chunk())
    assert {s[0] for s in SHAPES} >= {1, 2, 63, 257, 4099} and {s[1] for s in SHAPES} == {1, 5, 24, 96, 192}
    assert {s[2] for s in SHAPES} == {1, 3, 9} and {s[3] for s in SHAPES} == {0, 1, 2, 4}
    assert {s[4] for s in SHAPES} == {"mixed", "dense", "equal", "zero", "two", "awkward", "negative"}
    assert any(n <= 20000 and (n + chunk - 1) // chunk >= 3 for n, *_ in SHAPES)
    assert (1600 + chunk - 1) // chunk >= 3


@pytest.mark.parametrize("n,T,S,C,kind", SHAPES)
def test_records_at_every_shape(gpu_lib, n, T, S, C, kind):
    g = profile(S, n, T, kind, seed=n + T + S + C)
    if kind == "mixed" and T >= 5:
        g[0, :, 2] = np.nan                                   # a slot that is all NaN
        g[S - 1, n // 2, T - 1] = np.nan                      # and a row whose peak is one
    cls = class_bytes(S, n, C, seed=n + C)
    groups = groups_for(S)
    index = np.random.default_rng(n).permutation(n) if n > 1 and C != 1 else None
    pos = g[np.isfinite(g) & (g > 0)]
    above = 0.5 if kind == "awkward" else float(np.median(pos)) if pos.size else 0.0
    assert kind != "awkward" or (g == F32(0.5)).any()          # (above equal to a value that is there: `>` is strict)
    # an ensemble's layout as it stands; a padded one off a 16-byte boundary in the other order; padded and aligned
    for pad, off, layout in ((0, 0, "nst"), (3, 1, "snt"), (4, 4, "nst")):
        rep = native(gpu_lib, g, cls, C, above, index, groups, pad, off, layout)
        pr.check_report(rep, g, cls, C, above, index, groups, what=(n, T, S, C, kind, pad, off, layout))


def test_empty_class_nan_slot_and_close_keys(gpu_lib):
    S, n, T, C = 3, 700, 8, 2
    g = profile(S, n, T, "awkward", seed=5)
    g[1, :, 3] = np.nan
    g[2, :5, 0] = 3.4e38                                       # a tie for the largest value
    cls = class_bytes(S, n, C, seed=6)
    assert not (cls[1] == 0).any() and (cls[0] == 0).any()
    index = np.random.default_rng(7).permutation(n)
    rep = native(gpu_lib, g, cls, C, 0.5, index, [0, 0, 1])
    pr.check_report(rep, g, cls, C, 0.5, index, [0, 0, 1], what="awkward")
    assert (rep.slot[1, 0]["count"] == 0).all() and (rep.slot[1, 0]["worst_index"] == -1).all()
    assert np.isnan(rep.slot[1, 0]["total"]).all() and int(rep.peak[1, 0]["count"]) == 0
    assert int(rep.day[1, 0]["slots"]) == 0 and int(rep.day[1, 0]["peak_slot"]) == -1 and np.isnan(rep.day[1, 0]["energy"])
    assert (rep.slot[1, :, 3]["count"] == 0).all() and int(rep.day[1, 2]["slots"]) == T - 1
    assert int(rep.slot[1, 2, 3]["n_nan"]) == int((cls[1] < C).sum())
    assert int(rep.peak[1, 2]["count"]) == 0                  # every row of scenario 1 holds a NaN
    tied = [i for i in range(5) if cls[2, i] < C]
    assert tied and int(rep.slot[2, 2, 0]["worst_index"]) == min(index[i] for i in tied)


def test_null_outputs_repeatability_and_a_pool_of_one(gpu_lib):
    S, n, T, C = 3, 300, 5, 2
    g = profile(S, n, T, "negative", seed=11)
    cls = class_bytes(S, n, C, seed=12)
    groups = [0, 1, 0]
    full = native(gpu_lib, g, cls, C, 0.1, None, groups)
    again = native(gpu_lib, g, cls, C, 0.1, None, groups)
    for k in OUTPUTS:
        assert getattr(full, k).tobytes() == getattr(again, k).tobytes(), k          # two calls, the same bytes
    # a pool of one scenario repeats that scenario's records byte for byte, total included
    assert full.pooled_slot[1].tobytes() == full.slot[1].tobytes() and full.pooled_peak[1].tobytes() == full.peak[1].tobytes()
    assert full.pooled_slot[0].tobytes() != full.slot[0].tobytes()
    assert (full.pooled_slot[0]["count"] == full.slot[0]["count"] + full.slot[2]["count"]).all()
    for r in range(1, len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, r):
            part = native(gpu_lib, g, cls, C, 0.1, None, groups, want=want)
            for k in OUTPUTS:
                assert (getattr(part, k) is None) == (k not in want)
                if k in want:
                    assert getattr(part, k).tobytes() == getattr(full, k).tobytes(), (want, k)


@pytest.mark.parametrize("n,T,S,C,kind", [(257, 24, 3, 2, "mixed"), (1600, 24, 1, 2, "negative"), (63, 96, 9, 1, "awkward"),
                                          (300, 5, 3, 0, "dense")])
def test_slot_records_against_the_convergence_report(gpu_lib, n, T, S, C, kind):
    """revs_conv_report with K = 1 and S T columns as its scenarios, one call per set: every field of iter_rec but total
    (another order of summation: within the bound) -- and worst_scenario, which there is the column."""
    import torch
    from revs_admm_amd._lib import BILL_DTYPE, check, ptr
    assert S * T <= 4096
    g = profile(S, n, T, kind, seed=n + T)
    cls = class_bytes(S, n, C, seed=3)
    index = np.random.default_rng(4).permutation(n)
    above = 0.5
    rep = native(gpu_lib, g, cls, C, above, index)
    dev = torch.device("cuda:0")
    d_hist = torch.from_numpy(np.ascontiguousarray(g.transpose(1, 0, 2)).reshape(1, n * S * T)).to(dev)
    d_index = torch.from_numpy(index.astype(np.int32)).to(dev)
    cols = S * T
    for q, mask in enumerate(pr.set_masks(cls, C, S, n)):
        keep = np.ascontiguousarray(np.repeat(mask, T, axis=0), np.uint8)            # (S T, n): a mask T times over
        d_keep = torch.from_numpy(keep).to(dev)
        d_iter = torch.empty(cols * BILL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        nb = int(gpu_lib.revs_conv_report_scratch(cols, n, 1, 0))
        d_scratch = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
        check(gpu_lib.revs_conv_report(cols, n, 1, ptr(d_hist), n * cols, ptr(d_keep), ptr(d_index), None, 0, above, 1,
                                       ptr(d_iter), None, None, None, None, ptr(d_scratch),
                                       torch.cuda.current_stream(dev).cuda_stream), "revs_conv_report")
        it = d_iter.cpu().numpy().view(BILL_DTYPE).reshape(S, T)
        mine = rep.slot[:, q, :]
        for k in BILL_DTYPE.names:
            if k == "total":
                x = g.astype(np.float64)
                for s in range(S):
                    for t in range(T):
                        if mine[s, t]["count"]:
                            v = x[s, mask[s], t]
                            v = v[np.isfinite(v)]
                            assert abs(mine[s, t]["total"] - it[s, t]["total"]) <= 2 * v.size * 2.0 ** -53 * np.abs(v).sum()
            elif k == "worst_scenario":
                want = np.where(mine["count"] > 0, np.arange(S)[:, None] * T + np.arange(T)[None, :], -1)
                assert (it[k] == want).all() and (mine[k] == np.where(mine["count"] > 0, np.arange(S)[:, None], -1)).all()
            else:
                assert mine[k].tobytes() == it[k].tobytes(), (q, k)


def _check_against_free(rep, free, what):
    """A method's report against the free function's on the same schedules in the caller's order: every selected field
    bit for bit, totals (and what follows from them) within the summation bound."""
    for name in ("slot", "peak", "pooled_slot", "pooled_peak"):
        a, b = getattr(rep, name), getattr(free, name)
        assert a.shape == b.shape, (what, name)
        for k in a.dtype.names:
            if k != "total":
                assert a[k].tobytes() == b[k].tobytes(), (what, name, k)
        ok = a["count"] > 0
        assert (np.isnan(a["total"]) == ~ok).all()
    assert rep.classes == free.classes and rep.groups.tolist() == free.groups.tolist()


def _bound_totals(rep, g, cls, C, what):
    masks = pr.set_masks(cls, C, *g.shape[:2])
    ref = [pr.slot_records(g, masks, [s], rep.above) for s in range(g.shape[0])]
    for s in range(g.shape[0]):
        for q in range(len(masks)):
            for t in range(g.shape[2]):
                br.check_record(rep.slot[s, q, t], ref[s][q][t], (what, s, q, t))
    pr.check_days(rep.day, rep.slot, rep.peak, what)


def test_engine_end_to_end(gpu_lib):
    from test_gpu_conv import _single
    from revs_admm_amd import load_profile as lp
    w, make = _single()
    e, f = make(), make()
    for x in (e, f):
        x.run_steps(3)
    ev = (w.homes["ev"] != 0).astype(np.int64)
    P = e.result()[0]
    sched = {None: P, "load": w.load, "uncontrolled": e.rule_schedule("uncontrolled").cpu().numpy()[e.inv_perm]}
    for profile_, g in sched.items():
        rep = e.load_profile_report(profile_, above=1.0)
        free = lp.load_profile_report(g, ev, 2, ("without EV", "with EV"), above=1.0)
        assert rep.slot.shape == (1, 3, 24) and rep.classes == ("without EV", "with EV", "all")
        _check_against_free(rep, free, profile_)
        _bound_totals(rep, np.asarray(g, F32)[None], ev[None], 2, profile_)
        # worst_index is in the caller's order
        t = int(rep.day[0, 2]["peak_slot"])
        assert np.asarray(g, F32)[int(rep.slot[0, 2, t]["worst_index"]), t] == F32(rep.slot[0, 2, t]["max"])
    assert (rep.slot[0, 0]["count"] == (ev == 0).sum()).all() and (rep.slot[0, 2]["count"] == len(ev)).all()
    one = e.load_profile_report(e.rule_schedule("last_minute"), classes=None)
    assert one.slot.shape == (1, 1, 24) and one.classes == ("all",)
    own = e.load_profile_report("load", classes=np.arange(300) % 3)
    assert own.slot.shape == (1, 4, 24) and (own.slot[0, 1]["count"] == 100).all()
    with pytest.raises(ValueError, match="profile must be"):
        e.load_profile_report("cheapest")
    with pytest.raises(ValueError, match="classes must be"):
        e.load_profile_report(classes="pv")
    # the state is as it was: the run goes on bit for bit as one that was never asked
    e.step()
    f.step()
    for x, y in zip(e.get_state(), f.get_state()):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(e.result(), f.result()):
        assert x.tobytes() == y.tobytes()


def test_ensemble_end_to_end(gpu_lib):
    from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
    from revs_admm_amd import load_profile as lp
    w = _workload(n=300, n_nodes=30)
    homes = _mixed_scenarios(w, 3)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for x in (a, b):
        x.run_steps(2)
    ev = np.stack([h["ev"] != 0 for h in homes]).astype(np.int64)
    groups = [0, -1, 0]
    load3 = np.broadcast_to(w.load[None], (3,) + w.load.shape)
    sched = {None: b.result()[0], "load": load3,
             "uncontrolled": b.rule_schedule("uncontrolled").permute(1, 0, 2).cpu().numpy()[:, b.inv_perm]}
    for profile_, g in sched.items():
        rep = b.load_profile_report(profile_, groups=groups, above=0.5)
        free = lp.load_profile_report(g, ev, 2, ("without EV", "with EV"), groups=groups, above=0.5)
        assert rep.slot.shape == (3, 3, 24) and rep.pooled_slot.shape == (1, 3, 24) and rep.n_groups == 1
        _check_against_free(rep, free, profile_)
        _bound_totals(rep, np.asarray(g, F32), ev, 2, profile_)
        s, t = 2, int(rep.day[2, 1]["peak_slot"])
        assert np.asarray(g, F32)[s, int(rep.slot[s, 1, t]["worst_index"]), t] == F32(rep.slot[s, 1, t]["max"])
    assert (rep.slot[:, 1, 0]["count"] == ev.sum(1)).all()
    assert rep.peak_change(rep).shape == (3, 3) and (rep.peak_change(rep) == 0).all()
    assert rep.mean().shape == (3, 3, 24) and rep.aggregate().tobytes() == rep.slot["total"].tobytes()
    assert rep.group_day_mean()["peak"].shape == (1, 3)
    np.testing.assert_allclose(rep.group_day_mean()["peak"][0], rep.day["peak"][[0, 2]].mean(0), rtol=1e-15)
    a.step()
    b.step()
    for s in range(3):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
        assert a.multipliers(s).tobytes() == b.multipliers(s).tobytes(), s
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()


def test_study_load_profile_on_both_paths(gpu_lib, golden):
    """REVS.study(load_profile=True) on the 121144 feeder, 2 seeds x {distributed, individual}: the methods' rows, then
    the base load once per case, classes by each row's EV homes, pooled by method -- the yard-stick's records of the
    report's own rows, on the host path and on the device_report path; without the flag the field stays None."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    res = [int(h) for h in z["res_id"]]
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), group_by="method", max_iterations=3, v0=1.03,
                arrays=True, mode="relaxed", bills=True)
    load = f32(z["LOAD"])
    for path in (dict(), dict(device_report=True)):
        labels, rep = fx.study(tariff, all_homes, dist, com, ensemble=True, load_profile=True, **path, **grid)
        lp = rep.load_profile
        rows = rep.load_profile_rows
        assert [r["method"] for r in rows] == ["distributed", "individual"] * 2 + ["load", "load"] and rows[:4] == labels
        assert [r["seed"] for r in rows[4:]] == [1234, 56]
        assert lp.slot.shape == (6, 3, 24) and lp.pooled_slot.shape == (2, 3, 24) and lp.groups.tolist() == [0, 1, 0, 1, -1, -1]
        assert lp.classes == ("without EV", "with EV", "all")
        g = np.concatenate([rep.node_p.astype(F32), np.stack([load, load])])
        ev = np.stack([rep.bills.keep[s] for s in (0, 1, 2, 3, 0, 2)]).astype(np.int64)
        pr.check_report(lp, g, ev, 2, 0.0, None, lp.groups.tolist(), what=("study", tuple(path)))
        # the residences without an EV draw their base load under every method; the schedules change the EV homes' day
        for s in range(4):
            for k in ("median", "max", "count"):
                assert lp.slot[s, 0][k].tobytes() == lp.slot[4 + s // 2, 0][k].tobytes()
        assert (lp.day[:4, 1]["peak"] > lp.day[[4, 4, 5, 5], 1]["peak"]).all()
    plain = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)[1]
    assert plain.load_profile is None and plain.load_profile_rows is None
