"""The inputs of tests/operator_cases.py cover what they claim to cover, and its comparison rejects
what it is meant to reject -- on the numpy double alone, no GPU.  tests/test_gpu_operator_kernels.py
holds the kernels of csrc/operator_kernels.hip to the same double with the same comparison."""
import numpy as np
import pytest

import operator_cases as oc
from fake_kernels import FakeKernels, g0f, view

T_EDGES = (1, 7, 32, 33, 64, 65, 128, 129, 256)


def _frac(mask):
    return float(np.mean(mask))


@pytest.mark.parametrize("T", T_EDGES)
def test_node_layout(T):
    node_ptr, isn = oc.node_layout(T)
    counts = np.diff(node_ptr)
    hs = 256 // oc.lanes(T)
    assert 18 <= len(counts) <= 22 and node_ptr[0] == 0 and node_ptr.dtype == np.int64
    assert counts[0] == 0 and counts[-1] == 0 and (counts[1:-1] == 0).any()
    want = {c for c in (1, hs - 1, hs, hs + 1, 2 * hs + 3, 49, 130) if c > 0}
    assert want <= set(counts.tolist())
    assert list(counts) != sorted(counts) and list(counts) != sorted(counts, reverse=True)
    assert ((isn == 0) == (counts == 0)).all()
    np.testing.assert_allclose(isn[counts > 0], 1 / np.sqrt(counts[counts > 0]))
    assert [oc.lanes(t) for t in (1, 32, 33, 64, 65, 128, 129, 256)] == [32, 32, 64, 64, 128, 128, 256, 256]


def _all_different(x):
    return len(np.unique(x)) == x.size


def _clip_parts(pre, bs, lo=oc.VLO, hi=oc.VHI):
    return _frac(pre < bs * lo), _frac(pre > bs * hi), _frac((pre > bs * lo) & (pre < bs * hi))


@pytest.mark.parametrize("M,T", [(37, 7), (50, 24), (300, 33), (11, 96), (5, 256)])
@pytest.mark.parametrize("bscale_on", [True, False])
def test_clip_cases_end_at_both_bounds_and_inside(M, T, bscale_on):
    for alpha in (1.6, 1.0):
        for make, zt in ((oc.make_node_update, "usa"), (oc.make_nodefast_update, "zt")):
            a, s = make(M, T, 3, bscale_on, None, alpha)
            pre = alpha * a[zt].sum(axis=0) + (1 - alpha) * a["zv"] + a["yv"] / a["rho_v"][None, :]
            assert min(_clip_parts(pre, oc._bs(a))) >= 0.10, (make.__name__, alpha)
            for name in ("rho_v", "bscale") if bscale_on else ("rho_v",):
                assert _all_different(a[name])
            assert not np.allclose(a[zt][0], a[zt][-1])               # slabs differ
    a, s = oc.make_init_node(M, T, bscale_on)
    assert min(_clip_parts(a["cx"], oc._bs(a))) >= 0.10
    a, s = oc.make_nodefast_feas(M, T, 3, bscale_on, True)
    assert min(_clip_parts(a["v0"].sum(axis=0), oc._bs(a))) >= 0.10


@pytest.mark.parametrize("T", T_EDGES)
def test_home_pass_cases_update_to_both_signs(T):
    for alpha in (1.6, 1.0):
        for a, s, entry in ((*oc.make_home_pass(T, "res", alpha), "revs_op_home_pass"),
                            (*oc.make_home_pass_fused(T, 3, True, alpha), "revs_op_home_pass_fused")):
            ref = oc.run_fake(entry, a, s)
            # after the update z = max(u, 0), y = rho_b min(u, 0), s_b = z + y: sign(s_b) = sign(u)
            assert _frac(ref["sb"] > 0) >= 0.10 and _frac(ref["sb"] < 0) >= 0.10
            assert _frac(a["sb"] > 0) >= 0.10 and _frac(a["sb"] < 0) >= 0.10
            assert _frac(a["g0"] < 0) >= 0.10
            assert _all_different(a["rho_b"]) and _all_different(a["isn"][a["isn"] > 0])
            assert (a["isn"][np.diff(a["node_ptr"]) == 0] == 0).all()
            if entry.endswith("fused"):               # its node update clips on all three sides too
                pre = alpha * a["usa"].sum(axis=0) + (1 - alpha) * a["zv"] + a["yv"] / a["rho_v"][None, :]
                assert min(_clip_parts(pre, oc._bs(a))) >= 0.10
    a, s = oc.make_home_pass(T, "res")
    new = oc.run_fake("revs_op_home_pass", dict(a, res=np.zeros((8, T))), s)["res"]
    ref = oc.run_fake("revs_op_home_pass", a, s)["res"]
    rows = [1, 2, 5, 6, 7]
    if T > 1:
        assert (a["res"][rows] > new[rows]).any() and (a["res"][rows] < new[rows]).any()
    assert (ref[rows] == np.maximum(a["res"][rows], new[rows])).all()
    assert (ref[[0, 3, 4]] == a["res"][[0, 3, 4]]).all() and (a["res"][[0, 3, 4]] > 0).all()


@pytest.mark.parametrize("T", (7, 33, 256))
def test_node_prep_cases_hold_negative_g0(T):
    outs = []
    for preclamp in (0, 1):
        a, s = oc.make_node_prep(T, preclamp, True)
        a = dict(a, **{k: v for k, v in oc.make_node_prep(T, 0, True)[0].items() if k in ("pe", "ps", "gm", "isn")})
        g = g0f(a["pe"], a["ps"], a["gm"], s["kappa"])
        assert _frac(g < 0) >= 0.10
        ref = oc.run_fake("revs_op_node_prep", a, s)
        empty = np.diff(a["node_ptr"]) == 0
        assert np.isposinf(ref["gmin"][empty]).all() and np.isfinite(ref["gmin"][~empty]).all()
        assert (ref["p0"][empty] == 0).all()
        outs.append(ref)
    assert (outs[0]["p0"] != outs[1]["p0"]).any() and (outs[0]["gmin"] != outs[1]["gmin"]).any()
    assert oc.same_bits(outs[0]["g0_out"], outs[1]["g0_out"])        # g0_out is never clamped


@pytest.mark.parametrize("M,T", [(1, 1), (37, 7), (300, 33), (3, 300)])
@pytest.mark.parametrize("fill", ["zero", "above"])
def test_stats_cases_with_and_without_violation(M, T, fill):
    for make, entry in ((oc.make_nodefast_feas, "revs_op_nodefast_feas"),
                        (oc.make_nodefast_finish, "revs_op_nodefast_finish")):
        kw = dict(nslab=3, stats=fill)
        a, s = make(M, T, violate=False, **kw)
        ref = oc.run_fake(entry, a, s)
        assert ref["stats"][0] == a["stats"][0]                      # no violation: as given
        if entry.endswith("feas") or fill == "above":
            assert oc.same_bits(ref["stats"], a["stats"])
        if M * T >= 64:                  # (a single element need not violate)
            a, s = make(M, T, violate=True, **kw)
            ref = oc.run_fake(entry, a, s)
            if fill == "zero":
                assert ref["stats"][0] > 0 and ref["stats"][1] > 0
            else:
                assert oc.same_bits(ref["stats"], a["stats"])        # pre-filled above: stays


def test_res_cases_lie_on_both_sides():
    for a, s, entry, rows in ((*oc.make_node_update(37, 7, 3, True, "fill"), "revs_op_node_update", [0, 3, 4]),
                              (*oc.make_nodefast_update(37, 7, 3, True, "fill"), "revs_op_nodefast_update", [0, 3, 4]),
                              (*oc.make_nodefast_dualres(37, 7, 3, "fill"), "revs_op_nodefast_dualres", [2, 5, 6, 7])):
        new = oc.run_fake(entry, dict(a, res=np.zeros((8, 7))), s)["res"]
        ref = oc.run_fake(entry, a, s)["res"]
        other = [r for r in range(8) if r not in rows]
        assert (a["res"][rows] > new[rows]).any() and (a["res"][rows] < new[rows]).any()
        assert (ref[rows] == np.maximum(a["res"][rows], new[rows])).all()
        assert (ref[other] == a["res"][other]).all() and (new[other] == 0).all()


def test_the_double_compares_equal_to_itself_and_leaves_inputs_alone():
    cases = [("revs_op_g0", oc.make_g0(37, 7)), ("revs_op_init_home", oc.make_init_home(37, 7)),
             ("revs_op_export", oc.make_export(37, 7)), ("revs_aggregate_f32", oc.make_aggregate(33, False)),
             ("revs_op_init_node", oc.make_init_node(37, 7)), ("revs_op_row_scale", oc.make_row_scale(37, 7)),
             ("revs_op_node_w", oc.make_node_w(37, 7)), ("revs_op_node_scale", oc.make_node_scale(37, 7, 3)),
             ("revs_op_node_update", oc.make_node_update(37, 7, 3, True, "fill")),
             ("revs_op_nodefast_scale", oc.make_nodefast_scale(37, 7, 3)),
             ("revs_op_nodefast_update", oc.make_nodefast_update(37, 7, 3, False, "fill")),
             ("revs_op_nodefast_dualres", oc.make_nodefast_dualres(37, 7, 3, "fill")),
             ("revs_op_nodefast_feas", oc.make_nodefast_feas(37, 7, 3)),
             ("revs_op_nodefast_finish", oc.make_nodefast_finish(37, 7, 3)),
             ("revs_op_home_pass", oc.make_home_pass(33, "res")),
             ("revs_op_home_pass", oc.make_home_pass(7, "rhs")),
             ("revs_op_home_pass_fused", oc.make_home_pass_fused(65, 3)),
             ("revs_op_node_prep", oc.make_node_prep(7, 1)), ("revs_op_node_apply", oc.make_node_apply(129, 0))]
    assert {e for e, _ in cases} | {"revs_aggregate_f64"} == set(oc.ARGS)
    for entry, (a, s) in cases:
        ref, got = oc.run_both(entry, a, s)
        assert got is None
        assert oc.compare(entry, a, s, ref, ref) == {"ulp32": 0}
        written = set(oc.bounds(entry, a, s))
        for name, was in a.items():
            if was is not None and name in written and name not in ("zv", "yv", "sb", "rhat", "res", "stats"):
                assert not (ref[name] == oc.SENTINEL).any(), (entry, name)   # outputs are written in full


def test_close_is_the_stated_bound():
    ref = np.array([1.0, -3.0, np.inf])
    S, chain = np.array([2.0, 3.0, 1.0]), np.array([0, 5, 0])
    tol = 2 * (chain + 8) * 2.0 ** -53 * S
    assert oc.close(ref, ref, S, chain)
    assert oc.close(ref + [0.9 * tol[0], -0.9 * tol[1], 0], ref, S, chain)
    assert not oc.close(ref + [1.5 * tol[0], 0, 0], ref, S, chain)
    assert not oc.close(ref + [0, 3 * tol[1], 0], ref, S, chain)
    assert not oc.close(np.array([1.0, -3.0, 1e300]), ref, S, chain)
    assert not oc.close(np.array([1.0, np.nan, np.inf]), ref, S, chain)
    assert oc.close(np.zeros(3), np.zeros(3), 0.0, 0) and not oc.close(np.full(3, 1e-300), np.zeros(3), 0.0, 0)


# ---- one deliberate mistake each: the comparison must refuse it -----------------------------------
class RhoByRow(FakeKernels):
    """rho indexed by row (i / T) instead of by slot (i % T)"""
    @staticmethod
    def _rows(p, m, T):
        rho = view(p, (T,), np.float64)
        mixed = np.ascontiguousarray(np.repeat(rho[np.arange(m) % T][:, None], T, axis=1))
        return mixed

    def revs_op_node_w(self, m, T, zv, yv, rho_v, w, stream):
        d = lambda p: view(p, (m, T), np.float64)
        d(w)[:] = self._rows(rho_v, m, T) * d(zv) - d(yv)
        return 0

    def revs_op_nodefast_scale(self, m, T, nslab, wh, ph0, lam, rho_v, kappa, xh, sx, stream):
        d = lambda p: view(p, (m, T), np.float64)
        l = view(lam, (m,), np.float64)[:, None]
        x = (kappa * d(ph0) + l * view(wh, (nslab, m, T), np.float64).sum(axis=0)) / \
            (kappa + self._rows(rho_v, m, T) * l * l)
        d(xh)[:] = x
        d(sx)[:] = l * x
        return 0

    def revs_op_home_pass(self, m, T, node_ptr, isn, sb, g0, xc, rho_b, kappa, alpha, rhat, cty, res, stream):
        assert not xc                                     # the form without update: rhat only
        node, n = self._seg(m, node_ptr)
        rb = view(rho_b, (T,), np.float64)[node % T][:, None]        # one value per residence row
        SB, G0 = view(sb, (n, T), np.float64), view(g0, (n, T), np.float64)
        acc = np.zeros((m, T))
        np.add.at(acc, node, kappa * G0 + rb * np.maximum(SB, 0) - np.minimum(SB, 0))
        view(rhat, (m, T), np.float64)[:] = view(isn, (m,), np.float64)[:, None] * acc
        return 0


class AlphaOne(FakeKernels):
    def revs_op_home_pass(self, m, T, node_ptr, isn, sb, g0, xc, rho_b, kappa, alpha, *rest):
        return super().revs_op_home_pass(m, T, node_ptr, isn, sb, g0, xc, rho_b, kappa, 1.0, *rest)

    def revs_op_nodefast_update(self, m, T, nslab, zt, rho_v, bscale, alpha, *rest):
        return super().revs_op_nodefast_update(m, T, nslab, zt, rho_v, bscale, 1.0, *rest)

    def revs_op_node_update(self, m, T, nslab, va, rhat, usa, rho_v, rho_b, bscale, kappa, alpha, *rest):
        return super().revs_op_node_update(m, T, nslab, va, rhat, usa, rho_v, rho_b, bscale, kappa, 1.0, *rest)


class LastSlabOut(FakeKernels):
    """the first nslab - 1 slabs of a contiguous [nslab][m][T] array are what nslab - 1 reads"""
    def revs_op_node_scale(self, m, T, nslab, *rest):
        return super().revs_op_node_scale(m, T, nslab - 1, *rest)

    def revs_op_node_update(self, m, T, nslab, *rest):
        return super().revs_op_node_update(m, T, nslab - 1, *rest)

    def revs_op_nodefast_scale(self, m, T, nslab, *rest):
        return super().revs_op_nodefast_scale(m, T, nslab - 1, *rest)

    def revs_op_nodefast_update(self, m, T, nslab, *rest):
        return super().revs_op_nodefast_update(m, T, nslab - 1, *rest)

    def revs_op_nodefast_dualres(self, m, T, nslab, *rest):
        return super().revs_op_nodefast_dualres(m, T, nslab - 1, *rest)

    def revs_op_nodefast_feas(self, m, T, nslab, *rest):
        return super().revs_op_nodefast_feas(m, T, nslab - 1, *rest)

    def revs_op_nodefast_finish(self, m, T, nslab, *rest):
        return super().revs_op_nodefast_finish(m, T, nslab - 1, *rest)


class BoundScaleIgnored(FakeKernels):
    def revs_op_init_node(self, m, T, cx, rho_v, bscale, *rest):
        return super().revs_op_init_node(m, T, cx, rho_v, None, *rest)

    def revs_op_node_update(self, m, T, nslab, va, rhat, usa, rho_v, rho_b, bscale, *rest):
        return super().revs_op_node_update(m, T, nslab, va, rhat, usa, rho_v, rho_b, None, *rest)

    def revs_op_nodefast_update(self, m, T, nslab, zt, rho_v, bscale, *rest):
        return super().revs_op_nodefast_update(m, T, nslab, zt, rho_v, None, *rest)

    def revs_op_nodefast_feas(self, m, T, nslab, v0, bscale, *rest):
        return super().revs_op_nodefast_feas(m, T, nslab, v0, None, *rest)


class ResRow3To4(FakeKernels):
    """the maximum of |usa| (row 3) merged into row 4, that of |z_v| lost"""
    def _swap(self, call, T, res):
        new = np.zeros((8, T))
        rc = call(new.ctypes.data)
        o = view(res, (8, T), np.float64)
        o[0] = np.maximum(o[0], new[0])
        o[4] = np.maximum(o[4], new[3])
        return rc

    def revs_op_node_update(self, m, T, *rest):
        *head, res, stream = rest
        return self._swap(lambda p: FakeKernels.revs_op_node_update(self, m, T, *head, p, stream), T, res)

    def revs_op_nodefast_update(self, m, T, *rest):
        *head, res, stream = rest
        return self._swap(lambda p: FakeKernels.revs_op_nodefast_update(self, m, T, *head, p, stream), T, res)


class IsnOutOfRhat(FakeKernels):
    def revs_op_home_pass(self, m, T, node_ptr, isn, sb, g0, xc, rho_b, kappa, alpha, rhat, cty, res, stream):
        rc = super().revs_op_home_pass(m, T, node_ptr, isn, sb, g0, xc, rho_b, kappa, alpha, rhat, cty, res, stream)
        i = view(isn, (m,), np.float64)[:, None]
        r = view(rhat, (m, T), np.float64)
        r[:] = np.where(i > 0, r / np.where(i > 0, i, 1.0), r)
        return rc


class XcFromNeighbour(FakeKernels):
    def revs_op_home_pass(self, m, T, node_ptr, isn, sb, g0, xc, *rest):
        self._keep = np.ascontiguousarray(np.roll(view(xc, (m, T), np.float64), 1, axis=0))
        return super().revs_op_home_pass(m, T, node_ptr, isn, sb, g0, self._keep.ctypes.data, *rest)


class GminIsMax(FakeKernels):
    def revs_op_node_prep(self, m, T, node_ptr, isn, pe, ps, gm, kappa, preclamp, p0, gmin, g0_out, stream):
        rc = super().revs_op_node_prep(m, T, node_ptr, isn, pe, ps, gm, kappa, preclamp, p0, gmin, g0_out, stream)
        node, n = self._seg(m, node_ptr)
        f = lambda p: view(p, (n, T), np.float32)
        g = g0f(f(pe), f(ps), f(gm), kappa)
        mx = np.full((m, T), -np.inf)
        np.maximum.at(mx, node, np.maximum(g, 0) if preclamp else g)
        view(gmin, (m, T), np.float64)[:] = np.where(np.isfinite(mx), mx, np.inf)
        return rc


MUTANTS = [
    (RhoByRow, "revs_op_node_w", lambda: oc.make_node_w(37, 7)),
    (RhoByRow, "revs_op_nodefast_scale", lambda: oc.make_nodefast_scale(37, 7, 3)),
    (RhoByRow, "revs_op_home_pass", lambda: oc.make_home_pass(33, "rhs")),
    (AlphaOne, "revs_op_home_pass", lambda: oc.make_home_pass(33, "res")),
    (AlphaOne, "revs_op_home_pass_fused", lambda: oc.make_home_pass_fused(33, 3)),
    (AlphaOne, "revs_op_nodefast_update", lambda: oc.make_nodefast_update(37, 7, 3, True, "fill")),
    (AlphaOne, "revs_op_node_update", lambda: oc.make_node_update(37, 7, 3, True, "fill")),
    (LastSlabOut, "revs_op_node_scale", lambda: oc.make_node_scale(37, 7, 3)),
    (LastSlabOut, "revs_op_node_update", lambda: oc.make_node_update(37, 7, 3)),
    (LastSlabOut, "revs_op_home_pass_fused", lambda: oc.make_home_pass_fused(65, 3)),
    (LastSlabOut, "revs_op_nodefast_scale", lambda: oc.make_nodefast_scale(37, 7, 3)),
    (LastSlabOut, "revs_op_nodefast_update", lambda: oc.make_nodefast_update(37, 7, 3)),
    (LastSlabOut, "revs_op_nodefast_dualres", lambda: oc.make_nodefast_dualres(37, 7, 3)),
    (LastSlabOut, "revs_op_nodefast_feas", lambda: oc.make_nodefast_feas(37, 7, 3)),
    (LastSlabOut, "revs_op_nodefast_finish", lambda: oc.make_nodefast_finish(37, 7, 3)),
    (BoundScaleIgnored, "revs_op_init_node", lambda: oc.make_init_node(37, 7)),
    (BoundScaleIgnored, "revs_op_node_update", lambda: oc.make_node_update(37, 7, 3)),
    (BoundScaleIgnored, "revs_op_home_pass_fused", lambda: oc.make_home_pass_fused(7, 1)),
    (BoundScaleIgnored, "revs_op_nodefast_update", lambda: oc.make_nodefast_update(37, 7, 1)),
    (BoundScaleIgnored, "revs_op_nodefast_feas", lambda: oc.make_nodefast_feas(37, 7, 1)),
    (ResRow3To4, "revs_op_node_update", lambda: oc.make_node_update(37, 7, 1, True, "fill")),
    (ResRow3To4, "revs_op_nodefast_update", lambda: oc.make_nodefast_update(37, 7, 1, True, "fill")),
    (IsnOutOfRhat, "revs_op_home_pass", lambda: oc.make_home_pass(7, "rhs")),
    (IsnOutOfRhat, "revs_op_home_pass", lambda: oc.make_home_pass(129, "res")),
    (IsnOutOfRhat, "revs_op_home_pass_fused", lambda: oc.make_home_pass_fused(33, 1)),
    (XcFromNeighbour, "revs_op_home_pass", lambda: oc.make_home_pass(33, "upd")),
    (XcFromNeighbour, "revs_op_home_pass_fused", lambda: oc.make_home_pass_fused(256, 1)),
    (GminIsMax, "revs_op_node_prep", lambda: oc.make_node_prep(33, 0)),
    (GminIsMax, "revs_op_node_prep", lambda: oc.make_node_prep(7, 1)),
]


@pytest.mark.parametrize("mutant,entry,make", MUTANTS, ids=[f"{m.__name__}-{e[5:]}-{i}" for i, (m, e, _) in enumerate(MUTANTS)])
def test_the_comparison_rejects_a_subtly_wrong_kernel(mutant, entry, make):
    a, s = make()
    ref, _ = oc.run_both(entry, a, s)
    bad, _ = oc.run_both(entry, a, s, fake=mutant())
    oc.compare(entry, a, s, ref, ref)
    with pytest.raises(AssertionError, match="outside the rounding bound|off by more"):
        oc.compare(entry, a, s, ref, bad)
    # and by a margin: the mistake moves some written element by 1e-3 S or more
    moved = 0.0
    for name, b in oc.bounds(entry, a, s).items():
        if len(b) == 2:
            S = np.broadcast_to(b[0], ref[name].shape)
            if ((S == 0) & (bad[name] != ref[name])).any():
                moved = np.inf                            # bits were owed
            ok = np.isfinite(ref[name]) & np.isfinite(bad[name]) & (S > 0)
            if ok.any():
                with np.errstate(invalid="ignore"):
                    moved = max(moved, float((np.abs(bad[name] - ref[name])[ok] / S[ok]).max()))
    assert moved >= 1e-3, moved
