"""tests/select_ref.py on the CPU: its restatement of the candidate-row selection against the other numpy writing of
the same rule (FakeKernels.revs_op_dual_select), and its columns against what their names claim -- so that the GPU
tests of tests/test_gpu_select.py cannot pass on inputs that miss the branch they are named for."""
import numpy as np
import pytest

import select_ref as sr

SIZES = [1, 2, 255, 256, 257, 2048, 2049, 4096, 4097, 16384]
KADDS = [0, 1, 16, 128, 200]
A = 128


def _fake(M, kadd):
    """FakeKernels.revs_op_dual_select (nslab = 1) on case(M): everything it writes."""
    from fake_kernels import FakeKernels
    v, y, pnq, _ = sr.case(M)
    nt = v.shape[1]
    b = dict(vfull=np.full((M, nt), -5.0), cidx=np.full((nt, A), -5, np.int64),
             ccnt=np.full(nt, -5, np.int32), cval=np.full((nt, 3, A), -5.0), stats=np.full((nt, 8), -5.0))
    vs, ys, ps = np.array(v), np.array(y), np.array(pnq)
    p = lambda a: a.ctypes.data
    assert FakeKernels().revs_op_dual_select(M, nt, 1, p(vs), p(ps), p(ys), sr.VLO, sr.VHI, kadd, p(b["vfull"]), None,
                                             None, p(b["cidx"]), p(b["ccnt"]), p(b["cval"]), p(b["stats"]), 9.0,
                                             None) == 0
    return b


@pytest.mark.parametrize("kadd", KADDS)
@pytest.mark.parametrize("M", SIZES)
def test_restatement_equals_the_test_double(M, kadd):
    f, r = _fake(M, kadd), sr.expected(M, kadd)
    np.testing.assert_array_equal(f["vfull"], r["vfull"])
    np.testing.assert_array_equal(f["stats"][:, :4], r["sums"])
    np.testing.assert_array_equal(f["ccnt"], r["ccnt"])
    np.testing.assert_array_equal(f["cidx"], r["cidx"])
    np.testing.assert_array_equal(f["cval"], r["cval"])
    assert (f["stats"][:, 5] == 9.0).all()


def _added(M, kadd, name, amax=A):
    """(rows admitted behind the multipliers, the column's violations) of the named column."""
    v, y, pnq, names = sr.case(M, amax)
    t, r = names.index(name), sr.expected(M, kadd, amax)
    ns, n = int(r["sums"][t, 2]), max(int(r["ccnt"][t]), 0)
    return r["cidx"][t, ns:n], r["viol"][:, t]


@pytest.mark.parametrize("M", SIZES)
def test_columns_are_what_their_names_claim(M):
    v, y, pnq, names = sr.case(M)
    assert len(names) == len(set(names)) == sr.T and v.shape == y.shape == (M, sr.T)
    k = v / sr.G
    assert (k == np.round(k)).all() and np.abs(k).max() < 256
    assert ((y == np.round(y)) & (np.abs(y) <= 8)).all()
    q = pnq[2] / sr.G
    assert (q == np.round(q)).all() and (q <= 0).all() and (pnq[0] == v).all()
    r = sr.expected(M, 16)
    ns, nv = r["sums"][:, 2].astype(int), r["sums"][:, 3].astype(int)
    at = names.index
    assert ns[at("nothing")] == 0 and nv[at("nothing")] == 0 and r["ccnt"][at("nothing")] == 0
    assert nv[at("nv256")] == min(256, M) and nv[at("nv257")] == min(257, M)
    assert len(np.unique(r["viol"][:, at("distinct")])) - (M > 191) == min(M, 191) == nv[at("distinct")]
    for want in (127, 128, 129):
        t = at(f"ns{want}")
        assert ns[t] == min(want, M)
        if M >= 255:
            assert nv[t] == 40
            assert r["ccnt"][t] == {127: 128, 128: 128, 129: -1}[want]
    for i, want in enumerate((0, 3, 60, 100, 125, 8, 1, 128)):
        assert ns[at(f"random{i}_ns{want}")] == min(want, M)
    assert nv[at("all_violated")] == M and ns[at("all_violated")] == 0
    assert nv[at("few_mult_no_viol")] == 0 and ns[at("few_mult_no_viol")] == min(5, M)
    t = at("neg_zero")
    negz = (y[:, t] == 0) & np.signbit(y[:, t])
    assert negz.sum() == min(25, M) and (r["viol"][negz, t] > 0).all() and ns[t] == min(3, M - negz.sum())
    t = at("mult_on_violated")                 # in the head, once, with the sign of y; never among the added rows
    rows = np.flatnonzero(y[:, t])
    assert len(rows) == min(20, M) and (np.abs(np.abs(v[rows, t]) - sr.VHI) == 50 * sr.G).all()
    np.testing.assert_array_equal(r["cidx"][t, :len(rows)], rows)
    np.testing.assert_array_equal(r["cval"][t, 0, :len(rows)], np.sign(y[rows, t]))
    assert not np.isin(r["cidx"][t, len(rows):max(r["ccnt"][t], 0)], rows).any()
    if M >= 255:
        assert (np.sign(v[rows, t]) != np.sign(y[rows, t])).any()          # (a multiplier of the other side's sign)
        t = at("up_down_pairs")
        hi, lo = v[:, t] > sr.VHI, v[:, t] < sr.VLO
        assert hi.sum() == lo.sum() == 60
        np.testing.assert_array_equal(np.sort(r["viol"][hi, t]), np.sort(r["viol"][lo, t]))
        n = int(r["ccnt"][t])
        assert set(r["cval"][t, 0, :n]) == {1.0, -1.0}
        # ties decide who is admitted: in each of these columns at least two admitted rows share their violation with
        # another violated row (admitted or not)
        for kadd in (16, 128):
            for name in ("all_tie", "tie_lanes", "ends", "one_thread"):
                added, viol = _added(M, kadd, name)
                vals, cnt = np.unique(viol[viol > 0], return_counts=True)
                shared = np.isin(viol[added], vals[cnt > 1])
                assert shared.sum() >= 2, (name, kadd)
        added, viol = _added(M, 16, "ends")
        assert set(added[:2]) == {0, M - 1} and viol[0] == viol[M - 1] == viol.max()
        added, viol = _added(M, 16, "tie_lanes")
        top = [r_ for r_ in (5, 6, 69, 261, 5 + 256 * 17, M - 1) if r_ < M]
        assert list(added[:len(top)]) == sorted(top)
        added, viol = _added(M, 128, "all_tie")
        assert list(added) == list(np.flatnonzero(viol > 0)[:128])         # the winners are the lowest rows


def test_one_thread_owns_every_winner_at_16384():
    """M = 16384, kadd = 128: the 64 largest violations of `one_thread` (and of `all_violated`, where nv = M keeps the
    stand-alone kernel off its collected path) sit on the rows r = 5 (7) mod 256 -- one thread's 64 rows, bit 63 of its
    mask included -- in three tied levels."""
    for name, lane in (("one_thread", 5), ("all_violated", 7)):
        added, viol = _added(16384, 128, name)
        assert len(added) == 128
        first = added[:64]
        assert (first % 256 == lane).all() and lane + 256 * 63 in first
        assert len(np.unique(viol[first])) == 3 and viol[first].min() > np.delete(viol, first).max()
    assert 5 + 256 * 63 == 16133


@pytest.mark.parametrize("M", [1, 257, 4097, 16384])
def test_columns_of_the_512_row_lists(M):
    v, y, pnq, names = sr.case(M, 512)
    for kadd in (16, 512, 600):
        r = sr.expected(M, kadd, 512)
        assert r["cidx"].shape == (sr.T, 512) and r["cval"].shape == (sr.T, 3, 512)
        for want, cnt in ((511, 512), (512, 512), (513, -1)):
            t = names.index(f"ns{want}")
            assert r["sums"][t, 2] == min(want, M)
            if M > 600:
                assert r["ccnt"][t] == cnt and r["sums"][t, 3] == 40
        if M == 16384:                          # the last word of the kernel's `taken` bitmap
            added, _ = _added(M, kadd, "ends", 512)
            assert set(added[:2]) == {0, M - 1}


@pytest.mark.parametrize("M", SIZES + [8200])
def test_star_forest_gives_the_node_sums_back(M):
    from revs_admm_amd.feeder import feeder_tree, tree_voltage_host
    v = sr.case(M)[0] if M in SIZES else sr.columns(M)[0]
    par, er, cons = sr.star_forest(M)
    tr = feeder_tree(par, er, cons, np.ones(M, bool))
    assert tr["n"] == {2049: 2056, 4097: 4104, 8200: 8208}.get(M, max(8, -(-M // 8) * 8))
    np.testing.assert_array_equal(tree_voltage_host(tr, np.array(v)), v)
