"""tests/tree_cases.py on the CPU: the inputs of the non-star tree tests are exact -- the integer recursion, feeder.py's
numpy restatement of the three prefix sums and the dense R agree bit for bit, every sum stays far below 2^53 -- and they
are not degenerate: subtrees span wavefronts and the middle of the tree, end-order is not preorder.  A restatement with
the end-order gather taken in preorder passes on select_ref.star_forest and fails on every tree here (no GPU)."""
import numpy as np
import pytest

import select_ref as sr
import tree_cases as tc
from revs_admm_amd.feeder import feeder_tree, tree_voltage_host

NODES = (8, 2048, 2056, 4096, 4104, 8192, 8193, 16384)          # what tests/test_gpu_tree_topologies.py uses
UNIT_KINDS = ("chain", "comb", "binary", "caterpillar")
UNIT_SIZES = (1, 257, 2048, 2049, 4097, 8200, 16384)             # tests/test_gpu_select.py's tree sizes


def _tree(c):
    return feeder_tree(*c["forest"], c["checked"])


def _assert_not_degenerate(tr, what):
    n, end, j = int(tr["n"]), tr["end"].astype(np.int64), np.arange(int(tr["n"]))
    ipt = 8 if n <= 8192 else 16
    assert (end - j > 64 * ipt).any(), (what, "no subtree beyond one wavefront's positions")
    # (a chain is the one tree whose end-order IS preorder -- every subtree ends where the chain does: it is here for
    # the depth of its carries and the C[end - 1] lookups, and the other kinds hold the end-order gather)
    assert np.array_equal(tr["eo"], j) == (what[0] == "chain"), (what, "end-order is preorder")
    assert (tr["cle"] != j).any(), (what, "cle is the identity")
    if n > 2048:
        assert ((j < n // 2) & (end > n // 2)).any(), (what, "no subtree across the middle")


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("n", NODES)
def test_integer_recursion_equals_the_prefix_sums(kind, n):
    c = tc.weighted_case(kind, n)
    tr = _tree(c)
    assert tr["n"] == {8193: 8208}.get(n, n)                     # (8193 nodes: the first count padded to 16)
    for inj, want in ((c["p"], c["v"]), (c["y"], c["d"])):
        got = tree_voltage_host(tr, inj * c["checked"][:, None])
        assert np.array_equal(got, want), kind
        assert np.array_equal(tree_voltage_host(tr, inj), want), "unchecked rows inject"
    assert c["widest"] < 2 ** 50 and (c["v"] / sr.G == np.rint(c["v"] / sr.G)).all()
    assert (c["v"][~c["checked"]] == 0).all() and c["v"][c["checked"]].max() > 0
    if n >= 2048:
        _assert_not_degenerate(tr, (kind, n))


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("n", NODES)
def test_weighted_cases_hold_what_they_promise(kind, n):
    c = tc.weighted_case(kind, n)
    parent, edge_r, cons_of = c["forest"]
    m, on, chk = c["m"], c["on"], c["checked"]
    assert len(parent) == n and c["p"].shape == c["y"].shape == c["q"].shape == (m, 3)
    assert (c["wq"] == 0).any() and c["wq"].max() == 64 or n == 8
    rows = cons_of[cons_of >= 0]
    assert len(set(rows)) == len(rows) == on.sum() == m - 5 and on[rows].all() and not (chk & ~on).any()
    assert (c["y"][~chk] == 0).all() and ((c["y"] != 0).sum(axis=0) >= 1).all()
    if n >= 2048:
        assert (parent > np.arange(n)).any(), "no parent behind its child"
        assert 0.1 < (cons_of < 0).mean() < 0.2 and 0.1 < (on & ~chk).sum() / on.sum() < 0.2
        assert (np.diff(rows) < 0).any(), "rows in node order"
        kids = np.bincount(parent[parent >= 0], minlength=n)
        unchecked = np.zeros(n, bool)
        unchecked[cons_of >= 0] = ~chk[rows]
        if kind != "hub":                                        # (a hub has no interior: one root, leaves)
            assert ((cons_of < 0) & (kids > 0) & (parent >= 0)).any(), "no junction in the interior"
            assert (unchecked & (kids > 0) & (parent >= 0)).any(), "no unchecked row in the interior"


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("n", [8, 2048])
def test_integer_recursion_equals_the_dense_product(kind, n):
    """synthetic.radial_R of the same forest, restricted to the checked rows' nodes: R p with every product and sum exact"""
    c = tc.weighted_case(kind, n)
    parent, edge_r, cons_of = c["forest"]
    node = np.flatnonzero((cons_of >= 0) & c["checked"][np.maximum(cons_of, 0)])
    Rn = tc.dense_R(parent, edge_r)[np.ix_(node, node)]
    for inj, want in ((c["p"], c["v"]), (c["y"], c["d"])):
        assert np.array_equal(Rn @ inj[cons_of[node]], want[cons_of[node]]), kind


@pytest.mark.parametrize("kind", UNIT_KINDS)
@pytest.mark.parametrize("M", UNIT_SIZES)
def test_injections_round_trip(kind, M):
    """tree_voltage_host(tree, injections(forest, v)) == v for select_ref.case(M), bit for bit"""
    v = sr.case(M)[0]
    forest = tc.unit_tree(kind, M)
    tr = feeder_tree(*forest, np.ones(M, bool))
    p = tc.injections(forest, v)
    assert np.array_equal(tree_voltage_host(tr, p), v)
    assert np.abs(p).sum(axis=0).max() / sr.G < 2 ** 40          # (every prefix of the injections: exact)
    if M >= 2048:
        _assert_not_degenerate(tr, (kind, M))
        assert (forest[0] > np.arange(M)).any()


@pytest.mark.parametrize("kind,M,split", [("chain", 2048, 0), ("comb", 2048, 0), ("binary", 2048, 0), ("caterpillar", 2048, 0),
                                          ("comb", 2038, 10), ("chain", 255, 10), ("chain", 16384, 0)])
def test_injections_in_integers(kind, M, split):
    """The same round trip through the integer recursion (p on the 2^-11 grid, w = 1 or 0.5 in halves), with its budget."""
    v = sr.case(M)[0][:, :6]
    forest = tc.unit_tree(kind, M, split)
    assert len(forest[0]) == M + split and (forest[2] < 0).sum() == split
    p = tc.injections(forest, v)
    got, widest = tc.exact_voltages(forest, np.ones(M, bool), p, p_bits=11, w_bits=1)
    assert np.array_equal(got, v) and widest < 2 ** 50


@pytest.mark.parametrize("M", [257, 2048, 4097])
def test_a_preorder_gather_passes_on_stars_and_fails_on_trees(M):
    """The negative control: the wrong restatement returns v on star_forest(M) -- the inputs the tree kernels were held
    to bit for bit so far cannot see the end-order gather -- and not on any tree of this module."""
    v = sr.case(M)[0]
    star = feeder_tree(*sr.star_forest(M), np.ones(M, bool))
    assert np.array_equal(tc.tree_voltage_preorder_gather(star, np.array(v)), v)
    for kind in UNIT_KINDS + ("hub",):
        forest = tc.unit_tree(kind, M)
        tr = feeder_tree(*forest, np.ones(M, bool))
        p = tc.injections(forest, v)
        assert np.array_equal(tree_voltage_host(tr, p), v)
        assert np.array_equal(tc.tree_voltage_preorder_gather(tr, p), v) == (kind == "chain"), kind     # (chain: see above)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_a_preorder_gather_fails_on_the_weighted_cases(kind):
    """... and on the forward grid: every kind but the chain, whose end-order is its preorder."""
    for n in (2048, 8193):
        c = tc.weighted_case(kind, n)
        assert np.array_equal(tc.tree_voltage_preorder_gather(_tree(c), c["p"]), c["v"]) == (kind == "chain"), (kind, n)


def test_topologies():
    assert list(tc.chain(4)) == [-1, 0, 1, 2] and list(tc.hub(4)) == [-1, 0, 0, 0]
    assert list(tc.binary(7)) == [-1, 0, 0, 1, 1, 2, 2] and list(tc.caterpillar(7)) == [-1, 0, 1, 2, 0, 1, 2]
    assert list(tc.comb(9, tooth=4)) == [-1, 0, 1, 2, 0, 4, 5, 6, 4]
    rng = np.random.default_rng(0)
    for kind in tc.KINDS:
        a = tc.topology(kind, 300)
        b = tc.relabel(a, rng)
        depth = lambda par: sorted(np.bincount(par[par >= 0], minlength=len(par)))      # the children counts survive
        assert depth(a) == depth(b) and (b > np.arange(300)).any() and len(tc._levels(b)) == 300
