"""Candidate-row selection on every path it is implemented on, against the numpy restatement of tests/select_ref.py,
bit for bit (inputs on the 2^-10 grid: every sum the kernels form is exact, see there; tests/test_select_ref.py checks
on the CPU that the columns are what their names claim).  The 24 columns of one launch are 24 scenarios of the rule;
which branch of csrc/select_body.h a slot takes follows from M and from the column's counts:

  M <= 2048          eager loads (stand-alone body), violations in registers
  2048 < M <= 4096   violations in registers (`inreg`), loaded behind the compaction
  4096 < M <= 16384  rows re-read every round, the taken ones in a 64-bit mask per thread
  nv <= 256          stand-alone body only: candidates collected one per thread (nv256 | nv257: the two sides)
  ns = 127, 128, 129 room for one added row, for none, flagged -1

(a) the dense rows kernel + dual_select_body<true>; (b) the same behind the tiled rows kernel (more than 256 columns);
(c) the tree rows kernels in front of it, handing over through LDS (tree <= 2048 nodes, 3 m doubles fit), through
global memory in the same workgroup (they do not fit) or to a launch of its own (larger trees) -- on the forest of
roots on which R p = p and on a chain, a comb and a balanced tree under random node numbers, where the node sums are
the injections whose tree form is v (tests/tree_cases.py: unit_tree, injections) and the expectations are the same; (d)
dual_select_body<false> inside the residence sweep's launch, fed by the restatement itself; (e) the 512-row lists of
csrc/newton_big.hip.  chain_rows_select_body (the folded chain's own selection) and revs_op_dual_tree_select_model_step
are held to a restatement built on this one, branch by branch, in tests/test_gpu_chain_kv.py (columns:
tests/chain_cases.py); revs_op_dual_select_model_step to its parts in tests/test_gpu_newton.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import select_ref as sr
import tree_cases as tc

pytestmark = pytest.mark.gpu

A, A_BIG, T = 128, 512, sr.T
SIZES = [1, 2, 255, 256, 257, 2048, 2049, 4096, 4097, 16384]
JUNK = -5
SEQ = 11.0


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")       # (a copy: the shared cases are read-only)


def _junk(shape, dtype=None):
    import torch
    return torch.full(shape, JUNK, dtype=dtype or torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _dev(M, amax=A):
    """case(M) on the device (read-only inputs, uploaded once per size)."""
    v, y, pnq, _ = sr.case(M, amax)
    return dict(v=_up(v), y=_up(y), pnq=_up(pnq))


def _lists(nt=T, amax=A):
    """The selection's outputs, filled with junk so that anything it leaves unwritten shows."""
    import torch
    return dict(cidx=_junk((nt, amax), torch.int64), ccnt=_junk((nt,), torch.int32), cval=_junk((nt, 3, amax)),
                stats=_junk((nt, 8)))


def _columns_off(got, want, names):
    """names of the columns (slots) in which two [T][...] arrays differ"""
    bad = (np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1)
    return [names[t % len(names)] for t in np.flatnonzero(bad)]


def _assert_lists(b, exp, names, seq=SEQ, stats=True):
    import torch
    torch.cuda.synchronize()
    g = {k: t.cpu().numpy() for k, t in b.items()}
    for k in ("ccnt", "cidx", "cval"):
        assert np.array_equal(g[k], exp[k]), (k, _columns_off(g[k], exp[k], names))
    if stats:
        assert np.array_equal(g["stats"][:, 0:4], exp["sums"]), _columns_off(g["stats"][:, 0:4], exp["sums"], names)
        assert (g["stats"][:, 5] == seq).all()
        assert (g["stats"][:, [4, 6, 7]] == JUNK).all()          # (not the selection's to write)


def _assert_partials(part, exp, names):
    p = part.cpu().numpy()
    fold = np.concatenate([p[:, :, 0:1].max(axis=0), p[:, :, 1:4].sum(axis=0)], axis=1)
    assert np.array_equal(fold, exp["sums"]), _columns_off(fold, exp["sums"], names)


# ---- (a) dense rows + the stand-alone selection ----------------------------------------------------------------------
@pytest.mark.parametrize("kadd", [0, 1, 16, 128, 200])
@pytest.mark.parametrize("M", SIZES)
def test_dense_rows_and_selection(gpu_lib, M, kadd):
    from revs_admm_amd._lib import check, ptr
    d, exp, names = _dev(M), sr.expected(M, kadd), sr.case(M)[3]
    nblk = int(gpu_lib.revs_op_dual_blocks(M))
    b, vfull, viol, part = _lists(), _junk((M, T)), _junk((M, T)), _junk((nblk, T, 4))
    check(gpu_lib.revs_op_dual_select(M, T, 1, ptr(d["v"]), ptr(d["pnq"]), ptr(d["y"]), sr.VLO, sr.VHI, kadd, ptr(vfull),
                                      ptr(viol), ptr(part), ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]),
                                      ptr(b["stats"]), SEQ, None), "revs_op_dual_select")
    _assert_lists(b, exp, names)
    assert np.array_equal(vfull.cpu().numpy(), exp["vfull"]) and np.array_equal(viol.cpu().numpy(), exp["viol"])
    _assert_partials(part, exp, names)


def test_more_rows_than_the_selection_holds_is_an_error(gpu_lib):
    """M = 16385: one row more than a thread's 64-bit mask covers -- refused, nothing launched, nothing written."""
    from revs_admm_amd._lib import ptr
    M = 16385
    b, vfull, viol, part = _lists(), _junk((M, T)), _junk((M, T)), _junk((256, T, 4))
    v, y, pnq = _junk((M, T)), _junk((M, T)), _junk((3, M, T))
    rc = gpu_lib.revs_op_dual_select(M, T, 1, ptr(v), ptr(pnq), ptr(y), sr.VLO, sr.VHI, 16, ptr(vfull), ptr(viol),
                                     ptr(part), ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]), SEQ, None)
    assert rc != 0 and b"16384" in gpu_lib.revs_last_error()
    import torch
    torch.cuda.synchronize()
    for t in (vfull, viol, part, *b.values()):
        assert (t == JUNK).all()


# ---- (b) more than 256 columns: the tiled rows kernel ----------------------------------------------------------------
def test_tiled_columns(gpu_lib):
    from revs_admm_amd._lib import check, ptr
    M, nt, kadd = 257, 300, 16
    v, y, pnq, names = sr.case(M)
    rep = np.arange(nt) % T
    v, y, pnq = v[:, rep], y[:, rep], np.ascontiguousarray(pnq[:, :, rep])
    exp = sr.restate(v, y, pnq, sr.VLO, sr.VHI, kadd)
    for k in ("cidx", "ccnt", "cval", "sums"):                   # (a repeated column is a repeated answer)
        assert np.array_equal(exp[k], sr.expected(M, kadd)[k][rep])
    nblk = int(gpu_lib.revs_op_dual_blocks(M))
    b, vfull, viol, part = _lists(nt), _junk((M, nt)), _junk((M, nt)), _junk((nblk, nt, 4))
    dv, dy, dp = _up(v), _up(y), _up(pnq)
    check(gpu_lib.revs_op_dual_select(M, nt, 1, ptr(dv), ptr(dp), ptr(dy), sr.VLO, sr.VHI, kadd, ptr(vfull), ptr(viol),
                                      ptr(part), ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]), SEQ,
                                      None), "revs_op_dual_select")
    _assert_lists(b, exp, names)
    assert np.array_equal(vfull.cpu().numpy(), exp["vfull"]) and np.array_equal(viol.cpu().numpy(), exp["viol"])
    _assert_partials(part, exp, names)


# ---- (c) the tree forms in front of the selection --------------------------------------------------------------------
def _device_tree(parent, edge_r, cons_of, m):
    from revs_admm_amd import _lib
    from revs_admm_amd.feeder import feeder_tree
    tr = feeder_tree(parent, edge_r, cons_of, np.ones(m, bool))
    keep = (_up(tr["pack"].view(np.int64)), _up(tr["w"]))
    return _lib.Tree(tr["n"], keep[0].data_ptr(), keep[1].data_ptr()), keep, tr


def _rows_tree(lib, m, nt, tree, pnq, y, kadd, vfull, viol, part, b):
    from revs_admm_amd._lib import check, ptr
    check(lib.revs_op_dual_rows_tree(m, nt, C.byref(tree), ptr(pnq), ptr(y), sr.VLO, sr.VHI, kadd, ptr(vfull), ptr(viol),
                                     ptr(part), None, ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]),
                                     SEQ, 1, None), "revs_op_dual_rows_tree")


FORESTS = ("star", "chain", "comb", "binary")


def _with_forests(cases):
    """every case on every forest; the forest of roots keeps the id the case had before the trees were added"""
    return [pytest.param(*c, f, id="-".join(map(str, c)) + ("" if f == "star" else "-" + f)) for f in FORESTS for c in cases]


def _forest(kind, M):
    return sr.star_forest(M) if kind == "star" else tc.unit_tree(kind, M)


@functools.lru_cache(maxsize=None)
def _dev_pnq(kind, M):
    """case(M)'s node terms with the injections whose tree form on _forest(kind, M) is v in the place of v"""
    if kind == "star":
        return _dev(M)["pnq"]
    v, y, pnq, _ = sr.case(M)
    pnq = pnq.copy()
    pnq[0] = tc.injections(_forest(kind, M), v)
    return _up(pnq)


@pytest.mark.parametrize("M,kadd,forest", _with_forests([(M, kadd) for kadd in (16, 128)
                                                         for M in (1, 257, 2048, 2049, 4097, 8200, 16384)]))
def test_tree_rows_and_selection(gpu_lib, M, kadd, forest):
    """star: R p = p, so the tree kernels judge the same v as the dense path; chain | comb | binary: R p = v by the
    injections of tests/tree_cases.py, through subtrees that span wavefronts.  Up to 2048 nodes (256 x 8
    positions) rows and selection share a workgroup and the rows go through LDS; beyond (512 x 8 at 2049, 1024 x 8 at
    4097, 1024 x 16 at 8200 and 16384) the selection is a launch of its own behind them."""
    d, exp, names = _dev(M), sr.expected(M, kadd), sr.case(M)[3]
    tree, keep, tr = _device_tree(*_forest(forest, M), M)
    b, vfull, viol, part = _lists(), _junk((M, T)), _junk((M, T)), _junk((1, T, 4))
    _rows_tree(gpu_lib, M, T, tree, _dev_pnq(forest, M), d["y"], kadd, vfull, viol, part, b)
    _assert_lists(b, exp, names)
    _assert_partials(part, exp, names)
    if M > 2048:                      # (up to 2048 nodes the rows are staged in LDS: vfull / viol are scratch there)
        assert np.array_equal(vfull.cpu().numpy(), exp["vfull"]) and np.array_equal(viol.cpu().numpy(), exp["viol"])


@pytest.mark.parametrize("kadd,forest", _with_forests([(16,), (128,)]))
def test_tree_rows_hand_over_through_global_memory(gpu_lib, kadd, forest):
    """2048 tree nodes scattered over m = 4500 rows: 3 m doubles do not fit in LDS beside the scan buffer, so rows and
    selection share a workgroup but meet in vfull / viol.  Rows without a position in the tree (y = 0 there) keep
    v = 0 and violation 0 -- whatever the node sums hold at them -- and are never admitted."""
    import torch
    m, n = 4500, 2048
    rng = np.random.default_rng(6)
    v, y, names = sr.columns(m, 1)
    pnq = sr.node_terms(v, 1)
    cons = rng.permutation(m)[:n].astype(np.int64)
    on = np.zeros(m, bool)
    on[cons] = True
    y = np.where(on[:, None], y, 0.0)
    exp = sr.restate(np.where(on[:, None], v, 0.0), y, np.where(on[:, None], pnq, 0.0), sr.VLO, sr.VHI, kadd)
    assert (exp["sums"][:, 3] > 256).any() and (exp["ccnt"] > 0).sum() >= 20 and (exp["ccnt"] >= kadd).any()
    parent, edge_r, cons_of = _forest(forest, n)              # (row r of the forest is row cons[r] of the launch)
    if forest != "star":
        pnq = pnq.copy()
        pnq[0][cons] = tc.injections((parent, edge_r, cons_of), v[cons])
    tree, keep, tr = _device_tree(parent, edge_r, cons[cons_of], m)
    z = lambda: torch.zeros(m, T, dtype=torch.float64, device="cuda:0")
    b, vfull, viol, part = _lists(), z(), z(), _junk((1, T, 4))
    _rows_tree(gpu_lib, m, T, tree, _up(pnq), _up(y), kadd, vfull, viol, part, b)
    _assert_lists(b, exp, names)
    _assert_partials(part, exp, names)
    assert np.array_equal(vfull.cpu().numpy(), exp["vfull"]) and np.array_equal(viol.cpu().numpy(), exp["viol"])
    for t in range(T):
        assert on[exp["cidx"][t, :max(exp["ccnt"][t], 0)]].all()


# ---- (d) the selection inside the residence sweep's launch -----------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(gpu_lib):
    """A small sweep (600 residences on 60 nodes, continuous chargers) and what revs_agent_step_out leaves of it."""
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import check, ptr
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(600, T, n_nodes=60, seed=9, binary_feasible=False, stress=1.0)
    n = w.N
    rng = np.random.default_rng(4)
    order = np.argsort(w.node_of, kind="stable")
    s = dict(n=n, homes=_up(w.homes[order].view(np.uint8).reshape(n, _lib.HOME_DTYPE.itemsize)),
             load=_up(w.load[order].astype(np.float32)), node32=_up(w.node_of[order].astype(np.int32)),
             cost=_up(w.cost.astype(np.float32)))
    for k in ("pe", "pen", "ps"):
        s[k] = _up(rng.uniform(0, 3, (n, T)).astype(np.float32))
    s["gm"] = _up(rng.normal(0, 1, (n, T)).astype(np.float32))
    s["pd"] = _lib.PDHG()
    gpu_lib.revs_pdhg_defaults(C.byref(s["pd"]))

    def outs():
        f32 = dict(dtype=torch.float32, device="cuda:0")
        return dict(ps=torch.zeros(n, T, **f32), g=torch.zeros(n, T, **f32), diff=torch.zeros(n, **f32),
                    dsq=torch.zeros(n, **f32), status=torch.zeros(n, dtype=torch.int32, device="cuda:0"))
    s["outs"] = outs
    s["common"] = lambda o: (n, T, ptr(s["cost"]), ptr(s["homes"]), ptr(s["load"]), ptr(s["pe"]), ptr(s["pen"]),
                             ptr(s["ps"]), ptr(s["gm"]), ptr(o["ps"]), ptr(o["g"]), None, None, ptr(o["diff"]),
                             ptr(o["dsq"]), ptr(o["status"]), None, 5.0, 1, C.byref(s["pd"]))
    s["ref"] = outs()
    check(gpu_lib.revs_agent_step_out(*s["common"](s["ref"]), None), "revs_agent_step_out")
    torch.cuda.synchronize()
    assert (s["ref"]["diff"] > 0).any()
    return s


def _sweep_with_selection(lib, s, m, kadd, y, vfull, viol, part, nblk):
    import torch
    from revs_admm_amd._lib import check, ptr
    b, o = _lists(), s["outs"]()
    p_next = torch.zeros(m, T, dtype=torch.float64, device="cuda:0")
    pe2 = torch.zeros(s["n"], T, dtype=torch.float32, device="cuda:0")
    check(lib.revs_agent_step_select(*s["common"](o), m, ptr(part), ptr(y), sr.VLO, sr.VHI, kadd, ptr(vfull), ptr(viol),
                                     ptr(b["cidx"]), ptr(b["ccnt"]), ptr(b["cval"]), ptr(b["stats"]), SEQ,
                                     ptr(s["node32"]), ptr(p_next), ptr(pe2), nblk, None), "revs_agent_step_select")
    torch.cuda.synchronize()
    for k, ref in s["ref"].items():
        assert torch.equal(o[k], ref), k
    assert (p_next[60:] == 0).all() and (p_next[:60] > 0).any()
    return b


@pytest.mark.parametrize("kadd", [16, 128])
@pytest.mark.parametrize("m", [257, 2049, 4097, 16384])
def test_selection_inside_the_sweep(gpu_lib, sweep, m, kadd):
    """dual_select_body<false> on its own: voltages, violations and ONE block of partial sums as the restatement
    writes them (no GPU rows kernel in front), m rows whatever the sweep's 60 nodes.  No eager loads and no collected
    path here: every column with violated rows goes through the scan rounds, with the violations in registers
    (m <= 4096) or behind the mask."""
    d, exp, names = _dev(m), sr.expected(m, kadd), sr.case(m)[3]
    b = _sweep_with_selection(gpu_lib, sweep, m, kadd, d["y"], _up(exp["vfull"]), _up(exp["viol"]),
                              _up(exp["sums"].reshape(1, T, 4)), 1)
    _assert_lists(b, exp, names)


def test_selection_inside_the_sweep_behind_the_rows_kernel(gpu_lib, sweep):
    """sel_nblk = 0: the selection folds the revs_op_dual_blocks(m) blocks revs_op_dual_rows left."""
    from revs_admm_amd._lib import check, ptr
    m, kadd = 4097, 16
    d, exp, names = _dev(m), sr.expected(m, kadd), sr.case(m)[3]
    nblk = int(gpu_lib.revs_op_dual_blocks(m))
    assert nblk == 256
    vfull, viol, part = _junk((m, T)), _junk((m, T)), _junk((nblk, T, 4))
    check(gpu_lib.revs_op_dual_rows(m, T, 1, ptr(d["v"]), ptr(d["pnq"]), ptr(d["y"]), sr.VLO, sr.VHI, ptr(vfull),
                                    ptr(viol), ptr(part), None, None), "revs_op_dual_rows")
    b = _sweep_with_selection(gpu_lib, sweep, m, kadd, d["y"], vfull, viol, part, 0)
    _assert_lists(b, exp, names)
    _assert_partials(part, exp, names)


# ---- (e) the 512-row lists -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kadd", [16, 512, 600])
@pytest.mark.parametrize("M", [1, 257, 4097, 16384])
def test_big_lists(gpu_lib, M, kadd):
    """revs_op_dual_select_big on the restatement's own row arrays; the ns columns carry 511, 512 and 513 multipliers
    (room for one added row, for none, flagged -1 with the whole list padding); `ends` admits row 16383: the last word
    of the kernel's bitmap of taken rows."""
    from revs_admm_amd._lib import check, ptr
    d, exp, names = _dev(M, A_BIG), sr.expected(M, kadd, A_BIG), sr.case(M, A_BIG)[3]
    b, vfull, viol = _lists(T, A_BIG), _up(exp["vfull"]), _up(exp["viol"])
    check(gpu_lib.revs_op_dual_select_big(M, T, ptr(d["y"]), ptr(vfull), ptr(viol), sr.VLO, sr.VHI, kadd, ptr(b["cidx"]),
                                          ptr(b["ccnt"]), ptr(b["cval"]), None), "revs_op_dual_select_big")
    _assert_lists(b, exp, names, stats=False)
    assert (b["stats"] == JUNK).all()
