"""revs_bill_rows / revs_bill_study and bills.py on the GPU against tests/bills_ref.py: bills and deviations bit for
bit numpy's, the records' counts, extremes, whiskers and worst entries exactly, quartiles within 2 ulps, totals within
the worst case of any summation order.  Every call writes into junk-filled outputs with guard bytes behind them."""
import numpy as np
import pytest

import across_ref as ar
import bills_ref as br

pytestmark = pytest.mark.gpu

GUARD, JUNK = 256, 0xA5


def _out(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), JUNK, dtype=torch.uint8, device="cuda:0")


def _intact(t, nbytes):
    return bool((t[nbytes:] == JUNK).all())


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rows(lib, g, tariff, layout="study"):
    """g (S, n, T) on the host -> bill (S, n) from the device, through the layout asked for."""
    import torch
    S_, n, T = g.shape
    if layout == "study":
        d_g, ss, si = _up(g), n * T, T
    elif layout == "ensemble":
        d_g, ss, si = _up(g.transpose(1, 0, 2)), T, S_ * T
    else:                                                         # rows apart: padding behind every row
        pad = np.full((S_, n, T + 5), np.nan, g.dtype)
        pad[:, :, :T] = g
        d_g, ss, si = _up(pad), n * (T + 5), T + 5
    out, d_tariff = _out(8 * S_ * n), _up(tariff)
    rc = lib.revs_bill_rows(S_, n, T, d_g.data_ptr(), int(g.dtype == np.float64), ss, si, d_tariff.data_ptr(),
                            out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.revs_last_error()
    assert _intact(out, 8 * S_ * n)
    return out[:8 * S_ * n].cpu().numpy().view(np.float64).reshape(S_, n)


def test_rows_bit_for_bit(gpu_lib):
    rng = np.random.default_rng(5)
    for T in (1, 24, 25, 96, 192):
        tariff = rng.uniform(0.05, 0.4, T)
        for n in (1, 63, 65, 257, 1025):
            for S in (1, 3):
                g32 = rng.uniform(-3.0, 9.0, (S, n, T)).astype(np.float32)
                for g in (g32, g32.astype(np.float64) * np.pi):
                    want = br.bills(g, tariff)
                    for layout in ("study", "ensemble", "padded"):
                        got = rows(gpu_lib, g, tariff, layout)
                        assert got.tobytes() == want.tobytes(), (T, n, S, g.dtype, layout)


def test_rows_into_a_slice(gpu_lib):
    import torch
    rng = np.random.default_rng(6)
    n, T = 130, 24
    g = rng.uniform(0, 5, (2, n, T)).astype(np.float32)
    tariff = rng.uniform(0.05, 0.4, T)
    buf = _out(8 * 5 * n)
    d_g, d_tariff = _up(g.transpose(1, 0, 2)), _up(tariff)       # (held until the launch is done)
    rc = gpu_lib.revs_bill_rows(2, n, T, d_g.data_ptr(), 0, T, 2 * T, d_tariff.data_ptr(), buf.data_ptr() + 8 * 2 * n, None)
    torch.cuda.synchronize()
    assert rc == 0
    raw = buf.cpu().numpy()
    assert (raw[:8 * 2 * n] == JUNK).all() and (raw[8 * 4 * n:] == JUNK).all()
    assert raw[8 * 2 * n:8 * 4 * n].tobytes() == br.bills(g, tariff).tobytes()


class Rep:
    pass


def study(lib, bill, base, keep=None, ior=None, groups=None, dev_out=True, summary=True, pooled=True, scratch=True):
    """revs_bill_study on junk-filled outputs -> Rep(dev, summary_bill, summary_dev, pooled_bill, pooled_dev, groups,
    n_groups); an output not asked for is None."""
    import torch
    from revs_admm_amd._lib import BILL_DTYPE
    S, n = bill.shape
    gid = np.full(S, -1, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = int(gid.max()) + 1
    pooled = pooled and G > 0
    h_base = np.asarray(base, np.int32)
    d_bill = _up(bill)
    d_keep = None if keep is None else _up(np.asarray(keep, np.uint8))
    d_ior = None if ior is None else _up(np.asarray(ior, np.int32))
    o_dev = _out(8 * S * n) if dev_out else None
    o_sum = _out(96 * 2 * S) if summary else None
    o_pool = _out(96 * 2 * G) if pooled else None
    nb = lib.revs_bill_study_scratch(S, n)
    assert nb == 8 * S * n
    o_scr = _out(nb) if scratch else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.revs_bill_study(S, n, d_bill.data_ptr(), h_base.ctypes.data, p(d_keep), p(d_ior),
                             gid.ctypes.data if G else None, G, p(o_dev), p(o_sum), p(o_pool), p(o_scr), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.revs_last_error()
    for t, nbytes in ((o_dev, 8 * S * n), (o_sum, 96 * 2 * S), (o_pool, 96 * 2 * G), (o_scr, nb)):
        assert t is None or _intact(t, nbytes)
    r = Rep()
    r.dev = None if o_dev is None else o_dev[:8 * S * n].cpu().numpy().view(np.float64).reshape(S, n)
    rec = None if o_sum is None else o_sum[:96 * 2 * S].cpu().numpy().view(BILL_DTYPE).reshape(S, 2)
    pool = None if o_pool is None else o_pool[:96 * 2 * G].cpu().numpy().view(BILL_DTYPE).reshape(G, 2)
    r.summary_bill, r.summary_dev = (None, None) if rec is None else (rec[:, 0], rec[:, 1])
    r.pooled_bill, r.pooled_dev = (None, None) if pool is None else (pool[:, 0], pool[:, 1])
    r.groups, r.n_groups = gid, G
    return r


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def same_numbers(a, b):
    """Bit for bit where the values are numbers, NaNs in the same places (IEEE leaves a NaN's sign and payload open:
    0.0 / 0.0 is 0xFFF8... on the host and 0x7FF8... on the device)."""
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())


def grid_values(rng, shape, spread=40):
    """Values on a 2^-10 grid around 1: ties are the rule."""
    return 1.0 + rng.integers(-spread, spread + 1, shape) / 1024.0


def check(lib, bill, base, keep=None, ior=None, groups=None, what=""):
    r = study(lib, bill, base, keep, ior, groups)
    dev = br.deviations(bill, base)
    assert same_numbers(r.dev, dev), what
    br.check_report(r, bill, dev, keep, ior, what)
    return r


def test_deviations_bit_for_bit(gpu_lib):
    rng = np.random.default_rng(7)
    bill = rng.uniform(-2.0, 30.0, (5, 300))
    bill[1, 5] = 0.0             # a zero baseline bill: +-inf or NaN, as IEEE has it
    bill[0, 5] = 3.0
    bill[1, 6] = bill[2, 6] = 0.0
    bill[1, 7] = np.nan
    bill[3, 8] = np.nan
    bill[1, 9] = -0.0
    base = [1, 1, -1, 0, 3]      # (scenario 1 is its own base; 2 has none; 4's base has a base itself)
    r = study(gpu_lib, bill, base, summary=False, pooled=False, scratch=False)
    want = br.deviations(bill, base)
    assert same_numbers(r.dev, want)
    assert np.isnan(want[2]).all() and (want[1][np.isfinite(want[1])] == 0.0).all() and np.isinf(want[0, 5])
    assert np.isnan(want[1, 5]) and np.isnan(want[0, 7]) and np.isnan(want[3, 8]) and np.isnan(want[4, 8])


def test_records_small_counts(gpu_lib):
    """Kept counts 0, 1, 2, 3, 4, 5, 8, 12: every remainder of (count - 1) e mod 4, and the empty record."""
    rng = np.random.default_rng(8)
    S, n = 8, 12
    bill = grid_values(rng, (S, n), 6)
    keep = np.zeros((S, n), bool)
    for s, k in enumerate((0, 1, 2, 3, 4, 5, 8, 12)):
        keep[s, rng.permutation(n)[:k]] = True
    r = check(gpu_lib, bill, [7, 7, 0, 0, -1, 4, 5, 7], keep, None, [0, 0, 1, 1, 2, 2, 3, 3], "small counts")
    assert r.summary_bill["count"].tolist() == [0, 1, 2, 3, 4, 5, 8, 12]
    assert r.pooled_bill["count"].tolist() == [1, 5, 9, 20]
    assert r.summary_dev["count"][4] == 0 and r.summary_dev["worst_scenario"][4] == -1


def test_records_special_values(gpu_lib):
    """Negatives, -0.0 beside +0.0, infinities and NaNs among the bills; a scenario with nothing kept; caller-side
    indices that reverse the rows."""
    rng = np.random.default_rng(9)
    S, n = 6, 777
    bill = grid_values(rng, (S, n)) - 1.0                        # around zero: both signs, exact zeros
    bill[0, ::7] = -0.0
    bill[0, 1::7] = 0.0
    bill[1, 3] = np.inf
    bill[2, 4] = -np.inf
    bill[2, 9:12] = np.nan
    bill[4] = -np.abs(bill[4]) - 0.25                            # a scenario of negatives only
    bill[5] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)         # zeros of both signs alone
    keep = rng.random((S, n)) < 0.7
    keep[3] = False
    ior = np.arange(n)[::-1].copy()
    r = check(gpu_lib, bill, [1, 0, 0, 0, 2, 4], keep, ior, [0, 0, 1, 1, 1, 2], "special values")
    assert r.summary_bill["count"][3] == 0 and r.summary_bill["n_nan"][3] == 0 and r.summary_bill["n_nan"][2] > 0
    assert r.summary_bill["max"][5] == 0.0 and not np.signbit(r.summary_bill["max"][5])
    assert not np.signbit(r.summary_bill["min"][5]) and r.summary_bill["n_above"][5] == 0
    # the worst of all-equal values: the lowest caller-side index, which is the LAST kept row here
    assert r.summary_bill["worst_index"][5] == ior[np.flatnonzero(keep[5])].min()
    check(gpu_lib, bill, [1, 0, 0, 0, 2, 4], None, None, [0, 0, 1, 1, 1, 2], "special values, everything kept")


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_records_around_the_workgroup_width(gpu_lib, n):
    rng = np.random.default_rng(n)
    bill = grid_values(rng, (3, n), 300) * 7.0
    keep = rng.random((3, n)) < 0.9
    r = check(gpu_lib, bill, [2, 0, -1], keep, rng.permutation(n), [0, 1, 0], f"n={n}")
    # a pool of one scenario equals that scenario's summary in every field
    assert same_bits(r.pooled_bill[1], r.summary_bill[1]) and same_bits(r.pooled_dev[1], r.summary_dev[1])


def test_records_across_a_mask_word(gpu_lib):
    rng = np.random.default_rng(10)
    S, n = 65, 37
    bill = grid_values(rng, (S, n))
    groups = np.full(S, -1)
    groups[[63, 64]] = 0
    groups[[1, 2, 62]] = 1
    groups[64 - 1 - 3] = 2                                      # (a pool of one)
    base = (np.arange(S) + 64) % S
    r = check(gpu_lib, bill, base, rng.random((S, n)) < 0.8, None, groups, "S=65")
    assert r.pooled_bill["worst_scenario"][0] in (63, 64)
    assert same_bits(r.pooled_dev[2], r.summary_dev[60]) and same_bits(r.pooled_bill[2], r.summary_bill[60])


def test_records_more_groups_than_one_launch(gpu_lib):
    """S = 449: 8 mask words a group, 56 groups a launch -- 60 groups take two; the deviations take two launches too."""
    rng = np.random.default_rng(11)
    S, n = 449, 5
    bill = grid_values(rng, (S, n), 4)
    base = rng.integers(-1, S, S)
    r = check(gpu_lib, bill, base, None, None, np.arange(S) % 60, "S=449")
    assert (r.pooled_bill["count"] >= 7 * n).all()


def test_records_indices_above_65535(gpu_lib):
    rng = np.random.default_rng(12)
    S, n = 2, 70000
    bill = grid_values(rng, (S, n), 500)
    top = bill.max() + 1.0
    bill[1, 66000] = bill[1, 69999] = bill[0, 65537] = top
    keep = np.ones((S, n), bool)
    keep[0, 65537] = False
    r = check(gpu_lib, bill, [1, -1], keep, None, [0, 0], "n=70000")
    assert (r.pooled_bill["worst_scenario"][0], r.pooled_bill["worst_index"][0]) == (1, 66000)
    ior = np.arange(n)[::-1].copy()
    r = check(gpu_lib, bill, [1, -1], keep, ior, [0, 0], "n=70000, reversed")
    assert (r.pooled_bill["worst_scenario"][0], r.pooled_bill["worst_index"][0]) == (1, 0)


def test_golden_schedules(gpu_lib, golden):
    """The stored schedules of the 121144 feeder as S = 3 (distributed, centralized, individual) through bills.py."""
    from revs_admm_amd import bills
    from test_bills_host import golden_bills
    P, tariff, ev = golden_bills(golden[0])
    P = P[[0, 2, 1]]
    keep = np.tile(ev, (3, 1))
    want = br.bills(P, tariff)
    for base in ([-1, 0, 0], [2, 2, -1]):
        rep = bills.bill_report(P, tariff, base=base, groups=[0, 1, 1], keep=keep)
        assert same_bits(rep.bill, want) and same_bits(rep.dev, br.deviations(want, base))
        assert rep.base.tolist() == base and rep.n_groups == 2 and same_bits(rep.keep, keep)
        br.check_report(rep, rep.bill, rep.dev, keep, None, base)
        dev32 = bills.bill_report(P.astype(np.float32), tariff, base=base, groups=[0, 1, 1], keep=keep, arrays=False)
        assert dev32.bill is None and dev32.dev is None and dev32.summary_bill["count"].tolist() == [267] * 3
    d = rep.summary_dev[0]                                       # distributed against individual: ties are the rule
    assert (d["count"], d["n_above"], d["median"]) == (267, 126, 0.0) and abs(d["max"] - 33.7678739) < 1e-6
    assert abs(d["q3"] - 0.9312025) < 1e-6
    c = rep.summary_dev[1]                                       # centralized against individual
    assert c["count"] == 267 and c["n_nan"] == 0
    # BillReport.across: per residence across the group's scenarios, against across_ref with T = 1
    got = rep.across()
    vals = np.where(keep, rep.dev, np.nan)[:, :, None]
    ref = ar.across_cells(vals, None, rep.groups, 2, -np.inf, 0.0, 1, ())[:, :, 0]
    ar.check_records(got, ref, "bills across")
    assert got.shape == (2, P.shape[1]) and got["count"][1][ev].tolist() == [1] * 267 and (got["count"][:, ~ev] == 0).all()
    assert got["n_violations"][0][ev].sum() == 126


def test_invariants(gpu_lib):
    rng = np.random.default_rng(13)
    S, n = 4, 1500
    bill = grid_values(rng, (S, n), 100) * 3.0
    keep = rng.random((S, n)) < 0.6
    base, groups = [3, 3, 3, -1], [0, 1, 1, 2]
    a = study(gpu_lib, bill, base, keep, None, groups)
    b = study(gpu_lib, bill, base, keep, None, groups)
    for k in ("dev", "summary_bill", "summary_dev", "pooled_bill", "pooled_dev"):
        assert same_bits(getattr(a, k), getattr(b, k)), k                            # two calls: identical bytes
    assert same_bits(a.pooled_bill[0], a.summary_bill[0]) and same_bits(a.pooled_dev[0], a.summary_dev[0])
    assert same_bits(a.pooled_bill[2], a.summary_bill[3]) and same_bits(a.pooled_dev[2], a.summary_dev[3])
    c = study(gpu_lib, bill, base, keep, None, groups, dev_out=False)                # deviations in the scratch only
    assert c.dev is None
    for k in ("summary_bill", "summary_dev", "pooled_bill", "pooled_dev"):
        assert same_bits(getattr(a, k), getattr(c, k)), k
    # every combination of outputs: what is asked for is what the full call gives (study() checks the guards)
    for dev_out in (True, False):
        for summary in (True, False):
            for pooled in (True, False):
                if not (dev_out or summary or pooled):
                    continue
                r = study(gpu_lib, bill, base, keep, None, groups, dev_out, summary, pooled,
                          scratch=summary or pooled)
                assert r.dev is None or same_bits(r.dev, a.dev)
                assert r.summary_dev is None or (same_bits(r.summary_dev, a.summary_dev) and same_bits(r.summary_bill, a.summary_bill))
                assert r.pooled_dev is None or (same_bits(r.pooled_dev, a.pooled_dev) and same_bits(r.pooled_bill, a.pooled_bill))


@pytest.mark.parametrize("n", [1, 2, 1025])
@pytest.mark.parametrize("case", ["all_equal", "first_digit"])
def test_records_ranks_share_or_part(gpu_lib, n, case):
    """The selection where the three ranks share a prefix through all eight digits (every value equal) and where they
    part at the first (both signs, magnitudes 2^-900 .. 2^900): rows of 1, 2 and 1025 entries, three scenarios in pools
    of two and of one."""
    rng = np.random.default_rng(60 + n)
    if case == "all_equal":
        bill, base = np.full((3, n), 3.25), [1, 0, -1]
    else:
        bill = rng.choice([-1.0, 1.0], (3, n)) * 2.0 ** rng.integers(-900, 901, (3, n)).astype(np.float64)
        base = [-1, -1, -1]                          # (no deviations: their quotients would overflow)
    r = check(gpu_lib, bill, base, None, None, [0, 0, 1], f"{case}, n={n}")
    assert r.pooled_bill["count"].tolist() == [2 * n, n]
    assert same_bits(r.pooled_bill[1], r.summary_bill[2])
    if case == "all_equal":
        for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi"):
            assert (r.pooled_bill[k] == 3.25).all() and (r.summary_bill[k] == 3.25).all(), k
        assert (r.pooled_bill["n_fliers"] == 0).all() and (r.pooled_dev["q1"][0] == 0.0)
    elif n == 1025:
        assert r.pooled_bill["q1"][0] < 0.0 < r.pooled_bill["q3"][0]       # (another sign: another first digit)
