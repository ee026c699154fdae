"""The scalar rules of csrc/boxplot.h, compiled for the host into tests/boxplot_rules_main.cpp and run as a program of its
own (nothing is loaded into Python), against numpy.percentile (linear) and matplotlib.cbook.boxplot_stats' formulas
restated in numpy (network_ref.box_stats), bit for bit: ordered keys and their round trip, quartiles, whisker limits,
whiskers, fliers, the settled-among-zeros rule.  No GPU.

What this does NOT show: that the header keeps a compiler from fusing a product into the sum behind it.  An x86-64
compiler does not contract 1.5 (q3 - q1) into either limit with or without the header's pragmas (the product has two
uses), so the program prints the same limits either way.  That property is a matter of the gfx950 code: the cases with
a datum exactly on the limit in test_gpu_network.py / test_gpu_study.py, and a reading of the kernels' assembly."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import network_ref as nr
from revs_admm_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def run_rules(tmp_path_factory):
    """-> f(lines): the program's output lines for the request lines."""
    d = tmp_path_factory.mktemp("boxplot_rules")
    exe = str(d / "boxplot_rules")
    subprocess.run([build.hipcc(), "-x", "hip", "--offload-host-only", "-O2", "-std=c++17",
                    "-I", os.path.join(build.ROOT, "include"), "-I", build.CSRC,
                    os.path.join(HERE, "boxplot_rules_main.cpp"), "-o", exe], check=True)

    def run(lines):
        path = str(d / "requests.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def hx(v):
    return f"{np.float64(v).view(np.uint64):016x}"


def same(got_hex, want):
    """bit for bit; any NaN equals any NaN"""
    got = np.uint64(int(got_hex, 16)).view(np.float64)
    want = np.float64(want)
    return (np.isnan(got) and np.isnan(want)) or got.view(np.uint64) == want.view(np.uint64)


def limit_pairs():
    """(q1, q3) from a seed, and which of them give another lower / upper limit when the product is not rounded."""
    rng = np.random.default_rng(20250)
    q = np.sort(rng.uniform(0.2, 1.3, (2000, 2)), axis=1)
    q1, q3 = q[:, 0], q[:, 1]
    iqr = q3 - q1
    lo, hi = q1 - 1.5 * iqr, q3 + 1.5 * iqr
    flo = np.array([float(Fraction(a) - Fraction(3, 2) * Fraction(d)) for a, d in zip(q1, iqr)])
    fhi = np.array([float(Fraction(b) + Fraction(3, 2) * Fraction(d)) for b, d in zip(q3, iqr)])
    return q1, q3, lo, hi, flo != lo, fhi != hi, fhi


def samples():
    rng = np.random.default_rng(77)
    out = []
    for n in (1, 2, 3, 4, 5, 8, 9):                 # every remainder of (k - 1) e mod 4
        out.append(rng.normal(0.0, 3.0, n))
        out.append(-np.abs(rng.normal(0.0, 3.0, n)))
        out.append(np.full(n, 0.7))                  # all equal
        out.append(np.round(rng.uniform(0.0, 2.0, n)))   # ties across the ranks
    out.append(np.array([1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 3.0, 50.0]))
    out.append(np.array([2.0, 2.0, 3.0, 3.0]))      # the rank's value repeats, the next is another
    out.append(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]))
    out.append(np.array([-0.0, -0.0, -0.0]))
    out.append(np.array([-np.inf, 1.0, 2.0, 3.0, np.inf]))
    out.append(np.array([-np.inf, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, np.inf]))
    out.append(np.array([-np.inf, np.inf]))
    out.append(np.array([5e-324, 1e-310, -3e-320, 0.0, 2e-308, -2.2e-308, 7e-315]))
    out.append(np.array([5e-324, 1e-323, 1.5e-323, 2e-323]))
    # a datum exactly on numpy's upper limit where the unrounded product gives a lower one: a whisker, no flier
    q1, q3, _, hi, _, dhi, fhi = limit_pairs()
    picked = 0
    for j in np.flatnonzero(dhi & (fhi < hi))[:8]:
        m = 0.5 * (q1[j] + q3[j])
        out.append(np.array([0.1, 0.15, q1[j], q1[j], m, q3[j], q3[j], hi[j], hi[j]]))
        picked += 1
    assert picked > 0
    return out


def test_quartiles_whiskers_fliers(run_rules):
    xs = samples()
    got = run_rules(["S %d %s" % (x.size, " ".join(hx(v) for v in x)) for x in xs])
    for x, line in zip(xs, got):
        x = x + 0.0                                  # (-0.0 orders and is reported as +0.0)
        with np.errstate(invalid="ignore"):
            b = nr.box_stats(x)
            lo, hi = b["q1"] - 1.5 * (b["q3"] - b["q1"]), b["q3"] + 1.5 * (b["q3"] - b["q1"])
        f = line.split()
        want = (b["q1"], b["median"], b["q3"], lo, hi, b["whisker_lo"], b["whisker_hi"])
        for name, g, w in zip(("q1", "median", "q3", "lim_lo", "lim_hi", "whisker_lo", "whisker_hi"), f, want):
            assert same(g, w), (x, name, g, hx(w))
        assert int(f[7]) == b["n_fliers"], (x, f[7], b["n_fliers"])


def test_datum_on_the_limit_is_a_whisker(run_rules):
    q1, q3, _, hi, _, dhi, fhi = limit_pairs()
    j = int(np.flatnonzero(dhi & (fhi < hi))[0])
    x = np.array([0.1, 0.15, q1[j], q1[j], 0.5 * (q1[j] + q3[j]), q3[j], q3[j], hi[j], hi[j]])
    f = run_rules(["S %d %s" % (x.size, " ".join(hx(v) for v in x))])[0].split()
    assert same(f[6], hi[j]) and int(f[7]) == 0


def test_limits_round_the_product(run_rules):
    """The limits' formula against numpy's, on pairs for which one rounding less gives another limit (so that the pairs
    can tell the two apart wherever a compiler does fuse; this host build does not: see the module's docstring)."""
    q1, q3, lo, hi, dlo, dhi, _ = limit_pairs()
    assert dlo.any() and dhi.any()                   # pairs for which a fused multiply-add gives another limit
    got = run_rules([f"L {hx(a)} {hx(b)}" for a, b in zip(q1, q3)])
    for j, line in enumerate(got):
        g = line.split()
        assert same(g[0], lo[j]) and same(g[1], hi[j]), (q1[j], q3[j], line)


def specials64():
    return np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
                     1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, np.nextafter(1.0, 2.0)])


def test_key_order_double(run_rules):
    rng = np.random.default_rng(5)
    v = rng.integers(0, 2 ** 64, 3000, dtype=np.uint64).view(np.float64)
    v = np.concatenate([v[~np.isnan(v)], rng.normal(0.0, 1.0, 1000), specials64()])
    got = [line.split() for line in run_rules([f"K {hx(a)}" for a in v])]
    key = np.array([int(g[0], 16) for g in got], dtype=np.uint64)
    for a, g in zip(v, got):
        assert same(g[1], a + 0.0), (a, g)           # the round trip; -0.0 comes back as +0.0
    o = np.argsort(v, kind="stable")
    vs, ks = v[o], key[o]
    assert np.array_equal(vs[1:] > vs[:-1], ks[1:] > ks[:-1]) and np.all(ks[1:] >= ks[:-1])


def test_key_order_float(run_rules):
    rng = np.random.default_rng(6)
    u = rng.integers(0, 2 ** 32, 3000, dtype=np.uint32)
    v = u.view(np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)
    v = np.concatenate([v[~np.isnan(v)], rng.normal(0.0, 1.0, 1000).astype(np.float32), sp])
    got = [line.split() for line in run_rules([f"F {int(a.view(np.uint32)):08x}" for a in v])]
    key = np.array([int(g[0], 16) for g in got], dtype=np.uint64)
    for a, g in zip(v, got):
        assert same(g[1], np.float64(a) + 0.0), (a, g)
    assert int(got[len(v) - len(sp)][0], 16) == 0x80000000       # +0.0f: the key the zeros rule names
    o = np.argsort(v, kind="stable")
    vs, ks = v[o], key[o]
    assert np.array_equal(vs[1:] > vs[:-1], ks[1:] > ks[:-1]) and np.all(ks[1:] >= ks[:-1])


def test_settled_among_zeros(run_rules):
    cases = [(r, nneg, nzero) for nneg in (0, 1, 3) for nzero in (0, 1, 4) for r in range(0, 9)]
    got = run_rules(["Z %d %d %d" % c for c in cases])
    for (r, nneg, nzero), line in zip(cases, got):
        s, ans, left, eq = line.split()
        if nneg <= r < nneg + nzero:                 # the r-th smallest is a zero: r - nneg zeros lie below it
            assert (int(s), int(ans, 16), int(left), int(eq)) == (1, 0x80000000, r - nneg, nzero)
        else:
            assert int(s) == 0
