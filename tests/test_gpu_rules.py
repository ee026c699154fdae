"""revs_rule_schedule on the GPU, through the C ABI (include/revs_admm_ops.h, "rule schedules"; csrc/rule_kernels.hip):
every policy, fill and charger type on random records plus one of each edge case, bit for bit the numpy restatement
(tests/rules_ref.py); every subset of the outputs gives the same bits; nothing is written beyond the buffers; and the
individual mode's kernel gives the very same powers where its optimum is a rule schedule."""
import numpy as np
import pytest

import rules_ref as rr

pytestmark = pytest.mark.gpu

CANARY = 0x5A17C0DE
PAD = 64                                                         # canary words behind (and before) every buffer
WANTS = ["".join(k for k, b in zip("psgx", bits) if b) for bits in np.ndindex(2, 2, 2, 2) if any(bits)]


class Buffers:
    """The inputs of one case on the device and fresh canary-fenced outputs per call.  shift: every array starts that
    many 4-byte words behind a 16-byte boundary."""

    def __init__(self, lib, homes, load, shift=0):
        import torch
        from revs_admm_amd._lib import HOME_DTYPE
        self.lib, self.torch, self.shift = lib, torch, shift
        self.rows, self.T = load.shape
        self.dev = torch.device("cuda:0")
        words = np.ascontiguousarray(homes).view(np.int32).reshape(-1)
        assert len(words) == self.rows * HOME_DTYPE.itemsize // 4
        self.homes = self.fenced(len(words), torch.int32)
        self.homes[1].copy_(torch.from_numpy(words))
        self.load = self.fenced(load.size, torch.float32)
        self.load[1].copy_(torch.from_numpy(np.ascontiguousarray(load, np.float32).reshape(-1)))

    def fenced(self, n, dtype):
        raw = self.torch.full((PAD + self.shift + n + PAD,), CANARY, dtype=self.torch.int32, device=self.dev)
        view = raw[PAD + self.shift:PAD + self.shift + n].view(dtype)
        assert view.data_ptr() % 16 == 4 * (self.shift % 4)
        return raw, view

    def intact(self, pair):
        raw, view = pair
        n = view.numel()
        lo, hi = raw[:PAD + self.shift].cpu().numpy(), raw[PAD + self.shift + n:].cpu().numpy()
        return len(hi) == PAD and (lo == CANARY).all() and (hi == CANARY).all()

    def run(self, policy, fill, integral, want="psgx"):
        """-> {letter: numpy array} of the outputs wanted; the canaries of every buffer are checked."""
        from revs_admm_amd._lib import check
        torch, rows, T = self.torch, self.rows, self.T
        size = dict(p=rows * T, s=rows * (T + 1), g=rows * T, x=rows)
        out = {k: self.fenced(size[k], torch.int32 if k == "x" else torch.float32) for k in want}
        ptr = lambda k: out[k][1].data_ptr() if k in out else None
        check(self.lib.revs_rule_schedule(rows, T, self.homes[1].data_ptr(), self.load[1].data_ptr(), policy, fill,
                                          integral, ptr("p"), ptr("s"), ptr("g"), ptr("x"),
                                          torch.cuda.current_stream().cuda_stream), "revs_rule_schedule")
        torch.cuda.synchronize()
        for k, pair in list(out.items()) + [("homes", self.homes), ("load", self.load)]:
            assert self.intact(pair), f"canary of {k} overwritten"
        shape = dict(p=(rows, T), s=(rows, T + 1), g=(rows, T), x=(rows,))
        return {k: out[k][1].cpu().numpy().reshape(shape[k]) for k in want}


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {i}: {got[i]!r} against {want[i]!r}")


def check_case(lib, homes, load, shift=0, subsets=True):
    buf = Buffers(lib, homes, load, shift)
    for policy, fill, integral in rr.combos():
        tag = f"rows {len(homes)}, T {load.shape[1]}, policy {policy}, fill {fill}, integral {integral}"
        p, soc, g, status = rr.rule_schedule(homes, load, policy, fill, integral)
        got = buf.run(policy, fill, integral)
        for k, want in (("p", p), ("g", g), ("x", status), ("s", soc)):
            same_bits(got[k], want, f"{tag}: {k}")
        # the state of charge against the recurrence over the powers the kernel wrote: one float32 rounding of a value
        # below 2 (1.2e-7) and the rounded powers over the capacity
        err = np.abs(got["s"] - rr.soc_recurrence(homes, got["p"])).max()
        assert err <= 1e-6, (tag, err)
        again = buf.run(policy, fill, integral)
        for k in "psgx":
            assert again[k].tobytes() == got[k].tobytes(), (tag, k)
        for want in (WANTS if subsets else ()):
            part = buf.run(policy, fill, integral, want)
            assert sorted(part) == sorted(want)
            for k in want:
                assert part[k].tobytes() == got[k].tobytes(), (tag, want, k)


@pytest.mark.parametrize("T", [1, 5, 24, 96, 192])
@pytest.mark.parametrize("rows", [1, 63, 257, 1000])
def test_rule_schedule_is_the_restatement_bit_for_bit(gpu_lib, rows, T):
    rng = np.random.default_rng(1000 * rows + T)
    if rows == 1:
        # one row cannot hold the edge cases: every one of them, and a random record, as a call of its own
        recs = np.concatenate([rr.edge_records(T), rr.random_records(rng, 1, T)])
        for i in range(len(recs)):
            check_case(gpu_lib, recs[i:i + 1], rng.uniform(0.1, 3.0, (1, T)).astype(np.float32), subsets=i < 2)
        return
    homes = rr.records(rng, rows, T)
    load = rng.uniform(0.1, 3.0, (rows, T)).astype(np.float32)
    load[rng.integers(0, rows, 5), rng.integers(0, T, 5)] *= -1.0                # (a net exporter here and there)
    assert len(homes) == rows and (homes["ev"] == 0).any() and (homes["nmax"] < 0).any()
    check_case(gpu_lib, homes, load)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_arrays_off_the_16_byte_boundary(gpu_lib, shift):
    """T % 4 == 0 with buffers (and records) that do not start on a 16-byte boundary: the dword path, the same bits."""
    rng = np.random.default_rng(shift)
    homes = rr.records(rng, 63, 24)
    check_case(gpu_lib, homes, rng.uniform(0.1, 3.0, (63, 24)).astype(np.float32), shift=shift, subsets=False)


def test_every_edge_case_is_what_it_says(gpu_lib):
    """The edge records do hit their cases (T = 24), and the kernel's answer to each is the contract's."""
    from revs_admm_amd.baselines import rule_schedule
    T = 24
    homes = rr.edge_records(T)
    load = np.full((len(homes), T), 0.5, np.float32)
    at = {name: i for i, name in enumerate(rr.EDGE_CASES)}
    r48 = np.float32(4.8)
    p, soc, g, st = rule_schedule(homes, load, "uncontrolled", "target", "binary")
    assert (p[at["no_ev"]] == 0).all() and (soc[at["no_ev"]] == 0).all() and st[at["no_ev"]] == 0
    assert (g[at["no_ev"]] == load[at["no_ev"]]).all()
    assert (p[at["empty_window"]] == 0).all() and st[at["empty_window"]] == 1 and (soc[at["empty_window"]] == np.float32(0.2)).all()
    assert p[at["end_beyond_T"]].tolist() == [0.0] * 22 + [r48] * 2 and st[at["end_beyond_T"]] == 1
    assert p[at["one_slot_at_end"]].tolist() == [0.0] * 23 + [r48] and st[at["one_slot_at_end"]] == 1
    assert (p[at["k_zero"]] == 0).all() and st[at["k_zero"]] == 0 and homes["nmin"][at["k_zero"]] == 0
    assert p[at["k_equals_W"]].tolist() == [0.0] * 21 + [r48] * 3 and st[at["k_equals_W"]] == 0
    assert homes["nmin"][at["k_equals_W"]] == homes["nmax"][at["k_equals_W"]] == 3
    assert p[at["k_above_W"]].tolist() == [0.0] * 22 + [r48] * 2 and st[at["k_above_W"]] == 1
    for name in ("nmax_negative", "nmin_above_nmax"):
        i = at[name]
        assert (p[i] == 0).all() and st[i] == 1 and (soc[i] == homes["initial"][i]).all() and (g[i] == load[i]).all()
    assert homes["nmax"][at["nmax_negative"]] < 0 and homes["nmin"][at["nmin_above_nmax"]] > homes["nmax"][at["nmin_above_nmax"]]
    assert (p[at["rating_zero_rows_open"]] == 0).all() and st[at["rating_zero_rows_open"]] == 0
    # a continuous charger, filled to 100 %: E_hi = 2 rating exactly -> two full slots and a remainder of +0.0
    pc, sc, _, stc = rule_schedule(homes, load, "uncontrolled", "full", "continuous")
    i = at["exact_multiple"]
    assert pc[i].tolist() == [0.0] * 20 + [r48] * 2 + [0.0] * 2 and stc[i] == 0 and sc[i, -1] == 1.0
    assert not np.signbit(pc).any()
    pl = rule_schedule(homes, load, "last_minute", "full", "continuous")[0]
    assert pl[i].tolist() == [0.0] * 22 + [r48] * 2
    pt = rule_schedule(homes, load, "trickle", "full", "continuous")[0]
    assert pt[i].tolist() == [0.0] * 20 + [np.float32(2.4)] * 4
    assert stc[at["rating_zero"]] == 1 and (pc[at["rating_zero"]] == 0).all()
    # uncontrolled, a remainder: 20 kWh from 0.2 to 0.9 at 4.8 kW = 2 slots and 14 - 9.6 kWh in the third
    j = at["end_beyond_T"]
    wide = homes[j:j + 1].copy()
    wide["start"], wide["end"] = 5, 20
    pw, sw, _, sx = rule_schedule(wide, load[:1], "uncontrolled", "target", "continuous")
    assert sx[0] == 0 and pw[0, :5].tolist() == [0.0] * 5 and pw[0, 5:7].tolist() == [r48] * 2
    assert abs(float(pw[0, 7]) - (0.7 * 20 - 2 * 4.8)) < 1e-5 and (pw[0, 8:] == 0).all() and abs(float(sw[0, -1]) - 0.9) < 1e-6


@pytest.mark.parametrize("rows, T", [(1000, 24), (257, 96)])
def test_individual_mode_kernel_gives_the_rule_schedules_on_monotone_tariffs(gpu_lib, rows, T):
    """revs_residence_solve takes the min(nmax, W) cheapest window slots while 0.01 c_t < 0.99 / capacity, ties to the
    earlier slot: its p_out is the ASAP (increasing, flat tariff) / ALAP (decreasing tariff) schedule of on/off
    chargers filled to 100 %, kernel against kernel.  (Records with nmin > nmax have empty rows under the rule
    schedules' contract; the individual mode never reads nmin: they are left out, as in tests/test_rules_host.py.)"""
    from revs_admm_amd.baselines import rule_schedule
    from revs_admm_amd.engine import residence_solve
    rng = np.random.default_rng(rows + T)
    homes = rr.records(rng, rows, T)
    homes = homes[homes["nmin"] <= homes["nmax"]]
    assert len(homes) > rows // 2
    load = rng.uniform(0.1, 3.0, (len(homes), T)).astype(np.float32)
    tariffs = dict(increasing=np.linspace(0.05, 0.9, T), flat=np.full(T, 0.3), decreasing=np.linspace(0.9, 0.05, T))
    for shape, tariff in tariffs.items():
        c = tariff.astype(np.float32)
        assert (0.01 * c.astype(np.float64).max() < 0.99 / homes["capacity"].astype(np.float64)).all()
        p_ind = residence_solve(c, homes, load)[0]
        p_rule = rule_schedule(homes, load, "last_minute" if shape == "decreasing" else "uncontrolled", "full", "binary")[0]
        assert p_ind.any()
        same_bits(p_rule, p_ind, f"{shape} tariff, T {T}")
