"""The bill report of an ensemble (bills.py) from the state on the device: every scenario's
bills straight from P_sch on the ensemble's own layout -- float[n][S][T], read through revs_bill_rows' strides, no copy
and no read-back of schedules -- and as the baseline the reference's individual optimum of the very records and loads
the sweep holds, from ONE revs_residence_solve over the n S records.  A method of AdmmEnsemble (mixed in by
ensemble.py); nothing here touches the run's state."""
from __future__ import annotations

import numpy as np
import torch

from . import baselines, bills
from ._lib import check, ptr


class EnsembleBillsMixin:
    def bill_report(self, baseline="individual", groups=None, ev_only=True, arrays=True,
                    baseline_fill="target") -> bills.BillReport:
        """bills.BillReport of the S scenarios' schedules P_sch under the engine's tariff (the float32 prices the sweep
        runs on, widened).

        baseline  "individual": every scenario is compared with the individual optimum of its own records and load
                  (lpsolver.solve_residences on the device: one revs_residence_solve over all n S records).  The report
                  then has 2 S rows: the first S are the ensemble's scenarios, with base[s] = S + s, the last S the
                  baselines' bills, in no group and without a baseline themselves.
                  "uncontrolled" / "last_minute" / "trickle" (baselines.POLICIES): the rule schedule of that name on the
                  same records and loads, filled to `baseline_fill` ("target" / "full"), for the charger of the engine's
                  mode -- ONE revs_rule_schedule over the n S records, its net load only; rows as for "individual".
                  None: bills only, S rows.  An (S, n, T) array in the caller's residence order: uploaded as float64,
                  rows S .. 2S - 1 as above.
        groups    None, or one integer per scenario (S of them): bills.bill_report_device's.
        ev_only   True: the records of scenario s cover the residences that own an EV in scenario s (the reference
                  compares EV residences; a residence without one pays the same under every schedule).
        arrays    False: the records alone are read back.
        bill / dev / keep and worst_index are in the caller's residence order, and every record is bit for bit what
        bills.bill_report gives on result()'s schedules.  The run's state is read, never written."""
        S, n, T = self.S_count, self.n_res, self.T_slot
        named = isinstance(baseline, str)
        individual = named and baseline == "individual"
        if named and not individual and baseline not in baselines.POLICIES:
            raise ValueError(f'bill report: baseline must be "individual", one of {sorted(baselines.POLICIES)}, None or an '
                             f'(S, n, T) array, got {baseline!r}')
        if named and not individual:
            baselines.rule_args(baseline, baseline_fill, self.mode)                      # (before anything is launched)
        if baseline is not None and not named:
            baseline = np.asarray(baseline, np.float64)
            if baseline.shape != (S, n, T):
                raise ValueError(f"bill report: a baseline must be (S, n, T) = {(S, n, T)} in the caller's residence "
                                 f"order, got {baseline.shape}")
        rows = S if baseline is None else 2 * S
        gid, G = bills.check_groups(S, groups)
        base = np.full(rows, -1, np.int32)
        if rows > S:
            base[:S] = S + np.arange(S)
            gid = np.concatenate([gid, np.full(S, -1, np.int32)])
        bills.check_bill_args(rows, n, T, np.zeros(T), base, gid if G else None, None)   # (before anything is launched)
        lib, st, dev = self.lib, self.stream, self.dev
        assert self.cost.numel() == T
        d_tariff = self.cost.double()
        d_bill = torch.empty(rows, n, dtype=torch.float64, device=dev)
        check(lib.revs_bill_rows(S, n, T, ptr(self.P_sch), 0, T, S * T, ptr(d_tariff), ptr(d_bill), st), "revs_bill_rows")
        if individual:
            f32 = dict(dtype=torch.float32, device=dev)
            p, g, soc = torch.empty(n * S, T, **f32), torch.empty(n * S, T, **f32), torch.empty(n * S, T + 1, **f32)
            check(lib.revs_residence_solve(n * S, T, ptr(self.cost), ptr(self.homes), ptr(self.load), ptr(p), ptr(soc),
                                           ptr(g), st), "revs_residence_solve")
            check(lib.revs_bill_rows(S, n, T, ptr(g), 0, T, S * T, ptr(d_tariff), ptr(d_bill[S:]), st), "revs_bill_rows")
        elif named:
            g = baselines.rule_schedule_device(self.homes, self.load, baseline, baseline_fill, self.mode, want="g",
                                               stream=st)[2]
            check(lib.revs_bill_rows(S, n, T, ptr(g), 0, T, S * T, ptr(d_tariff), ptr(d_bill[S:]), st), "revs_bill_rows")
        elif baseline is not None:
            d_base = self._up(baseline[:, self.perm, :])
            check(lib.revs_bill_rows(S, n, T, ptr(d_base), 1, n * T, T, ptr(d_tariff), ptr(d_bill[S:]), st),
                  "revs_bill_rows")
        d_keep = None
        if ev_only:                                # (ev: the first int32 of a 32-byte record; records are [n][S])
            ev = (self.homes.view(torch.int32)[:, 0].view(n, S).t() != 0).to(torch.uint8)
            d_keep = torch.cat([ev] * (rows // S)).contiguous()
        # The bills -- 2 S n doubles, not the schedules -- are put into the caller's residence order on the device before
        # they are summarised: `total` is a sum in a fixed order of the rows, so the records are then bit for bit those
        # of bills.bill_report on result()'s schedules (revs_bill_study's index_of_row would give the caller's
        # worst_index on the engine's order too, but the engine's order of summation).
        inv = self._up(np.asarray(self.inv_perm, np.int64))
        d_bill = d_bill.index_select(1, inv)
        if d_keep is not None:
            d_keep = d_keep.index_select(1, inv)
        return bills.native_bill_study(lib, st, d_bill, base, d_keep, None, gid, G, arrays)
