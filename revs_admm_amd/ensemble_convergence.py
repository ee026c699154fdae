"""The convergence report of an ensemble (convergence.py) from the history on the device:
run(history="device") leaves every scenario's residuals where the iterations wrote them -- float[iterations][n][S], the
sweep's own layout, which revs_conv_report reads as it is -- and convergence_report() reads back records only.  Methods
of AdmmEnsemble (mixed in by ensemble.py); nothing here touches the run's state."""
from __future__ import annotations

import numpy as np

from . import convergence


class EnsembleConvergenceMixin:
    def _history_on_device(self, history, iter_max):
        """run()'s check of `history` before anything runs -> whether the history stays on the device."""
        self.diff_history = None
        if history is True:
            return False
        if history != "device":
            raise ValueError(f'AdmmEnsemble.run: history must be True or "device", got {history!r}')
        if iter_max * self.n_res * self.S_count * 4 > int(2e9):
            raise ValueError(f'AdmmEnsemble.run: history="device" keeps the history in one piece of at most 2 GB; '
                             f"{iter_max} iterations x {self.n_res} residences x {self.S_count} scenarios x 4 bytes "
                             f"are more")
        return True

    def convergence_report(self, eps, patience=8, groups=None, keep=None, arrays=True) -> convergence.ConvergenceReport:
        """convergence.ConvergenceReport of the S scenarios of the last run(history="device").

        groups    None, or one integer per scenario: the pool it belongs to (convergence_report_device's).
        keep      None, or (S, n) booleans in the caller's residence order: the residences of scenario s the records
                  cover.
        arrays    False: no per-residence records.
        `residences`, `keep` and worst_index are in the caller's residence order.  Only records are read back."""
        hist = getattr(self, "diff_history", None)
        if hist is None:
            raise ValueError('convergence report: no history on the device -- run(history="device") first')
        S, n = self.S_count, self.n_res
        if keep is not None:
            keep = np.asarray(keep)
            if keep.shape != (S, n):
                raise ValueError(f"convergence report: keep must be (scenarios, residences) = {(S, n)} in the caller's "
                                 f"residence order, got {keep.shape}")
            keep = keep[:, self.perm]
        rep = convergence.convergence_report_device(hist, eps, S, keep, np.asarray(self.perm), groups, patience, arrays)
        return convergence.report_in_caller_order(rep, self.inv_perm)
