"""The steady state of lpsolver.solve_ADMM's loop (reference lpsolver.py:254-287) while the
operator's multipliers are expected to stand: the speculative iteration (the sweep enqueued behind
the operator's first evaluation, kept if that evaluation finds every row within tolerance) and the
bursts of the native loops -- revs_plan_stream_run_blocks (the default: verdicts by blocks, up to 32
iterations per launch, four rotating sets of state buffers),
revs_plan_stream_run (every launch judges itself) and, without the feeder's tree,
revs_plan_spec_run -- and what follows a failed verdict.  Methods of AdmmEngine (mixed in by
engine.py)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr


def _dp(t) -> int:
    """data_ptr() of a long-lived buffer, remembered on the tensor object itself (the bursts of
    the streaming loop are short: a dozen data_ptr() calls are microseconds of an idle GPU)."""
    d = getattr(t, "_revs_dp", None)
    if d is None:
        d = t.data_ptr()
        try:
            t._revs_dp = d
        except AttributeError:
            pass
    return d


class SteadyStateMixin:
    def _spec_book(self, n):
        """n speculative or streamed sweeps kept: each iteration's operator solve was its one evaluation."""
        self.op_iters_hist.extend([1] * n)
        self.op_path_hist.extend(["dual"] * n)
        self.newton_hist.extend([(0, 1, 0)] * n)
        self.op_converged = True
        self.spec_hist[0] += n
        self._spec_back = 1

    def _spec_finish(self, n, count, stt=None, hist=None):
        """After a native loop that enqueued `count` steady-state iterations and kept the first n: book them.  With
        n < count the verdict of iteration n failed (its sweep wrote to the spares only; every launch behind it was a
        no-op): finish it as step() finishes a discarded speculative sweep, from the evaluation's stats `stt` when
        they carry a dual value.  `hist`: row i receives the residences' diff of the i-th iteration.  Returns the
        number of iterations done."""
        if n:
            self._spec_book(n)
            self.iteration += n
        if n == count:
            if hist is not None:
                self.diff.copy_(hist[n - 1])         # (self.diff: always the last iteration's)
            return n
        self._fused_ready = False
        self._spec_discard(stt, False)
        self.P_est, self.P_est_new = self.P_est_new, self.P_est
        self.iteration += 1
        if hist is not None:
            hist[n].copy_(self.diff)
        return n + 1

    def _spec_discard(self, stt, write_sc):
        """A speculative sweep whose evaluation found rows beyond tolerance: finish the Newton
        solve (from the evaluation's stats `stt` when they carry a dual value), run the sweep
        on its answer; speculation backs off."""
        self.spec_hist[1] += 1
        self._spec_back = min(2 * self._spec_back, 64)
        self._spec_wait = self._spec_back
        if stt is not None:
            stt = self._dual_complete(self.yd[0], self._y_support, 0)
        if not self._operator_solve_newton(first=stt):
            self._admm_take_over()
        self.agent_step(write_sc)

    def _spec_step(self, write_sc):
        """step() while the multipliers of the last iteration are expected to stand: the operator's first evaluation
        and the sweep on its answer (into the spare buffers) enqueued together, the sweep kept if the evaluation finds
        every row within tolerance.  On a plan one native call, revs_plan_spec_step (sharded: in phases around the
        exchanges of the node sums); else issued from here."""
        o = self.op
        self._fold_resume = False
        if self._plan is not None:               # one native call: enqueue, wait, judge
            rm = C.c_double()
            fused_in = self._fused_ready
            p0 = self.pnq[0]
            p_in = self._fused_p if fused_in else p0
            p_out = None
            if o.fuse_home_pass and not self._y_support:
                p_out = self.p_alt if p_in.data_ptr() == p0.data_ptr() else p0
            self._fused_ready = False

            def call(phase):
                check(self.lib.revs_plan_spec_step(
                    self._plan, phase, ptr(self.yd[0]), int(self._y_support), ptr(self.P_est),
                    ptr(self.P_est_new), ptr(self.P_sch), ptr(self.G), ptr(self.P_sch_alt),
                    ptr(self.G_alt), ptr(self.S) if write_sc else None,
                    ptr(self.Csoc) if write_sc else None, int(fused_in), ptr(p_in), ptr(p_out),
                    ptr(self.P_est_alt), C.byref(rm), None, None, self.stream), "revs_plan_spec_step")
            ar_ahead = prod_ahead = False
            skip_product = fused_in and self._ar_ahead and self._prod_ahead
            if self.group is None:
                call(3)
            else:                                # home pass, exchange of p, the rest
                if not fused_in:
                    call(1)
                if not (fused_in and self._ar_ahead):
                    self._allreduce(p_in)        # the only exchange of the iteration
                self._ar_ahead = self._prod_ahead = False
                if p_out is None:
                    call(2 | (4 if skip_product else 0))
                else:
                    # enqueue product and sweep, then -- before waiting for the verdict --
                    # the exchange of the node sums this sweep leaves for the NEXT
                    # evaluation: it is stream-ordered behind the sweep, and its host-side
                    # cost overlaps the sweep instead of standing between two iterations
                    # (a discarded sweep makes it a wasted, harmless exchange; every rank
                    # takes the same decisions, so the collectives stay in step)
                    call(2 | 16 | (4 if skip_product else 0))
                    self._allreduce(p_out)
                    ar_ahead = True
                    if fused_in:
                        # ... and the next product behind it (not after an evaluation whose
                        # stats a discard would continue from: its node sums must survive)
                        check(self.lib.revs_plan_spec_step(
                            self._plan, 64, ptr(self.yd[0]), 0, None, None, None, None, None, None,
                            None, None, 0, ptr(p_out), ptr(p_in), None, None, None, None,
                            self.stream), "revs_plan_spec_step")
                        prod_ahead = True
                    call(32)
            kept = rm.value / self._scale <= o.eps
            # after a fused home pass the stats carry no dual value: a discarded sweep is
            # followed by a fresh evaluation instead of a continuation from these stats
            stt = None if (kept or fused_in) else self.stats_host[0].numpy().copy()
            if kept and p_out is not None:
                self._fused_ready, self._fused_p = True, p_out
                self._ar_ahead, self._prod_ahead = ar_ahead, prod_ahead
        else:
            self._dual_launch(self.yd[0], self._y_support, 0, full=False)
            self.agent_step(write_sc, to_alt=True)
            stt = self._dual_wait(0)
            kept = stt[:, 0].max() / self._scale <= o.eps
        if kept:
            self.P_sch, self.P_sch_alt = self.P_sch_alt, self.P_sch
            self.G, self.G_alt = self.G_alt, self.G
            self._spec_book(1)
        else:                          # rows need work: finish the solve, redo the sweep
            self._spec_discard(stt, write_sc)

    def _spec_run(self, count):
        """Up to `count` speculative iterations inside ONE native call, revs_plan_spec_run (one GPU, no multipliers,
        the fused home pass; the buffer rotation included, no Python between the launches), which returns at the
        first sweep that has to be discarded.  Returns the number of iterations done."""
        p0 = self.pnq[0]
        self._p_clear = None
        if self._fused_ready and self._fused_p is self.p_alt2:     # (revs_plan_spec_run knows two arrays)
            p0.copy_(self.p_alt2)
            self._fused_p = p0
        bufs = (self.P_est, self.P_est_new, self.P_est_alt, self.P_sch, self.P_sch_alt, self.G,
                self.G_alt)
        st = _lib.SpecState(*[ptr(t) for t in bufs], ptr(p0), ptr(self.p_alt),
                            ptr(self._fused_p) if self._fused_ready else None,
                            int(self._fused_ready))
        kept, fin, rm = C.c_int32(), C.c_int32(), C.c_double()
        check(self.lib.revs_plan_spec_run(self._plan, count, ptr(self.yd[0]), C.byref(st),
                                          self._scale, self.op.eps, C.addressof(kept), C.addressof(fin),
                                          C.addressof(rm), self.stream), "revs_plan_spec_run")
        n = kept.value
        by = self._rebind(st, bufs)
        self.P_est_alt = by[st.p_est_alt]
        self._fused_ready = bool(st.fused_ready)
        if self._fused_ready:
            self._fused_p = p0 if st.fused_p == p0.data_ptr() else self.p_alt
        # (the stats of a discarded sweep's evaluation carry a dual value unless it followed a fused home pass)
        stt = None if (n == count or fin.value) else self.stats_host[0].numpy().copy()
        return self._spec_finish(n, count, stt)

    def _stream_ok(self):
        """The steady state as one launch per iteration (revs_plan_stream_run) applies: a plan
        with the feeder's tree, no multipliers, speculation allowed, and -- sharded -- the
        library's own communicator."""
        o = self.op
        return (self._plan is not None and self._tree is not None and o.solver == "newton"
                and (self._block or self._tree.n <= _lib.TREE_SWEEP_MAX)     # (big trees: judged by blocks only)
                and o.speculate and self._spec_ok and o.fuse_home_pass and not self._y_support
                and (self.group is None or self._comm is not None))

    def _stream_run(self, count, hist=None):
        """Up to `count` steady-state iterations (at most the current burst), one launch each,
        enqueued in one go by the native loop; the first iteration whose rows are not within
        tolerance silences the launches behind it and is finished here as step() finishes a
        discarded speculative sweep.  Returns the number of iterations done (at least one).
        `hist`: float[>= count][n] on the device -- row i receives the residences' diff of the
        i-th iteration done here (run(): solve_ADMM's per-iteration diff without a host round
        trip per iteration)."""
        o = self.op
        self._fold_resume = False
        if self._block:
            return self._stream_run_blocks(count, hist)
        p0 = self._fused_p
        d0 = _dp(p0)
        if self._pn0 is None:
            self._pn0 = self.pnq[0]
        rest = [b for b in (self._pn0, self.p_alt, self.p_alt2) if _dp(b) != d0]
        # p[1] must be zero on entry.  The last launch of a fully kept call has just cleared the
        # array that is p[1] now (roles rotate): no fill launch then
        if self._p_clear is not None and _dp(self._p_clear) != d0:
            dc = _dp(self._p_clear)
            rest = [self._p_clear] + [b for b in rest if _dp(b) != dc]
        else:
            rest[0].zero_()
        self._p_clear = None
        if self.group is not None and not self._ar_ahead:
            self._allreduce(p0)
        pes = (self.P_est, self.P_est_new, self.P_est_alt)
        pss, gs, ps = (self.P_sch, self.P_sch_alt), (self.G, self.G_alt), (p0, rest[0], rest[1])
        st = self._stream_st
        by = {}
        for i in range(3):
            a, b = _dp(pes[i]), _dp(ps[i])
            st.p_est[i], st.p[i] = a, b
            by[a], by[b] = pes[i], ps[i]
        for i in range(2):
            a, b = _dp(pss[i]), _dp(gs[i])
            st.p_sch[i], st.gamma[i] = a, b
            by[a], by[b] = pss[i], gs[i]
        kept, rm = self._stream_out
        count = min(count, self._burst)
        st.diff_hist = None if hist is None else hist.data_ptr()
        check(self.lib.revs_plan_stream_run(self._plan, count, self._stream_st_ref, self._scale, o.eps,
                                            self._stream_out_ref[0], self._stream_out_ref[1], self.stream),
              "revs_plan_stream_run")
        n = kept.value
        self.P_est, self.P_est_new, self.P_est_alt = (by[st.p_est[i]] for i in range(3))
        self.P_sch, self.P_sch_alt = by[st.p_sch[0]], by[st.p_sch[1]]
        self.G, self.G_alt = by[st.gamma[0]], by[st.gamma[1]]
        self._fused_p = by[st.p[0]]
        self._p_clear = by[st.p[1]] if n == count else None
        return self._stream_finish(count, n, hist)

    def _stream_finish(self, count, n, hist):
        """The rest of a streaming burst of `count` launches of which n were kept: its record, the next burst's
        length (x4 after a fully kept one, back to stream_burst after a failed verdict), the node sums the loop
        left exchanged (sharded) but not multiplied, and the booking."""
        o = self.op
        self.stream_calls.append((count, n))
        self._burst = min(4 * self._burst, o.stream_burst_max) if n == count else o.stream_burst
        self._prod_ahead = False
        self._ar_ahead = self.group is not None
        return self._spec_finish(n, count, None, hist)

    def _state_pools(self):
        """The pools the residences' state buffers rotate through (allocated on first use): four sets for the
        block form's roll-back without copies, of which the folded chain borrows a third set for the sweep it
        enqueues unjudged.  self.P_est / P_est_new / P_est_alt / P_sch / P_sch_alt / G / G_alt are always members."""
        if self._sets is None:
            z = lambda t: torch.zeros_like(t)
            self._sets = dict(pe=[self.P_est, self.P_est_new, self.P_est_alt, z(self.P_est), z(self.P_est)],
                              ps=[self.P_sch, self.P_sch_alt, z(self.P_sch), z(self.P_sch)],
                              g=[self.G, self.G_alt, z(self.G), z(self.G)],
                              y=([self.pdhg_dual] + [z(self.pdhg_dual) for _ in range(3)]
                                 if self.pdhg_dual is not None else None))
        return self._sets

    def _stream_run_blocks(self, count, hist=None):
        """_stream_run with the verdicts taken by blocks and `stream_inner` iterations per launch
        (revs_plan_stream_run_blocks): the state rotates through four sets of buffers, so that a
        failed verdict deep inside a burst is undone without copies."""
        o = self.op
        self._state_pools()
        p0 = self._fused_p
        if self.group is not None and not self._ar_ahead:
            self._allreduce(p0)
        pool = self._sets
        st, by = self._sets_st, self._sets_by
        # The native call leaves the sets in the order the next call wants them (slot 0 = the state).  As long
        # as nothing else has touched the engine's tensors since, the struct is handed back as it is.
        sig = (id(self.P_est), id(self.P_est_new), id(self.P_sch), id(self.G), id(self.pdhg_dual))
        if sig != self._sets_sig:
            def roles(first, tensors, skip=()):
                rest = [t for t in tensors if t is not first and all(t is not x for x in skip)]
                return [first] + rest

            pes = roles(self.P_est, pool["pe"], skip=(self.P_est_new,))
            pss, gs = roles(self.P_sch, pool["ps"]), roles(self.G, pool["g"])
            ys = roles(self.pdhg_dual, pool["y"]) if pool["y"] is not None else [None] * 4
            assert len(pes) == len(pss) == len(gs) == len(ys) == 4
            for i in range(4):
                for arr, t in ((st.p_est, pes[i]), (st.p_sch, pss[i]), (st.gamma, gs[i]), (st.pdhg_dual, ys[i])):
                    arr[i] = None if t is None else _dp(t)
                    if t is not None:
                        by[_dp(t)] = t
            st.p_est_next = _dp(self.P_est_new)
        if self._pn0 is None:
            self._pn0 = self.pnq[0]
            self._pn_ptr = {id(self._pn0): _dp(self._pn0), id(self.p_alt): _dp(self.p_alt)}
        # (the sums handed over for the next call; by address: self.pnq[0] is a fresh view object wherever it is taken)
        p0_out = self.p_alt if _dp(p0) == _dp(self._pn0) else self._pn0
        pp = self._pn_ptr
        st.p0 = pp[id(p0)] if id(p0) in pp else _dp(p0)
        st.p0_out = pp[id(p0_out)]
        st.diff_hist = None if hist is None else hist.data_ptr()
        count = min(count, self._burst, 1000)
        kept, rm = self._stream_out
        check(self.lib.revs_plan_stream_run_blocks(self._plan, count, self._sets_ref, self._scale, o.eps,
                                                   self._stream_out_ref[0], self._stream_out_ref[1],
                                                   self._dmax_addr, self.stream),
              "revs_plan_stream_run_blocks")
        n = kept.value
        self.P_est, self.P_est_alt = by[st.p_est[0]], by[st.p_est[1]]
        self.P_sch, self.P_sch_alt = by[st.p_sch[0]], by[st.p_sch[1]]
        self.G, self.G_alt = by[st.gamma[0]], by[st.gamma[1]]
        if pool["y"] is not None:
            self.pdhg_dual = by[st.pdhg_dual[0]]       # (the plan already points at it)
        self._sets_sig = ((id(self.P_est), id(self.P_est_new), id(self.P_sch), id(self.G), id(self.pdhg_dual))
                          if n == count else None)
        self._p_clear = None
        if n == count:
            self._fused_p = p0_out
        if n:
            self._max_diff_bursts.append((self.iteration, self._dmax_buf[:n]))   # (folded into max_diff when next read)
        return self._stream_finish(count, n, hist)
