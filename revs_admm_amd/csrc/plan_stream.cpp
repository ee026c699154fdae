// The streaming steady state: one launch per ADMM iteration, verdicts per launch or by blocks (see revs_admm.h).
#include "plan.h"

// two HIP events around the bursts since revs_plan_stream_timing, on the bursts' own stream
static void timing_begin(revs_plan_t *plan, hipStream_t s) {
    if (plan->timing == 1 && hipEventRecord(plan->tev[0], s) == hipSuccess) { plan->timing = 2; plan->timed_launches = 0; }
}
static void timing_end(revs_plan_t *plan, hipStream_t s) {
    if (plan->timing == 2) (void)hipEventRecord(plan->tev[1], s);
}

// Wait for the record of launch `seq`; 0 = kept, 1 = its verdict failed, < 0 = error.
static int stream_wait(revs_plan_t *plan, unsigned int seq, hipStream_t s, double *rmax) {
    const volatile double *r = plan->rec_host + 4 * (seq % revs::kRecRing);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    static const bool trace = getenv("REVS_PLAN_TRACE") != nullptr;
    auto prev = t0;
    while (r[2] != (double)seq) {
        if (trace) {        // the longest the host itself was away from this loop
            const auto now = std::chrono::steady_clock::now();
            plan->t_wait = std::max(plan->t_wait, std::chrono::duration<double, std::micro>(now - prev).count());
            prev = now;
        }
        // (no HIP call in this loop: a hipStreamQuery here was measured to stop the host for
        // milliseconds now and then -- the runtime retires its finished commands inside it --
        // while the queue behind the awaited launch ran dry)
        if ((++spins & 0xFFFFF) == 0) {
            const auto waited = std::chrono::steady_clock::now() - t0;
            if (waited > std::chrono::seconds(2) && hipStreamQuery(s) == hipSuccess && r[2] != (double)seq) {
                revs::set_error("revs_plan_stream_run: stream idle but record %u missing", seq);
                return REVS_ELAUNCH;
            }
            if (waited > std::chrono::seconds(120)) {
                (void)hipStreamSynchronize(s);
                revs::set_error("revs_plan_stream_run: timed out waiting for record %u", seq);
                return REVS_ELAUNCH;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *rmax = r[0];
    return r[1] != 0.0 ? 1 : 0;
}

// The sequence numbers of the streaming launches wrap once in 4e9 launches: the control block starts over.
static int stream_wrap(revs_plan_t *plan, hipStream_t s, const char *who) {
    if (plan->stream_seq <= 0xFFFF0000u) return REVS_OK;
    const revs::StreamCtl ctl0{0u, 0u, 0ull};
    if (hipStreamSynchronize(s) != hipSuccess ||
        hipMemcpy(plan->ctl, &ctl0, sizeof(ctl0), hipMemcpyHostToDevice) != hipSuccess) {
        revs::set_error("%s: resetting the control block failed", who);
        return REVS_ELAUNCH;
    }
    plan->stream_seq = 0;
    return REVS_OK;
}

static void stream_rotate(revs_stream_state_t *st, int kept, int64_t n_homes) {
    if (kept <= 0) return;
    revs_stream_state_t r = *st;
    for (int i = 0; i < 3; ++i) { r.p_est[i] = st->p_est[(kept + i) % 3]; r.p[i] = st->p[(kept + i) % 3]; }
    for (int i = 0; i < 2; ++i) { r.p_sch[i] = st->p_sch[(kept + i) % 2]; r.gamma[i] = st->gamma[(kept + i) % 2]; }
    if (st->diff_hist) r.diff_hist = st->diff_hist + (int64_t)kept * n_homes;
    *st = r;
}

// The streaming loop with the verdicts taken by blocks (see include/revs_admm.h).  Iteration k of
// the call has number seq0 + k and consumes the node sums "of iteration k".  Enqueued in one burst:
//   verdict of iteration 0 (the caller's st->p0);
//   per block [k0, k0 + nb):  sweep launches of up to `inner` iterations each, iteration k
//       accumulating the sums of iteration k + 1 (and the partial maxima of its own diff) into
//       ring slice k - k0 | ONE all-reduce of the nb slices (sharded) | verdicts of iterations
//       k0+1 .. k0+nb (the last block: .. max_steps - 1, its last slice is the next call's st->p0;
//       its diff tail is folded into the extra record seq0 + max_steps) | the slices cleared;
// every launch is a no-op once an iteration at or before its own has failed.  With plan->overlap
// the all-reduce and the verdicts of block b go to the plan's second stream while the caller's
// stream runs block b + 1 (two ring halves; block b + 2 waits for block b's verdicts).  The
// blocks are B long, the last B iterations of a call split 3 : 1 so that the all-reduce nobody
// can hide -- the last one -- is a short one.  Then the records are read in order.
// Roll-back without copies: the residences' state lives in FOUR sets of buffers.  A block reads
// its entry set E_b and its launches alternate between the two sets that are neither E_b nor
// E_{b-1}, so the state a block started from survives until the block AFTER it has been enqueued
// -- and that one cannot start before this block's verdicts are in.  A failed iteration j means
// that sweeps behind j ran on an estimate that was not the operator's answer: the sweeps from the
// entry of the block that judged j up to j - 1 (all judged good) are run again from E_b, then sweep
// j itself (outputs to a spare set, carried multipliers in place): bit for bit the memory that the
// loop judging every launch leaves behind a failed verdict.
extern "C" int revs_plan_stream_run_blocks(revs_plan_t *plan, int32_t max_steps, revs_stream_sets_t *st,
                                           double scale, double eps, int32_t *kept_steps, double *rmax_last,
                                           double *dmax_out, void *stream) {
    REVS_REQUIRE(plan && st && kept_steps && rmax_last && max_steps >= 0 && max_steps < revs::kRecRing - 1 &&
                 scale > 0.0 && eps > 0.0, "revs_plan_stream_run_blocks: bad argument (at most %d steps per call)",
                 revs::kRecRing - 2);
    const revs_plan_desc_t &d = plan->d;
    REVS_REQUIRE(plan->tree.n > 0 && d.node_of && plan->block > 1 && d.recompute_pe_new,
                 "revs_plan_stream_run_blocks: needs a tree, node_of, recompute_pe_new and revs_plan_set_stream_block");
    const bool warm = d.mode == REVS_MODE_RELAXED_PDHG && d.pdhg_dual != nullptr;
    for (int i = 0; i < 4; ++i) {
        REVS_REQUIRE(st->p_est[i] && st->p_sch[i] && st->gamma[i] && (!warm || st->pdhg_dual[i]),
                     "revs_plan_stream_run_blocks: null buffer in set %d", i);
        for (int j = 0; j < i; ++j)
            REVS_REQUIRE(st->p_est[i] != st->p_est[j] && st->p_sch[i] != st->p_sch[j] && st->gamma[i] != st->gamma[j] &&
                         (!warm || st->pdhg_dual[i] != st->pdhg_dual[j]),
                         "revs_plan_stream_run_blocks: the four sets must be distinct buffers");
        REVS_REQUIRE(st->p_est_next != st->p_est[i], "revs_plan_stream_run_blocks: p_est_next must not be in a set");
    }
    REVS_REQUIRE(st->p0 && st->p0_out && st->p0 != st->p0_out && st->p_est_next,
                 "revs_plan_stream_run_blocks: p0 / p0_out / p_est_next missing (or p0 == p0_out)");
    REVS_REQUIRE(!warm || st->pdhg_dual[0] == d.pdhg_dual,
                 "revs_plan_stream_run_blocks: set 0 does not hold the plan's carried multipliers (%p, the plan's: %p)",
                 (void *)st->pdhg_dual[0], (void *)d.pdhg_dual);
    hipStream_t s = (hipStream_t)stream;
    *kept_steps = 0;
    *rmax_last = 0.0;
    if (max_steps == 0) return REVS_OK;
    if (stream_wrap(plan, s, "revs_plan_stream_run_blocks") != REVS_OK) return REVS_ELAUNCH;
    const unsigned int seq0 = plan->stream_seq + 1;
    const int64_t mt = (int64_t)d.m * d.T, nt = d.n_homes * (int64_t)d.T;
    (void)nt;
    const int B = plan->block, K = std::min(plan->inner, revs_agent_max_inner(d.T, d.pdhg.lanes));
    const int nranks = plan->comm ? plan->comm->nranks : 1, rank = plan->comm ? plan->comm->rank : 0;
    const int ntail = REVS_DMAX_SLOTS * nranks;
    const int64_t stride = mt + ntail;                   // doubles per ring slice: node sums, then every rank's partial maxima
    // (the second stream costs a burst ~0.15 ms of host time in event and cross-stream calls: a
    // burst of one block has nothing to hide behind and stays on the caller's stream)
    const bool ov = plan->overlap != 0 && max_steps > B;
    const double vtol = eps * scale;
    auto hip_ok = [&](hipError_t e, const char *what) -> int {
        if (e == hipSuccess) return REVS_OK;
        revs::set_error("revs_plan_stream_run_blocks: %s: %s", what, hipGetErrorString(e));
        return REVS_ELAUNCH;
    };
    {   // the ring: two halves of B slices (one half without the second stream)
        const size_t need = (size_t)2 * B * stride;
        if (plan->ring_cap < need) {
            if (plan->ring) { (void)hipStreamSynchronize(s); (void)hipFree(plan->ring); }
            plan->ring = nullptr;
            plan->ring_cap = 0;
            if (hip_ok(hipMalloc((void **)&plan->ring, sizeof(double) * need), "hipMalloc(ring)") != REVS_OK)
                return REVS_ELAUNCH;
            plan->ring_cap = need;
            plan->ring_dirty = true;
        }
    }
    // block starts: k0[b], b = 0 .. nblocks (k0[nblocks] = max_steps)
    std::vector<int> k0s;
    for (int k = 0; k < max_steps;) {
        k0s.push_back(k);
        const int rem = max_steps - k;
        k += rem > B ? B : (ov && rem >= 8 ? rem - (rem + 3) / 4 : rem);
    }
    const int nblocks = (int)k0s.size();
    k0s.push_back(max_steps);
    auto block_of = [&](int j) {       // the block whose verdicts cover iteration j >= 1: k0 < j <= k0 + nb
        int b = 0;
        while (k0s[b + 1] < j) ++b;
        return b;
    };
    auto ring_of = [&](int b) { return plan->ring + (ov ? (int64_t)(b & 1) * B * stride : 0); };
    // One launch: iterations k .. k + kin - 1 from set `in` to set `out`; their node sums and diff
    // tails to slices (k - k0) .. of `ring` (replay: one scratch region, no tails).
    const int32_t *const wg_order = plan_wg_order(plan);
    revs::SweepCall call = plan_sweep_call(d, stream);       // (what no launch of this run changes)
    auto sweep = [&](int k, int kin, int in, int out, double *slice0, bool replay, float *pe_next,
                     bool y_in_place) -> int {
        revs::StreamExtra sx{};
        sx.ctl = plan->ctl;
        sx.seq = seq0 + (unsigned int)k + 1u;            // (the kernel skips when bad < seq: at or before k)
        sx.base_seq = replay ? sx.seq : seq0;            // (a replayed sweep is never skipped)
        sx.verdict = false;
        sx.flags = plan->flags_dev;
        sx.kin = kin;
        sx.pe_out = st->p_est[out];
        sx.y_out = warm ? (y_in_place ? st->pdhg_dual[in] : st->pdhg_dual[out]) : nullptr;
        sx.slice_stride = stride;
        sx.diff_stride = st->diff_hist ? d.n_homes : 0;
        sx.dmax_out = replay ? nullptr : slice0 + mt + (int64_t)rank * REVS_DMAX_SLOTS;
        sx.wg_order = wg_order;
        call.p_est_old = st->p_est[in];
        call.p_sch = st->p_sch[in]; call.gamma = st->gamma[in];
        call.p_sch_out = st->p_sch[out]; call.gamma_out = st->gamma[out];
        call.diff = st->diff_hist ? st->diff_hist + (int64_t)k * d.n_homes : d.diff;
        call.pdhg_dual = warm ? st->pdhg_dual[in] : nullptr;
        call.p_next = slice0; call.pe2_out = pe_next;
        return revs::agent_step_stream(call, sx);
    };
    // events of the overlapped form: [2 b] = block b's sweeps are done, [2 b + 1] = its verdicts are
    // in, [2 nblocks] = the side stream has finished this call
    if (ov)
        while ((int)plan->events.size() < 2 * nblocks + 1) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                revs::set_error("revs_plan_stream_run_blocks: hipEventCreate failed");
                return REVS_ELAUNCH;
            }
            plan->events.push_back(e);
        }
    int rc = REVS_OK, launched = 0, checked = 0, failed_at = -1;
    double rm = 0.0;
    static const bool trace = getenv("REVS_PLAN_TRACE") != nullptr;
    const auto tr0 = std::chrono::steady_clock::now();
    timing_begin(plan, s);
    // The slices a call accumulates into are zero: every verdict launch clears what it has judged.
    // Only a fresh ring, or one a failed call left behind (silenced launches judge nothing), is cleared here.
    if (plan->ring_dirty) {
        rc = hip_ok(hipMemsetAsync(plan->ring, 0, sizeof(double) * plan->ring_cap, s), "hipMemsetAsync(ring)");
        plan->ring_dirty = false;
    }
    hipStream_t q = ov ? plan->side : s;                 // where the collective and the verdicts go
    std::vector<int> entry(nblocks + 1, 0);              // the set a block starts from
    int cur = 0, prev = 1;                               // prev: the entry of the block before (kept intact as well)
    for (int b = 0; b < nblocks && rc == REVS_OK; ++b) {
        const int k0 = k0s[b], nb = k0s[b + 1] - k0;
        double *ring = ring_of(b);
        entry[b] = cur;
        int wk[2], nw = 0;
        for (int i = 0; i < 4; ++i) if (i != cur && i != prev) wk[nw++] = i;
        // (overlapped: this block reuses the ring half of block b - 2, whose verdicts must be in
        // and the half cleared -- they also decide whether this block is a no-op -- and rewrites
        // the set block b - 2 started from)
        if (ov && b >= 2) rc = hip_ok(hipStreamWaitEvent(s, plan->events[2 * (b - 2) + 1], 0), "hipStreamWaitEvent");
        int in = cur, w = 0;
        const bool time_block = plan->timing != 0 && plan->comm && plan->cev[0] && b == 0;      // (a call's first block)
        if (time_block && rc == REVS_OK) rc = hip_ok(hipEventRecord(plan->cev[2], s), "hipEventRecord");
        for (int k = k0; k < k0 + nb && rc == REVS_OK;) {
            const int kin = std::min(K, k0 + nb - k);
            const bool last = (k + kin == max_steps);    // the call's last launch also prepares P_est[k+n+1]
            rc = sweep(k, kin, in, wk[w], ring + (int64_t)(k - k0) * stride, false, last ? st->p_est_next : nullptr, false);
            ++plan->timed_launches;
            in = wk[w];
            w ^= 1;
            k += kin;
            launched += kin;
        }
        if (time_block && rc == REVS_OK) rc = hip_ok(hipEventRecord(plan->cev[3], s), "hipEventRecord");
        prev = cur;
        cur = in;
        // The call's last block has nothing to run beside: without a collective its verdicts go behind its
        // sweeps on the caller's stream -- no hop between streams in front of the launch the host waits for
        // (a burst of one block never leaves the stream) -- once the block before has been judged (the
        // verdict launches share their arrival counter).
        const bool lastb = b + 1 == nblocks;
        const bool on_main = ov && lastb && !plan->comm;
        hipStream_t vq = on_main ? s : q;
        if (on_main) {
            if (b >= 1 && rc == REVS_OK)
                rc = hip_ok(hipStreamWaitEvent(s, plan->events[2 * (b - 1) + 1], 0), "hipStreamWaitEvent");
        } else {
            if (ov && rc == REVS_OK) rc = hip_ok(hipEventRecord(plan->events[2 * b], s), "hipEventRecord");
            if (ov && rc == REVS_OK) rc = hip_ok(hipStreamWaitEvent(q, plan->events[2 * b], 0), "hipStreamWaitEvent");
        }
        if (rc == REVS_OK && plan->comm) {
            if (time_block) rc = hip_ok(hipEventRecord(plan->cev[0], q), "hipEventRecord");
            if (rc == REVS_OK) rc = revs_comm_allreduce_f64(plan->comm, ring, (int64_t)nb * stride, 0, q);
            if (time_block && rc == REVS_OK) {
                rc = hip_ok(hipEventRecord(plan->cev[1], q), "hipEventRecord");
                plan->cev_valid = rc == REVS_OK;
                plan->cev_nb = nb;
            }
        }
        // block 0's launch also judges the call's first iteration (the caller's st->p0: its sweep ran
        // unjudged, like every other sweep of the block); the last block's also hands the call's last
        // slice over to the caller (st->p0_out) and folds its tail into the extra record
        const int judged = (lastb ? nb - 1 : nb) + (b == 0 ? 1 : 0);
        if (rc == REVS_OK)
            rc = revs::stream_block_verdict(plan->ctl, seq0, seq0 + (unsigned int)k0,
                                            seq0 + (unsigned int)k0 + (b == 0 ? 0u : 1u), judged, d.T, plan->tree,
                                            b == 0 ? st->p0 : nullptr, ring, stride, (int32_t)mt, ntail,
                                            lastb ? st->p0_out : nullptr, d.vlo, d.vhi, vtol,
                                            plan->grp_bits, plan->grp_dmax, plan->rec_dev, vq);
        if (ov && rc == REVS_OK) rc = hip_ok(hipEventRecord(plan->events[2 * b + 1], vq), "hipEventRecord");
    }
    entry[nblocks] = cur;
    if (ov) {        // the caller's stream is done when the side stream is (also after an error above)
        int r2 = hip_ok(hipEventRecord(plan->events[2 * nblocks], q), "hipEventRecord");
        if (r2 == REVS_OK) r2 = hip_ok(hipStreamWaitEvent(s, plan->events[2 * nblocks], 0), "hipStreamWaitEvent");
        if (rc == REVS_OK) rc = r2;
    }
    timing_end(plan, s);
    const auto tr1 = std::chrono::steady_clock::now();
    // records 0 .. launched - 1 are the iterations' verdicts; record `launched` carries the last
    // iteration's max diff only
    for (; rc == REVS_OK && checked <= launched && failed_at < 0; ++checked) {
        double r = 0.0;
        const int v = stream_wait(plan, seq0 + (unsigned int)checked, s, &r);
        if (v < 0) rc = v;
        else if (v == 1) failed_at = checked;
        if (checked < launched) rm = r;
        if (v >= 0 && dmax_out && checked >= 1)
            dmax_out[checked - 1] = plan->rec_host[4 * ((seq0 + (unsigned int)checked) % revs::kRecRing) + 3];
    }
    if (trace) {
        fprintf(stderr, "[revs_plan_stream_run_blocks] %d blocks of at most %d, %d iterations per launch%s: %d iterations "
                "enqueued in %.1f us, records read %.1f us later (host away from the wait loop for at most %.1f us), "
                "failed at %d\n", nblocks, B, K, ov ? ", overlapped" : "", launched,
                std::chrono::duration<double, std::micro>(tr1 - tr0).count(),
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr1).count(),
                plan->t_wait, failed_at);
        plan->t_wait = 0.0;
    }
    plan->stream_seq = seq0 + (unsigned int)std::max(launched, 1);
    *rmax_last = rm;
    if (failed_at >= 0 || rc != REVS_OK) {
        if (ov) (void)hipStreamSynchronize(plan->side);
        (void)hipStreamSynchronize(s);
        plan->ring_dirty = true;
        // The sticky status word has collected bits from sweeps that are now undone (they ran on an
        // estimate that was not the operator's answer): "a PDHG residence stopped at its cap" is a
        // statement about such a sweep's problem, not about the trajectory -- dropped here and set
        // again by the replay below for the sweeps that stand.  ("No solution" does not depend on
        // the estimate: kept.)
        if (plan->flags_host) *(volatile unsigned int *)plan->flags_host &= ~2u;
    }
    int kept = rc != REVS_OK ? 0 : (failed_at >= 0 ? failed_at : launched);
    int fin = cur;                                       // the set that holds the state at return
    if (rc == REVS_OK && failed_at >= 0) {
        // Block bf judged it.  If it is the first iteration of block bf + 1, that block's entry set IS
        // the state wanted (a block never writes the set it started from).  Otherwise go back to bf's
        // own entry and run the good sweeps k0 .. failed_at - 1 again, alternating between two sets
        // that are not the entry.
        const int bf = failed_at > 0 ? block_of(failed_at) : -1;
        int k = failed_at, in = entry[0];
        if (bf >= 0) {
            if (failed_at == k0s[bf + 1]) in = entry[bf + 1];
            else { k = k0s[bf]; in = entry[bf]; }
        }
        int wk[2], nw = 0;
        for (int i = 0; i < 4 && nw < 2; ++i) if (i != in) wk[nw++] = i;
        int w = 0;
        while (k < failed_at && rc == REVS_OK) {
            const int kin = std::min(K, failed_at - k);
            rc = sweep(k, kin, in, wk[w], plan->ring, true, nullptr, false);
            in = wk[w];
            w ^= 1;
            k += kin;
        }
        // ... and the failed iteration's own sweep, as the loop that judges every launch runs it:
        // outputs to a spare set, the carried multipliers updated in place
        int spare = 0;
        while (spare == in) ++spare;
        if (rc == REVS_OK) rc = sweep(failed_at, 1, in, spare, plan->ring, true, st->p_est_next, true);
        fin = in;
        if (rc != REVS_OK || hipStreamSynchronize(s) != hipSuccess) {
            if (rc == REVS_OK) revs::set_error("revs_plan_stream_run_blocks: replaying the block failed");
            rc = REVS_ELAUNCH;
            kept = 0;
        }
    }
    *kept_steps = kept;
    if (rc == REVS_OK && fin != 0) {                     // roles: set 0 = the state at return
        std::swap(st->p_est[0], st->p_est[fin]);
        std::swap(st->p_sch[0], st->p_sch[fin]);
        std::swap(st->gamma[0], st->gamma[fin]);
        std::swap(st->pdhg_dual[0], st->pdhg_dual[fin]);
    }
    if (rc == REVS_OK && warm) plan->d.pdhg_dual = st->pdhg_dual[0];
    if (st->diff_hist) st->diff_hist += (int64_t)kept * d.n_homes;
    return rc;
}

extern "C" int revs_plan_stream_run(revs_plan_t *plan, int32_t max_steps, revs_stream_state_t *st,
                                    double scale, double eps, int32_t *kept_steps,
                                    double *rmax_last, void *stream) {
    REVS_REQUIRE(plan && st && kept_steps && rmax_last && max_steps >= 0 && max_steps < revs::kRecRing &&
                 scale > 0.0 && eps > 0.0, "revs_plan_stream_run: bad argument (at most %d steps per call)",
                 revs::kRecRing - 1);
    const revs_plan_desc_t &d = plan->d;
    REVS_REQUIRE(plan->tree.n > 0 && plan->tree.n <= REVS_TREE_SWEEP_MAX && d.node_of,
                 "revs_plan_stream_run: the plan has no tree / node_of, or a tree of more than %d nodes (those are "
                 "judged by blocks: revs_plan_stream_run_blocks)", REVS_TREE_SWEEP_MAX);
    for (int i = 0; i < 3; ++i)
        REVS_REQUIRE(st->p_est[i] && st->p[i] && (i == 2 || (st->p_sch[i] && st->gamma[i])),
                     "revs_plan_stream_run: null buffer");
    REVS_REQUIRE(st->p[0] != st->p[1] && st->p[1] != st->p[2] && st->p[0] != st->p[2] &&
                 st->p_est[0] != st->p_est[1] && st->p_est[1] != st->p_est[2] && st->p_est[0] != st->p_est[2] &&
                 st->p_sch[0] != st->p_sch[1] && st->gamma[0] != st->gamma[1],
                 "revs_plan_stream_run: buffers must be distinct");
    hipStream_t s = (hipStream_t)stream;
    *kept_steps = 0;
    *rmax_last = 0.0;
    if (max_steps == 0) return REVS_OK;
    // (sequence numbers only grow: what an earlier call left in the control word is below this
    // call's first number and ignored by the kernels -- nothing to re-arm, no copy on the stream)
    if (stream_wrap(plan, s, "revs_plan_stream_run") != REVS_OK) return REVS_ELAUNCH;
    const unsigned int seq0 = plan->stream_seq + 1;
    const int64_t mt = (int64_t)d.m * d.T;
    REVS_REQUIRE(plan->block <= 1, "revs_plan_stream_run: verdicts by blocks go through revs_plan_stream_run_blocks");
    revs::SweepCall call = plan_sweep_call(d, stream);       // (what no launch of this run changes)
    call.pdhg_dual = d.pdhg_dual;
    auto launch = [&](int k) -> int {               // step k of this call (roles by rotation)
        revs::StreamExtra sx;
        sx.ctl = plan->ctl;
        sx.seq = seq0 + (unsigned int)k;
        sx.base_seq = seq0;
        sx.verdict = true;
        sx.tree = plan->tree;
        sx.p_in = st->p[k % 3];
        sx.p_zero = st->p[(k + 2) % 3];
        sx.vlo = d.vlo; sx.vhi = d.vhi; sx.vtol = eps * scale;
        sx.rec = plan->rec_dev + 4 * (sx.seq % revs::kRecRing);
        sx.flags = plan->flags_dev;
        sx.m = d.m;
        call.p_est_old = st->p_est[k % 3];
        call.p_est_new = d.recompute_pe_new ? nullptr : st->p_est[(k + 1) % 3];
        call.p_sch = st->p_sch[k % 2]; call.gamma = st->gamma[k % 2];
        call.p_sch_out = st->p_sch[(k + 1) % 2]; call.gamma_out = st->gamma[(k + 1) % 2];
        call.diff = st->diff_hist ? st->diff_hist + (int64_t)k * d.n_homes : d.diff;
        call.p_next = st->p[(k + 1) % 3]; call.pe2_out = st->p_est[(k + 2) % 3];
        int rc = revs::agent_step_stream(call, sx);
        if (rc != REVS_OK) return rc;
        if (plan->comm) rc = revs_comm_allreduce_f64(plan->comm, call.p_next, mt, 0, stream);
        return rc;
    };
    // All max_steps launches (and, sharded, their collectives) are enqueued in ONE burst, then
    // the records are read in order.  No decision is taken between launches -- a failed verdict
    // silences the launches behind it on the device -- so every rank of a sharded run issues the
    // same collectives whatever its timing, and the host never pauses between submissions (a
    // launch submitted after a pause was measured to start late: ~6 us always, milliseconds now
    // and then, whatever the queue holds).  The caller bounds max_steps by how many silenced
    // launches it is willing to waste behind a failure (AdmmEngine._stream_run).
    int launched = 0, checked = 0, failed_at = -1, rc = REVS_OK;
    double rm = 0.0;
    static const bool trace = getenv("REVS_PLAN_TRACE") != nullptr;
    const auto tr0 = std::chrono::steady_clock::now();
    auto tr1 = tr0;
    double slowest = 0.0;
    timing_begin(plan, s);
    for (; launched < max_steps; ++launched) {
        const auto a = trace ? std::chrono::steady_clock::now() : tr0;
        if ((rc = launch(launched)) != REVS_OK) goto out;
        ++plan->timed_launches;
        if (trace)
            slowest = std::max(slowest, std::chrono::duration<double, std::micro>(
                                            std::chrono::steady_clock::now() - a).count());
    }
    timing_end(plan, s);
    tr1 = std::chrono::steady_clock::now();
    for (; checked < launched && failed_at < 0; ++checked) {
        const int v = stream_wait(plan, seq0 + (unsigned int)checked, s, &rm);
        if (v < 0) { rc = v; goto out; }
        if (v == 1) failed_at = checked;
    }
    if (trace) {
        const auto tr2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[revs_plan_stream_run] %d launches in %.1f us (slowest %.1f us), records read "
                "%.1f us later (host away from the wait loop for at most %.1f us), %d kept\n", launched,
                std::chrono::duration<double, std::micro>(tr1 - tr0).count(), slowest,
                std::chrono::duration<double, std::micro>(tr2 - tr1).count(), plan->t_wait,
                failed_at >= 0 ? failed_at : launched);
        plan->t_wait = 0.0;
    }
out:
    plan->stream_seq = seq0 + (unsigned int)std::max(launched, 1) - 1;
    *rmax_last = rm;
    const int kept = rc != REVS_OK ? 0 : (failed_at >= 0 ? failed_at : launched);
    if (failed_at >= 0 || rc != REVS_OK)
        (void)hipStreamSynchronize(s);                   // the launches behind the failed one are no-ops
    *kept_steps = kept;
    stream_rotate(st, kept, d.n_homes);   // the roles, by the kept steps
    return rc;
}
