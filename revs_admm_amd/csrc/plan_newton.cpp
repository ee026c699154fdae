// The native Newton loops of a plan: the chain's acceptance test, the speculative step and its run, the chained
// Newton iteration and its run, the operator's Newton solve (see revs_admm.h).
#include "plan.h"

// Host-side acceptance test of a chained Newton iteration (operator_newton.py: _chain_launch): the
// checks AdmmEngine._operator_solve_newton would make on the two evaluations' stats, for the
// one outcome that needs no further launch.  See include/revs_admm.h.
// why: 0 accepted | 1 everything holds but the rows after the step are still above the tolerance (the
// step itself is a good Newton step: another iteration from it) | 2 anything else
int chain_accept_impl(int32_t T, const double *s0, const double *s1, double scale, double eps,
                      int32_t amax, int32_t kadd, int32_t chain_few, int32_t *nsup_sum,
                      int32_t *nsup_max, int *why) {
    *why = 2;
    if (!s0 || !s1 || T <= 0 || !(scale > 0.0) || !nsup_sum || !nsup_max) return 0;
    double rmax0 = 0.0, ns_max = 0.0, ncand_max = 0.0;
    for (int t = 0; t < T; ++t) {
        const double *a = s0 + 8 * t;
        if (a[2] > amax) return 0;                       // more multipliers than a model holds
        const double r = a[0] / scale;
        rmax0 = r > rmax0 ? r : rmax0;
        if (a[2] >= amax && a[3] > 0 && r > eps) return 0;
        const double room = kadd < amax - a[2] ? kadd : amax - a[2];
        const double nc = a[2] + (a[3] < room ? a[3] : room);
        ncand_max = nc > ncand_max ? nc : ncand_max;
        ns_max = a[2] > ns_max ? a[2] : ns_max;
    }
    if (!(rmax0 > eps)) return 0;                        // already converged: the general path
    if (ncand_max > 8) return 0;                         // not the small model
    if ((ns_max + kadd <= REVS_DUAL_FEW) != (chain_few != 0)) return 0;
    double rmax1 = 0.0, sum = 0.0, mx = 0.0;
    for (int t = 0; t < T; ++t) {
        const double *a = s0 + 8 * t, *b = s1 + 8 * t;
        const double D = a[1];
        if (a[0] / scale > eps &&                        // pending slot: Armijo on the full step
            !(b[1] >= D + 1e-4 * b[4] - 1e-11 * (D < 0 ? -D : D)))
            return 0;
        if (b[2] > amax) return 0;
        const double r = b[0] / scale;
        rmax1 = r > rmax1 ? r : rmax1;
        sum += b[2];
        mx = b[2] > mx ? b[2] : mx;
    }
    *nsup_sum = (int32_t)sum;
    *nsup_max = (int32_t)mx;
    if (!(rmax1 <= eps)) { *why = 1; return 0; }         // needs another iteration
    *why = 0;
    return 1;
}

extern "C" int revs_newton_chain_accept(int32_t T, const double *s0, const double *s1, double scale,
                                        double eps, int32_t amax, int32_t kadd, int32_t chain_few,
                                        int32_t *nsup_sum, int32_t *nsup_max) {
    int why = 0;
    return chain_accept_impl(T, s0, s1, scale, eps, amax, kadd, chain_few, nsup_sum, nsup_max, &why);
}

// The rows of R p and their bookkeeping fit one launch (the tile form: revs_op_dual_product_rows), the
// selection then takes one block per 32-row tile.
static bool rows_one_launch(const revs_plan_desc_t &d) { return d.T <= 32 && (d.m + 31) / 32 <= 256; }

// v = R p_in with the row bookkeeping (one launch when the tile form applies); clears p_out.
static int plan_product(revs_plan_t *plan, const double *y, const double *pin, double *pout,
                        void *stream) {
    const revs_plan_desc_t &d = plan->d;
    if (rows_one_launch(d))
        return revs_op_dual_product_rows(d.m, d.T, d.Rt, pin, d.pnq, y, d.vlo, d.vhi, d.ksplit,
                                         d.v_slabs, d.vfull, d.viol, d.partial, pout, plan->counters,
                                         stream);
    const int r = revs_gemm_tn_f64_split(d.m, d.T, d.m, d.Rt, pin, d.v_slabs, d.ksplit, stream);
    if (r != REVS_OK) return r;
    return revs_op_dual_rows(d.m, d.T, d.ksplit, d.v_slabs, d.pnq, y, d.vlo, d.vhi, d.vfull, d.viol,
                             d.partial, pout, stream);
}

extern "C" int revs_plan_spec_step(revs_plan_t *plan, int32_t phase, const double *y,
                                   int32_t use_y, const float *p_est, float *p_est_new,
                                   const float *p_sch, const float *gamma, float *p_sch_out,
                                   float *gamma_out, float *s_out, float *c_out, int32_t fused_in,
                                   const double *p_in, double *p_out, float *p_est_next,
                                   double *rmax_out, void *ev_mid, void *ev_end, void *stream) {
    if (phase == 64) {                       // a product run ahead, nothing else
        REVS_REQUIRE(plan && y && p_in && p_out && p_in != p_out, "revs_plan_spec_step: bad argument");
        return plan_product(plan, y, p_in, p_out, stream);
    }
    REVS_REQUIRE(plan && phase >= 1 && phase <= 63 && (!(phase & 28) || (phase & 2)) &&
                 (!(phase & 32) || phase == 32) && y && p_est && p_est_new && p_sch && gamma &&
                 p_sch_out && gamma_out && rmax_out && p_in, "revs_plan_spec_step: bad argument");
    REVS_REQUIRE(!(phase & 8) || p_out, "revs_plan_spec_step: running ahead needs p_out");
    const revs_plan_desc_t &d = plan->d;
    const bool fuse_out = p_out != nullptr;
    REVS_REQUIRE(!(fuse_out || fused_in) || (!use_y && d.node_of && (!fuse_out || p_est_next)),
                 "revs_plan_spec_step: fused home pass needs y = 0, node_of and p_est_next");
    REVS_REQUIRE(p_out != p_in && (fused_in || p_in == d.pnq),
                 "revs_plan_spec_step: p_in / p_out inconsistent");
    hipStream_t s = (hipStream_t)stream;
    const auto t_enter = std::chrono::steady_clock::now();
    int rc;
    if ((phase & 1) && !fused_in) {  // home pass of this evaluation (else: the last sweep did it)
        rc = plan_home_pass(d, p_est, p_sch, gamma, y, use_y, -1, p_est_new, stream);
        if (rc != REVS_OK) return rc;
    }
    if (!(phase & (2 | 32))) return REVS_OK;
    const double seq = (phase & 32) ? plan->seq : (plan->seq += 1.0);
    if (!(phase & 32)) {
    // node sums p_in: this evaluation's (from the home pass above, or from the last fused
    // sweep; all-reduced by a sharded caller between the phases); p_out: where this sweep
    // accumulates the next ones -- never the same array, so that clearing the latter cannot
    // race with the product reading the former
    const int sel_nblk = rows_one_launch(d) ? (d.m + 31) / 32 : 0;
    auto product = [&](const double *pin, double *pout) -> int {
        return plan_product(plan, y, pin, pout, stream);
    };
    if (!(phase & 4)) {                              // (else: the previous call ran it ahead)
        rc = product(p_in, p_out);
        if (rc != REVS_OK) return rc;
    }
    if (ev_mid) (void)hipEventRecord((hipEvent_t)ev_mid, s);
    // the candidate selection rides in the sweep's launch (its first T workgroups)
    rc = revs_agent_step_select(d.n_homes, d.T, d.cost, d.homes, d.load, p_est,
                                (d.recompute_pe_new && !use_y) ? nullptr : p_est_new, p_sch,
                                gamma, p_sch_out, gamma_out, s_out, c_out, d.diff, d.dsq,
                                d.status, d.pdhg_dual, (float)d.kappa, d.mode, &d.pdhg, d.m,
                                d.partial, y, d.vlo, d.vhi, d.kadd, d.vfull, d.viol, d.cand_idx,
                                d.cand_cnt, d.cand_val, d.stats, seq, fuse_out ? d.node_of : nullptr,
                                p_out, fuse_out ? p_est_next : nullptr, sel_nblk, stream);
    if (rc != REVS_OK) return rc;
    if (ev_end) (void)hipEventRecord((hipEvent_t)ev_end, s);
    if (phase & 8) {
        // The NEXT iteration's product, before this one's verdict is known: it needs only the
        // node sums this sweep leaves in p_out, and it keeps the queue from running dry while
        // the host turns around (a restart costs the stream ~6 us).  It clears the array that
        // held this evaluation's sums.  If this sweep is discarded it has computed nothing
        // anyone reads: the caller's next evaluation rewrites every array it touches.
        rc = product(p_out, const_cast<double *>(p_in));
        if (rc != REVS_OK) return rc;
    }
    if (phase & 16) return REVS_OK;          // the caller waits with a phase-32 call
    }
    // Wait for the evaluation, not the sweep (the select kernel tags the stats block).
    const volatile double *st = d.stats_host;
    const auto t0 = std::chrono::steady_clock::now();
    plan->t_launch += std::chrono::duration<double, std::micro>(t0 - t_enter).count();
    if ((rc = wait_tags(st, d.T, seq, s, "revs_plan_spec_step", "the evaluation", t0)) != REVS_OK) return rc;
    plan->t_wait += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    double mx = 0.0;
    for (int t = 0; t < d.T; ++t) mx = st[8 * t] > mx ? st[8 * t] : mx;
    *rmax_out = mx;
    return REVS_OK;
}

extern "C" int revs_plan_chain_step(revs_plan_t *plan, const double *y, double *y_trial,
                                    int32_t use_y, int32_t sup0, int32_t chain_few,
                                    const float *p_est, float *p_est_new, const float *p_sch,
                                    const float *gamma, float *p_sch_out, float *gamma_out,
                                    float *s_out, float *c_out, int32_t *accepted,
                                    int32_t *nsup_sum, int32_t *nsup_max, void *ev_mid,
                                    void *ev_end, void *stream) {
    REVS_REQUIRE(plan && y && y_trial && y != y_trial && p_est && p_est_new && p_sch && gamma &&
                 p_sch_out && gamma_out && accepted && nsup_sum && nsup_max && sup0 >= -1 && sup0 <= 1,
                 "revs_plan_chain_step: bad argument");
    const revs_plan_desc_t &d = plan->d;
    REVS_REQUIRE(d.cand_idx1 && d.cand_cnt1 && d.cand_val1 && d.stats1 && d.stats1_host && d.yhat &&
                 d.k_full && d.info && d.max_pivots > 0 && d.eps > 0,
                 "revs_plan_chain_step: the plan was created without the chain's buffers");
    hipStream_t s = (hipStream_t)stream;
    const PlanSet S[2] = {plan_set(d, 0), plan_set(d, 1)};
    const double scale = plan_scale(d);
    int sel_nblk = rows_one_launch(d) ? (d.m + 31) / 32 : 0;
    // home pass of an evaluation of multipliers yy: row-wise from the lists of set `sup`, or dense
    auto home_pass = [&](const double *yy, int uy, int sup) -> int {
        return plan_home_pass(d, p_est, p_sch, gamma, yy, uy, sup, p_est_new, stream);
    };
    // product R p and the row bookkeeping; the selection is left to the next launch
    // (a feeder of more than REVS_TREE_SWEEP_MAX nodes: the fused launches below do not hold it, its rows still come
    // from the tree form -- one block of partial sums per slot)
    const bool big_tree = plan->tree.n > REVS_TREE_SWEEP_MAX;
    const revs_tree_t tr = plan_tree(plan);
    if (big_tree) sel_nblk = 1;
    auto rows = [&](const double *yy, int uy, int k) -> int {
        if (big_tree)
            return revs_op_dual_rows_tree(d.m, d.T, &tr, d.pnq, yy, d.vlo, d.vhi, d.kadd, d.vfull, d.viol, d.partial,
                                          nullptr, S[k].ci, S[k].cc, S[k].cv, S[k].st, 0.0, 0, stream);
        return revs_op_dual_evaluate(2 | 4, d.m, d.T, d.node_ptr, p_est, p_sch, gamma, d.R, d.Rt, yy, uy,
                                     d.kappa, d.vlo, d.vhi, d.kadd, d.ksplit, d.d_slabs, d.v_slabs,
                                     d.pnq, p_est_new, d.vfull, d.viol, d.partial, S[k].ci, S[k].cc, S[k].cv,
                                     S[k].st, 0.0, plan->counters, stream);
    };
    // With the feeder as a tree the operator side between the home passes is the tree form of R p:
    // rows, selection, small model and step of every slot in ONE launch of T workgroups, the trial's
    // rows in another (its selection rides in the sweep's launch) -- no matrix stream at all.
    const bool tf = plan->tree.n > 0 && plan->tree.n <= REVS_TREE_SWEEP_MAX;
    int rc;
    if ((rc = home_pass(y, use_y, sup0)) != REVS_OK) return rc;
    if (tf) {
        rc = revs_op_dual_tree_select_model_step(d.m, d.T, &tr, d.pnq, y, d.vlo, d.vhi, d.kadd, d.vfull, d.viol,
                                                 d.partial, S[0].ci, S[0].cc, S[0].cv, S[0].st, 0.0, d.R, d.kappa,
                                                 d.delta, d.max_pivots, d.k_full, d.yhat, d.info, scale, d.eps, y_trial,
                                                 S[1].st + 4, stream);
    } else {
        if ((rc = rows(y, use_y, 0)) != REVS_OK) return rc;
        rc = revs_op_dual_select_model_step(d.m, d.T, d.partial, sel_nblk, y, d.vlo, d.vhi, d.kadd, d.vfull,
                                            d.viol, S[0].ci, S[0].cc, S[0].cv, S[0].st, 0.0, d.R,
                                            d.pnq + (int64_t)d.m * d.T, d.kappa, d.delta, d.max_pivots,
                                            d.k_full, d.yhat, d.info, scale, d.eps, y_trial, S[1].st + 4,
                                            stream);
    }
    if (rc != REVS_OK) return rc;
    if ((rc = home_pass(y_trial, 1, chain_few ? 0 : -1)) != REVS_OK) return rc;
    if (tf)
        rc = revs_op_dual_rows_tree(d.m, d.T, &tr, d.pnq, y_trial, d.vlo, d.vhi, d.kadd, d.vfull, d.viol, d.partial,
                                    nullptr, S[1].ci, S[1].cc, S[1].cv, S[1].st, 0.0, 0, stream);
    else
        rc = rows(y_trial, 1, 1);
    if (rc != REVS_OK) return rc;
    if (ev_mid) (void)hipEventRecord((hipEvent_t)ev_mid, s);
    const double seq = -(plan->seq += 1.0);          // (negative: not a spec-step tag)
    rc = revs_agent_step_select(d.n_homes, d.T, d.cost, d.homes, d.load, p_est, p_est_new, p_sch,
                                gamma, p_sch_out, gamma_out, s_out, c_out, d.diff, d.dsq, d.status,
                                d.pdhg_dual, (float)d.kappa, d.mode, &d.pdhg, d.m, d.partial, y_trial,
                                d.vlo, d.vhi, d.kadd, d.vfull, d.viol, S[1].ci, S[1].cc, S[1].cv, S[1].st, seq,
                                nullptr, nullptr, nullptr, tf ? 1 : sel_nblk, stream);
    if (rc != REVS_OK) return rc;
    if (ev_end) (void)hipEventRecord((hipEvent_t)ev_end, s);
    if ((rc = wait_tags(d.stats1_host, d.T, seq, s, "revs_plan_chain_step", "the evaluation")) != REVS_OK) return rc;
    *accepted = revs_newton_chain_accept(d.T, d.stats_host, d.stats1_host, scale, d.eps,
                                         REVS_DUAL_AMAX, d.kadd, chain_few, nsup_sum, nsup_max);
    return REVS_OK;
}

extern "C" int revs_plan_spec_run(revs_plan_t *plan, int32_t max_steps, const double *y,
                                  revs_spec_state_t *st, double scale, double eps,
                                  int32_t *kept_steps, int32_t *last_fused_in, double *rmax_out,
                                  void *stream) {
    REVS_REQUIRE(plan && max_steps >= 0 && y && st && kept_steps && last_fused_in && rmax_out &&
                 scale > 0.0 && st->p_est && st->p_est_new && st->p_est_alt && st->p_sch &&
                 st->p_sch_alt && st->gamma && st->gamma_alt && st->p0 && st->p_alt &&
                 st->p0 != st->p_alt && st->p0 == plan->d.pnq &&
                 (!st->fused_ready || st->fused_p == st->p0 || st->fused_p == st->p_alt),
                 "revs_plan_spec_run: bad argument");
    *kept_steps = 0;
    *last_fused_in = 0;
    *rmax_out = 0.0;
    bool ahead = false;                    // this iteration's product is already in the queue
    static const bool trace = getenv("REVS_PLAN_TRACE") != nullptr;
    const auto tr0 = std::chrono::steady_clock::now();
    for (int32_t k = 0; k < max_steps; ++k) {
        const int32_t fused_in = st->fused_ready;
        const double *p_in = fused_in ? st->fused_p : st->p0;
        double *p_out = p_in == st->p0 ? st->p_alt : st->p0;
        double rm = 0.0;
        const int32_t phase = 3 | (ahead ? 4 : 0) | (k + 1 < max_steps ? 8 : 0);
        ahead = (phase & 8) != 0;
        const int rc = revs_plan_spec_step(plan, phase, y, 0, st->p_est, st->p_est_new, st->p_sch, st->gamma,
                                           st->p_sch_alt, st->gamma_alt, nullptr, nullptr, fused_in, p_in,
                                           p_out, st->p_est_alt, &rm, nullptr, nullptr, stream);
        if (rc != REVS_OK) return rc;
        *rmax_out = rm;
        if (!(rm / scale <= eps)) {          // discard: the caller finishes this iteration
            *last_fused_in = fused_in;
            return REVS_OK;
        }
        std::swap(st->p_sch, st->p_sch_alt);
        std::swap(st->gamma, st->gamma_alt);
        st->fused_ready = 1;
        st->fused_p = p_out;
        std::swap(st->p_est, st->p_est_new);
        std::swap(st->p_est_new, st->p_est_alt);
        ++*kept_steps;
    }
    if (trace && *kept_steps > 0) {
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr0).count();
        fprintf(stderr, "[revs_plan_spec_run] %d steps, %.2f us per step on the host; launches %.2f us, "
                "waiting %.2f us per step\n", *kept_steps, us / *kept_steps, plan->t_launch / *kept_steps,
                plan->t_wait / *kept_steps);
        plan->t_launch = plan->t_wait = 0.0;
    }
    return REVS_OK;
}

// ---- the operator's Newton solve as one native call (see revs_admm.h) ---------------------------
extern "C" int revs_plan_set_newton(revs_plan_t *plan, const revs_newton_opts_t *o) {
    REVS_REQUIRE(plan && o && o->k_slabs && o->nks >= 1 && o->nks <= 64 && o->alpha_host && o->alpha_dev && o->info_host &&
                 o->newton_max >= 1 && o->ls_max >= 1, "revs_plan_set_newton: bad argument");
    plan->newton = *o;
    return REVS_OK;
}

extern "C" int revs_plan_newton_solve(revs_plan_t *plan, revs_newton_state_t *st, void *stream) {
    REVS_REQUIRE(plan && st && st->y && st->y_trial && st->y != st->y_trial && st->p_est && st->p_sch && st->gamma &&
                 st->p_est_new && st->sup >= -1 && st->sup <= 1, "revs_plan_newton_solve: bad argument");
    const revs_plan_desc_t &d = plan->d;
    const revs_newton_opts_t &o = plan->newton;
    REVS_REQUIRE(o.k_slabs && d.cand_idx1 && d.cand_cnt1 && d.cand_val1 && d.stats && d.stats_host && d.stats1 && d.stats1_host && d.yhat && d.k_full &&
                 d.info && d.max_pivots > 0 && d.eps > 0, "revs_plan_newton_solve: revs_plan_set_newton / the chain's buffers are missing");
    const int T = d.T, A = REVS_DUAL_AMAX;
    REVS_REQUIRE(T <= REVS_ENS_MAX_COLS, "revs_plan_newton_solve: T = %d", T);
    // the blocks the caller refers to still hold the evaluations it saw (every slot's record carries the evaluation's tag)
    for (int blk = 0; blk < 2; ++blk) {
        const double want = blk ? st->pre_tag : st->first_tag;
        if (!(blk ? st->have_pre : st->have_first) || want == 0.0) continue;
        const volatile double *b = blk ? d.stats1_host : d.stats_host;
        for (int t = 0; t < T; ++t)
            REVS_REQUIRE(b[8 * t + 5] == want, "revs_plan_newton_solve: stats block %d no longer holds evaluation %g (slot %d carries %g)",
                         blk, want, t, (double)b[8 * t + 5]);
    }
    hipStream_t s = (hipStream_t)stream;
    const PlanSet S[2] = {plan_set(d, 0), plan_set(d, 1)};
    const double scale = plan_scale(d);
    const int64_t mt = (int64_t)d.m * T;
    const bool tf = plan->tree.n > 0;     // rows by the tree form of R p (every shape: revs_op_dual_rows_tree)
    const revs_tree_t trh = plan_tree(plan);
    double *ycur = st->y, *ytrial = st->y_trial;
    // One evaluation of multipliers yy (p, N, D, the voltage rows, candidate lists and stats into set k; P_est_new =
    // the answer for yy), waited for: the selection tags the pinned stats block behind a system-scope fence.
    auto evaluate = [&](const double *yy, int uy, int k, int sup, double *out /* [T][8] */, int kadd) -> int {
        const double tag = (plan->seq += 1.0) + 0.25;      // (Python's evaluations: n + 0.5; the other native loops: whole numbers)
        auto phase = [&](int ph) -> int {
            if (tf)
                return revs_op_dual_evaluate_tree(ph, d.m, T, d.node_ptr, st->p_est, st->p_sch, st->gamma, d.R, &trh, yy, uy,
                                                  d.kappa, d.vlo, d.vhi, kadd, d.ksplit, d.d_slabs, d.pnq, st->p_est_new, d.vfull,
                                                  d.viol, d.partial, S[k].ci, S[k].cc, S[k].cv, S[k].st, tag, stream);
            return revs_op_dual_evaluate(ph, d.m, T, d.node_ptr, st->p_est, st->p_sch, st->gamma, d.R, d.Rt, yy, uy, d.kappa,
                                         d.vlo, d.vhi, kadd, d.ksplit, d.d_slabs, d.v_slabs, d.pnq, st->p_est_new, d.vfull, d.viol,
                                         d.partial, S[k].ci, S[k].cc, S[k].cv, S[k].st, tag, plan->counters, stream);
        };
        int rc;
        if (uy && sup >= 0) {             // few multipliers: shifts straight from their rows of R, no dense product
            rc = plan_home_pass(d, st->p_est, st->p_sch, st->gamma, yy, uy, sup, st->p_est_new, stream);
            if (rc == REVS_OK && plan->comm) rc = revs_comm_allreduce_f64(plan->comm, d.pnq, 3 * mt, 0, stream);
            if (rc == REVS_OK) rc = phase(2);
        } else if (!plan->comm) {
            rc = phase(3);
        } else {
            rc = phase(1);
            if (rc == REVS_OK) rc = revs_comm_allreduce_f64(plan->comm, d.pnq, 3 * mt, 0, stream);      // the only exchange
            if (rc == REVS_OK) rc = phase(2);
        }
        if (rc != REVS_OK) return rc;
        const volatile double *tg = S[k].st_host;
        if ((rc = wait_tags(tg, T, tag, s, "revs_plan_newton_solve", "an evaluation")) != REVS_OK) return rc;
        for (int i = 0; i < 8 * T; ++i) out[i] = tg[i];
        return REVS_OK;
    };
    std::vector<double> stt(8 * (size_t)T), stn(8 * (size_t)T), alpha((size_t)T), Dv((size_t)T);
    std::vector<char> pending((size_t)T);
    int cur = 0, rc = REVS_OK;
    if (st->have_first) for (int i = 0; i < 8 * T; ++i) stt[i] = d.stats_host[i];
    else if ((rc = evaluate(ycur, st->use_y, 0, st->use_y ? st->sup : -1, stt.data(), d.kadd)) != REVS_OK) return rc;
    // Rows admitted to a slot's model per Newton iteration: d.kadd (2: the warm solves' models stay small) -- but
    // plan->kadd_cold while some slot still shows more than plan->kadd_cold_at violated rows without a multiplier (a cold
    // solve: admitting two at a time makes it as many Newton iterations as half the rows that end up binding).
    // kadd_stt: what the evaluation behind `stt` admitted with (its candidate lists are that long).
    // ... and only while the rows admitted last time nearly all kept a multiplier (kept >= 0.5) or some slot already carries
    // 16 of them: rows that bind one by one, the 121144 feeder; on long laterals a handful of multipliers clears hundreds of
    // violated rows, most admitted rows end without one and a slot ends with 3-4 multipliers: there the small lists stay.
    int kadd_stt = d.kadd;
    double ns_prev = 0.0, adm_prev = 0.0;
    bool have_prev = false;
    int evals = 1, newton = 0, pivots = 0, stall = 0, n_small = 0, n_general = 0;
    bool ok_all = false, last_small = false, few = false, from_pre = st->have_pre != 0, big_needed = false;
    double best = INFINITY;
    for (;;) {
        double rmax = 0.0, ns_max = 0.0, nc_max = 0.0, nv_max = 0.0, ns_sum = 0.0, adm_now = 0.0;
        bool over = false, full = false;
        for (int t = 0; t < T; ++t) {
            const double *a = &stt[8 * t];
            if (a[2] > A) over = true;                           // more multipliers than a model holds
            const double r = a[0] / scale;
            rmax = std::max(rmax, r);
            // a slot whose model is full of multipliers while rows are still violated cannot take them in
            if (a[2] >= A && a[3] > 0 && r > d.eps) full = true;
            ns_max = std::max(ns_max, a[2]);
            nc_max = std::max(nc_max, a[2] + std::min(a[3], std::min((double)kadd_stt, A - a[2])));
            nv_max = std::max(nv_max, a[3]);
            ns_sum += a[2];
            adm_now += std::min(a[3], std::min((double)kadd_stt, A - a[2]));
        }
        const double kept = have_prev ? (ns_sum - ns_prev) / std::max(adm_prev, 1.0) : 0.0;
        if (over || full) big_needed = true;
        const int kadd_next = (plan->kadd_cold > d.kadd && nv_max > plan->kadd_cold_at && (kept >= 0.5 || ns_max >= 16.0)) ? plan->kadd_cold : d.kadd;
        ns_prev = ns_sum; adm_prev = adm_now; have_prev = true;
        if (over) break;
        if (rmax <= d.eps) { ok_all = true; break; }
        if (newton >= o.newton_max || full) break;
        // ... and a solve that stopped improving is not worth more iterations
        if (rmax < 0.5 * best) { best = rmax; stall = 0; }
        else if (++stall >= 10) break;
        ++newton;
        last_small = nc_max <= 8;
        few = ns_max + kadd_stt <= REVS_DUAL_FEW;
        // (the chain guessed how its trial's home pass gets d = R^T y / kappa -- row-wise or dense; another choice here
        // would differ in the last bits: then the trial is made again)
        const bool use_pre = st->have_pre && newton == 1 && last_small && few == (st->chain_few_in != 0);
        if (!use_pre) {
            if (last_small) {
                ++n_small;
                rc = revs_op_dual_model_small(d.m, T, d.R, d.pnq + mt, S[cur].ci, S[cur].cc, S[cur].cv, d.kappa, d.delta,
                                              d.max_pivots, d.k_full, d.yhat, d.info, stream);
            } else {
                ++n_general;
                rc = revs_op_dual_model(d.m, T, d.R, d.pnq + mt, S[cur].ci, S[cur].cc, S[cur].cv, d.kappa, d.delta,
                                        d.max_pivots, o.nks, o.k_slabs, d.k_full, d.yhat, d.info, stream);
            }
            if (rc != REVS_OK) return rc;
        } else {
            ++n_small;                                            // (the chain ran this model on this set)
        }
        bool any_pending = false;
        for (int t = 0; t < T; ++t) {
            Dv[t] = stt[8 * t + 1];
            pending[t] = stt[8 * t] / scale > d.eps;
            alpha[t] = pending[t] ? 1.0 : 0.0;
        }
        const int nxt = 1 - cur;
        int kadd_stn = kadd_next;
        for (int ls = 0; ls < o.ls_max; ++ls) {
            kadd_stn = (use_pre && ls == 0) ? d.kadd : kadd_next;      // (the chain's trial admitted with the plan's own)
            if (use_pre && ls == 0) {
                for (int i = 0; i < 8 * T; ++i) stn[i] = d.stats1_host[i];      // that trial and its evaluation: already there
            } else {
                from_pre = false;
                for (int t = 0; t < T; ++t) o.alpha_host[t] = alpha[t];        // read by the step kernel through its mapping
                // (the trial starts from the current multipliers: copied by the step's own launch)
                rc = revs::dual_step_copy(T, S[cur].ci, S[cur].cc, S[cur].cv, d.yhat, o.alpha_dev, ycur, d.m, ytrial,
                                          S[nxt].st + 4, stream);
                if (rc == REVS_OK) rc = evaluate(ytrial, 1, nxt, few ? cur : -1, stn.data(), kadd_next);
                if (rc != REVS_OK) return rc;
            }
            ++evals;
            // (slack 1e-11 |D|: the evaluations sum the squares rounded to 2^-32 so that the sums do not depend on their
            // order -- a rounding of ~1e-13 |D| per evaluation)
            any_pending = false;
            for (int t = 0; t < T; ++t) {
                const bool okk = stn[8 * t + 1] >= Dv[t] + 1e-4 * stn[8 * t + 4] - 1e-11 * std::fabs(Dv[t]);
                if (okk) pending[t] = 0;
                if (pending[t]) { any_pending = true; alpha[t] *= 0.5; }
            }
            if (!any_pending) break;
        }
        for (int t = 0; t < T; ++t) pivots += std::abs(o.info_host[t]);     // (the evaluation was waited for)
        if (any_pending) break;                                   // no ascent found: leave it to the ADMM forms
        std::swap(ycur, ytrial);
        cur = nxt;
        stt.swap(stn);
        kadd_stt = kadd_stn;
    }
    st->y = ycur;
    st->y_trial = ytrial;
    st->ok = ok_all;
    st->newton = newton;
    st->evals = evals;
    st->pivots = pivots;
    st->models_small = n_small;
    st->models_general = n_general;
    st->last_small = last_small;
    st->few = newton >= 1 ? (few ? 1 : 0) : 0;
    st->pre_kept = ok_all && from_pre && newton <= 1;
    st->cur = cur;
    double sum = 0.0, mx = 0.0;
    for (int t = 0; t < T; ++t) { sum += stt[8 * t + 2]; mx = std::max(mx, stt[8 * t + 2]); }
    st->nsup_sum = (int32_t)sum;
    st->nsup_max = (int32_t)mx;
    st->big_needed = big_needed ? 1 : 0;
    st->reserved_ = 0;
    if (!ok_all && !big_needed && hipMemsetAsync(ycur, 0, sizeof(double) * mt, s) != hipSuccess) {
        revs::set_error("revs_plan_newton_solve: clearing the multipliers failed");
        return REVS_ELAUNCH;
    }
    return REVS_OK;
}

extern "C" int revs_plan_chain_run(revs_plan_t *plan, int32_t max_steps, revs_chain_state_t *st,
                                   int32_t chain_few, int32_t *kept_steps, void *stream) {
    REVS_REQUIRE(plan && max_steps >= 0 && st && kept_steps && st->y && st->y_trial && st->p_est &&
                 st->p_est_new && st->p_sch && st->p_sch_alt && st->gamma && st->gamma_alt,
                 "revs_plan_chain_run: bad argument");
    *kept_steps = 0;
    for (int32_t k = 0; k < max_steps; ++k) {
        int32_t acc = 0, nsum = 0, nmax = 0;
        const int rc = revs_plan_chain_step(plan, st->y, st->y_trial, st->use_y, st->sup0, chain_few,
                                            st->p_est, st->p_est_new, st->p_sch, st->gamma,
                                            st->p_sch_alt, st->gamma_alt, nullptr, nullptr, &acc, &nsum,
                                            &nmax, nullptr, nullptr, stream);
        if (rc != REVS_OK) return rc;
        if (!acc) return REVS_OK;              // the caller's general loop takes this iteration
        std::swap(st->y, st->y_trial);
        st->use_y = nsum > 0;
        st->sup0 = (nsum > 0 && nmax + plan->d.kadd <= REVS_DUAL_FEW) ? 1 : -1;
        std::swap(st->p_sch, st->p_sch_alt);
        std::swap(st->gamma, st->gamma_alt);
        std::swap(st->p_est, st->p_est_new);
        ++*kept_steps;
    }
    return REVS_OK;
}
