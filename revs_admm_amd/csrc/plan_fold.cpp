// The folded chain: the binding steady state with one pass over the residences per ADMM iteration.
#include "plan.h"
#include <cstring>

// The binding steady state with ONE pass over the residences per ADMM iteration (see revs_admm.h).
// Per iteration k (parity par = k & 1, candidate sets / stats S0[par], S1[par]):
//   sweep     the residences' iteration with the operator's answer for the trial multipliers formed
//             inside (shifts from S0[par]'s lists), P_sch / G to the spares, pen to p_est_new; folds
//             the trial's node sums into fold_e2[par] and the sums of the same multipliers on the
//             new state into fold_e1[par ^ 1]
//   KV        [0, T): rows + selection of the trial -> S1[par] (the verdict the host polls);
//             [T, 2T): rows, selection, small model, step of iteration k + 1 -> S0[par ^ 1], the
//             next trial in y_spare; clears fold_e2[par ^ 1], fold_e1[par]
// then revs_newton_chain_accept on S0[par], S1[par]; accepted: roles rotate and iteration k + 1
// starts with its sweep -- its operator work is done.  The first iteration of a call that does not
// resume evaluates the multipliers with the evaluation kernel first.
int fold_alloc(revs_plan_t *plan) {
    const revs_plan_desc_t &d = plan->d;
    if (plan->fold_e2[0]) return REVS_OK;
    const size_t mt = (size_t)d.m * d.T;
    hipError_t e = hipSuccess;
    auto dev = [&](void **p, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
    };
    for (int i = 0; i < 2; ++i) {
        // the two sum arrays one sweep accumulates into -- fold_e2[par] | fold_e1[par ^ 1] -- are one
        // allocation: sharded, ONE all-reduce per iteration covers both
        // (double[m][T][4] = {p, N, q, 0} each)
        dev((void **)&plan->fold_e2[i], sizeof(double) * 8 * mt);
        if (e == hipSuccess) plan->fold_e1[i ^ 1] = plan->fold_e2[i] + 4 * mt;
        dev((void **)&plan->fold_ci[i], sizeof(int64_t) * (size_t)d.T * REVS_DUAL_AMAX);
        dev((void **)&plan->fold_cc[i], sizeof(int32_t) * (size_t)d.T);
        dev((void **)&plan->fold_cv[i], sizeof(double) * (size_t)d.T * 3 * REVS_DUAL_AMAX);
        if (e == hipSuccess) {
            void *h = nullptr, *dp = nullptr;
            e = hipHostMalloc(&h, sizeof(double) * 8 * (size_t)d.T, hipHostMallocMapped);
            if (e == hipSuccess) {
                memset(h, 0, sizeof(double) * 8 * (size_t)d.T);
                e = hipHostGetDevicePointer(&dp, h, 0);
            }
            plan->fold_st_host[i] = (double *)h;
            plan->fold_st_dev[i] = (double *)dp;
        }
    }
    dev((void **)&plan->fold_st_local[0], sizeof(double) * 8 * (size_t)d.T);
    dev((void **)&plan->fold_st_local[1], sizeof(double) * 8 * (size_t)d.T);
    dev((void **)&plan->fold_v[0], sizeof(double) * mt);
    dev((void **)&plan->fold_v[1], sizeof(double) * mt);
    dev((void **)&plan->fold_v[2], sizeof(double) * (size_t)d.T * 4);
    dev((void **)&plan->fold_info[0], sizeof(int32_t) * (size_t)d.T);
    dev((void **)&plan->fold_info[1], sizeof(int32_t) * (size_t)d.T);
    dev((void **)&plan->fold_sh[0], sizeof(double) * mt);
    dev((void **)&plan->fold_sh[1], sizeof(double) * (mt + 32 * (size_t)d.T));     // (+ the tuning build's stage stamps)
    if (e != hipSuccess) {
        revs::set_error("revs_plan_chain_fold_run: allocating the folded chain's buffers: %s", hipGetErrorString(e));
        return REVS_ELAUNCH;
    }
    return REVS_OK;
}

extern "C" int revs_plan_chain_fold_run(revs_plan_t *plan, int32_t max_steps, revs_chain_fold_state_t *st,
                                        int32_t *kept_steps, void *stream) {
    REVS_REQUIRE(plan && max_steps >= 0 && st && kept_steps && st->y && st->y_trial && st->y_spare &&
                 st->y != st->y_trial && st->y != st->y_spare && st->y_trial != st->y_spare && st->p_est &&
                 st->p_est_new && st->p_sch && st->p_sch_alt && st->gamma && st->gamma_alt,
                 "revs_plan_chain_fold_run: bad argument");
    const revs_plan_desc_t &d = plan->d;
    REVS_REQUIRE(plan->tree.n > 0 && plan->tree.n <= REVS_TREE_SWEEP_MAX && d.node_of && d.cand_idx1 && d.cand_cnt1 &&
                 d.cand_val1 && d.stats1 && d.stats1_host && d.yhat && d.k_full && d.info && d.max_pivots > 0 &&
                 d.eps > 0 && !d.pdhg.full_rows,
                 "revs_plan_chain_fold_run: needs the feeder as a tree (at most %d nodes), node_of, the chain's "
                 "buffers and the presolved PDHG form", REVS_TREE_SWEEP_MAX);
    REVS_REQUIRE(d.m <= REVS_CHAIN_FOLD_MAX_M, "revs_plan_chain_fold_run: m = %d constraint nodes, the folded chain's "
                 "operator launch holds %d (use revs_plan_chain_run)", d.m, REVS_CHAIN_FOLD_MAX_M);
    *kept_steps = 0;
    if (fold_alloc(plan) != REVS_OK) return REVS_ELAUNCH;
    hipStream_t s = (hipStream_t)stream;
    auto set_of = [&](int par, int which) -> PlanSet {
        if (par == 0) return plan_set(d, which);
        return PlanSet{plan->fold_ci[which], plan->fold_cc[which], plan->fold_cv[which], plan->fold_st_dev[which],
                       plan->fold_st_host[which]};
    };
    const double scale = plan_scale(d);
    const int64_t mt = (int64_t)d.m * d.T;
    bool have_k1 = st->resume != 0 && plan->fold_ready;
    int par = have_k1 ? plan->fold_par : 0;
    plan->fold_ready = false;
    st->resume = 0;
    int rc = REVS_OK;
    st->redone = 0;
    st->pivots = 0;
    // redo: Newton steps beyond the first that the current iteration has taken.  A trial that passes the
    // line search but leaves the rows above the tolerance IS the general loop's next Newton iterate, and its
    // evaluation on the current state is what the sweep has just folded (fold_e2[par]): the operator launch
    // without a verdict half runs rows / selection / model / step on those sums, and the iteration's sweep
    // and operator launch are made again from there -- the general loop's iterates, without its round trips.
    int redo = 0;
    bool redo_pending = false;
    const int kMaxRedo = plan->fold_redo;
    // Sweeps enqueued ahead of their iteration's turn (st->p_est_3 ...): `swept` = this iteration's sweep is in the
    // queue already.  Every sweep ORs its residences' status bits into its own host-visible word (three rotate: at
    // most two sweeps are unjudged at any time); a word joins the sticky one when its iteration is kept.
    REVS_REQUIRE((st->p_est_3 != nullptr) == (st->p_sch_3 != nullptr) && (st->p_est_3 != nullptr) == (st->gamma_3 != nullptr),
                 "revs_plan_chain_fold_run: the third set of state buffers is all three or none");
#ifdef REVS_TUNING        // (debugging aids of tuning builds; the product build has no process-wide toggles in this loop)
    static const bool no_spec = getenv("REVS_FOLD_NO_SPEC") != nullptr;
#else
    constexpr bool no_spec = false;
#endif
    const bool can_spec = st->p_est_3 != nullptr && !no_spec;
    bool swept = false;
    unsigned int sweep_no = 0;
    volatile unsigned int *const fwords = plan->flags_host ? (volatile unsigned int *)plan->flags_host + 1 : nullptr;
    if (fwords) fwords[0] = fwords[1] = fwords[2] = 0u;
    const bool warm = d.mode == REVS_MODE_RELAXED_PDHG && d.pdhg_dual != nullptr;
    REVS_REQUIRE(!warm || !st->pdhg_dual || (st->pdhg_dual == d.pdhg_dual && st->pdhg_dual_new && st->pdhg_dual_new != st->pdhg_dual &&
                                              (!st->p_est_3 || (st->pdhg_dual_3 && st->pdhg_dual_3 != st->pdhg_dual &&
                                                                st->pdhg_dual_3 != st->pdhg_dual_new))),
                 "revs_plan_chain_fold_run: pdhg_dual must be the plan's, with distinct spares");
    const bool ybuf = warm && st->pdhg_dual != nullptr;      // (else: updated in place, as before round 4)
    revs::SweepCall call = plan_sweep_call(d, stream);       // (what no launch of this run changes)
    call.diff = d.diff;
    auto sweep = [&](int parity, const float *pe, const float *ps, const float *gm, float *pe_out, float *ps_out, float *gm_out,
                     float *s_out, float *c_out, float *y_in, float *y_out) -> int {
        revs::ChainFold cf{plan->fold_sh[0], plan->fold_sh[1], d.m, d.kappa, plan->fold_e2[parity],
                           plan->fold_e1[parity ^ 1], pe_out};
        cf.y_out = ybuf ? y_out : nullptr;
        cf.wg_order = plan_wg_order(plan);
        call.p_est_old = pe;
        call.p_sch = ps; call.gamma = gm;
        call.p_sch_out = ps_out; call.gamma_out = gm_out;
        call.s_out = s_out; call.c_out = c_out;
        call.pdhg_dual = ybuf ? y_in : d.pdhg_dual;
        call.flags = plan->flags_dev ? plan->flags_dev + 1 + sweep_no % 3u : nullptr;
        int r = revs::agent_step_chain(call, cf);
        ++sweep_no;
        // Residences sharded: every rank's sweep has folded its own residences' addends -- exact and order-independent
        // (revs_q36 / revs_q32), so the all-reduced sums are the one-process sums bit for bit.  Both arrays in ONE
        // collective per iteration (8 M T doubles: {p, N, q, 0} per slot and node, twice); everything behind it is
        // replicated and deterministic.
        if (r == REVS_OK && plan->comm) r = revs_comm_allreduce_f64(plan->comm, plan->fold_e2[parity], 8 * mt, 0, stream);
        return r;
    };
    // The operator launch without a verdict half: rows, selection, small model, step and the trial's shifts of the
    // evaluation whose node sums are `e1` (layout `es`, see revs::ChainKvSide) -- no trial to judge.  Then the arrays
    // this iteration's sweep accumulates into are cleared: they start from zero.
    auto operator_first = [&](const double *e1, int32_t es, const PlanSet &S0, const PlanSet &S1) -> int {
        revs::ChainKv c0 = chain_kv_common(plan, scale);
        c0.e1 = revs::ChainKvSide{e1, st->y, d.vfull, d.viol, d.partial, S0.ci, S0.cc, S0.cv, S0.st, 0.0, es};
        plan->fold_st_local_valid = false;      // (this launch writes the host block itself)
        c0.info = plan->fold_info[par];
        c0.y_trial = st->y_trial;
        c0.lin_out = S1.st + 4;
        const int r = revs::chain_kv_launch(c0, stream);
        if (r != REVS_OK) return r;
        if (hipMemsetAsync(plan->fold_e2[par], 0, sizeof(double) * 4 * mt, s) != hipSuccess ||
            hipMemsetAsync(plan->fold_e1[par ^ 1], 0, sizeof(double) * 4 * mt, s) != hipSuccess) {
            revs::set_error("revs_plan_chain_fold_run: hipMemsetAsync failed");
            return REVS_ELAUNCH;
        }
        return REVS_OK;
    };
    for (int32_t k = 0; k < max_steps; ++k) {
        const PlanSet S0 = set_of(par, 0), S1 = set_of(par, 1), S0n = set_of(par ^ 1, 0), S1n = set_of(par ^ 1, 1);
        if (redo_pending) {
            redo_pending = false;
            if ((rc = operator_first(plan->fold_e2[par], 4, S0, S1)) != REVS_OK) return rc;
        } else if (!have_k1) {
            // entry: the multipliers' evaluation by the evaluation kernel (row-wise shifts from the
            // caller's list `sup0` when it has one), rows / selection / model / step in one launch
            rc = plan_home_pass(d, st->p_est, st->p_sch, st->gamma, st->y, st->use_y, st->sup0, st->p_est_new, stream);
            if (rc != REVS_OK) return rc;
            if (plan->comm && (rc = revs_comm_allreduce_f64(plan->comm, d.pnq, 3 * mt, 0, stream)) != REVS_OK) return rc;
            if ((rc = operator_first(d.pnq, 1, S0, S1)) != REVS_OK) return rc;
        }
        const unsigned int word_k = swept ? (sweep_no - 1u) % 3u : sweep_no % 3u;      // this iteration's sweep's status word
        if (!swept) {
            rc = sweep(par, st->p_est, st->p_sch, st->gamma, st->p_est_new, st->p_sch_alt, st->gamma_alt, st->s_out, st->c_out,
                       st->pdhg_dual, st->pdhg_dual_new);
            if (rc != REVS_OK) return rc;
        }
        swept = false;
        const double seq = -(plan->seq += 1.0);
        revs::ChainKv c = chain_kv_common(plan, scale);
        c.has_e2 = 1;
        c.e2 = revs::ChainKvSide{plan->fold_e2[par], st->y_trial, plan->fold_v[0], plan->fold_v[1], plan->fold_v[2],
                                 S1.ci, S1.cc, S1.cv, S1.st, seq, 4};
        // (the next iteration's stats stay on the device; this launch's verdict half hands the host the ones the launch
        // before left there for THIS iteration's acceptance test)
        c.e1 = revs::ChainKvSide{plan->fold_e1[par ^ 1], st->y_trial, d.vfull, d.viol, d.partial,
                                 S0n.ci, S0n.cc, S0n.cv, plan->fold_st_local[par ^ 1], 0.0, 4};
        if (plan->fold_st_local_valid) { c.fwd_src = plan->fold_st_local[par]; c.fwd_dst = S0.st; }
        plan->fold_st_local_valid = true;
        c.info = plan->fold_info[par ^ 1];     // (iteration k + 1's model)
        c.y_trial = st->y_spare;
        c.lin_out = S1n.st + 4;
        c.clr0 = plan->fold_e2[par ^ 1];
        c.clr1 = plan->fold_e1[par];
        c.prev_cidx = S0.ci;                  // the lists of the launch whose step wrote y_trial
        c.prev_ccnt = S0.cc;
        rc = revs::chain_kv_launch(c, stream);
        if (rc != REVS_OK) return rc;
        // The next iteration's sweep, unjudged: it needs this launch's shifts and cleared sum arrays (stream order) and
        // the state this iteration's sweep wrote; its own output goes to the third set.  (Not behind an iteration that
        // took extra Newton steps: the call returns behind that one.)
        const bool spec = can_spec && k + 1 < max_steps && redo == 0;
        if (spec) {
            rc = sweep(par ^ 1, st->p_est_new, st->p_sch_alt, st->gamma_alt, st->p_est_3, st->p_sch_3, st->gamma_3, nullptr, nullptr,
                       st->pdhg_dual_new, st->pdhg_dual_3);
            if (rc != REVS_OK) return rc;
        }
        // the trial's verdict: poll its tags (pinned memory), then the driver's own acceptance test
        if ((rc = wait_tags(S1.st_host, d.T, seq, s, "revs_plan_chain_fold_run", "the trial's verdict")) != REVS_OK) return rc;
        int32_t nsum = 0, nmax = 0;
        int why = 0;
        const int acc = chain_accept_impl(d.T, S0.st_host, S1.st_host, scale, d.eps, REVS_DUAL_AMAX, d.kadd, 1,
                                          &nsum, &nmax, &why);
#ifdef REVS_TUNING
        static const bool ftrace = getenv("REVS_FOLD_TRACE") != nullptr;
#else
        constexpr bool ftrace = false;
#endif
        if (ftrace && !acc) {
            double r0 = 0, r1 = 0, ncm = 0;
            int arm = 0;
            for (int t = 0; t < d.T; ++t) {
                const double *a = S0.st_host + 8 * t, *b = S1.st_host + 8 * t;
                r0 = std::max(r0, a[0] / scale);
                r1 = std::max(r1, b[0] / scale);
                ncm = std::max(ncm, a[2] + std::min(a[3], (double)d.kadd));
                if (a[0] / scale > d.eps && !(b[1] >= a[1] + 1e-4 * b[4] - 1e-11 * std::fabs(a[1]))) {
                    ++arm;
                    fprintf(stderr, "   slot %d: D0 %.17g D1 %.17g lin %.6g gain %.6g rows0 %.3g rows1 %.3g ns %g nv %g\n", t, a[1], b[1],
                            b[4], b[1] - a[1], a[0] / scale, b[0] / scale, a[2], a[3]);
                }
            }
            fprintf(stderr, "[fold] iteration %d (par %d, resumed %d) rejected: rows before %.3g after %.3g candidates %g armijo failures %d\n",
                    k, par, (int)have_k1, r0, r1, ncm, arm);
        }
        if (!acc) {
            // The speculative sweep of a rejected or redone iteration does not stand, and neither does what it
            // said about its own problems: "a PDHG residence stopped at its cap" is dropped from the sticky
            // status word, as revs_plan_stream_run_blocks does behind a roll-back (the sweep that replaces it
            // sets the bit again if it is true of the problem that counts; "no solution" does not depend on
            // the estimate: kept).  The carried PDHG multipliers ARE left where that sweep put them: another
            // warm start of the same problems.
            // (each sweep has its own word: this one's and the unjudged next one's are dropped -- the latter once it
            // has run; "no solution" does not depend on the estimate: kept)
            if (spec && hipStreamSynchronize(s) != hipSuccess) {
                revs::set_error("revs_plan_chain_fold_run: waiting for the unjudged sweep failed");
                return REVS_ELAUNCH;
            }
            if (fwords) {
                *(volatile unsigned int *)plan->flags_host |= (fwords[word_k] | (spec ? fwords[(word_k + 1u) % 3u] : 0u)) & 1u;
                fwords[word_k] = 0u;
                if (spec) fwords[(word_k + 1u) % 3u] = 0u;
            }
            // The caller's general loop takes this iteration (state untouched).  When the trial is a good
            // Newton step that merely left the rows above the tolerance -- the usual rejection with on/off
            // chargers -- the multipliers are handed back AT the trial (resume = 2): the caller goes on
            // from it instead of making the same step again.
            if (why == 1 && redo < kMaxRedo) {
                double *y_old = st->y;          // y := the step; the next trial goes where the speculative one went
                st->y = st->y_trial;
                st->y_trial = st->y_spare;
                st->y_spare = y_old;
                st->use_y = 1;
                st->sup0 = -1;
                ++redo;
                redo_pending = true;
                --k;
                continue;
            }
            st->redone = redo;
            if (why == 1) {
                std::swap(st->y, st->y_trial);
                st->use_y = 1;
                st->sup0 = -1;
                st->resume = 2;
                // (the pivots the step's model took: the caller's books count them with the solve it finishes)
                std::vector<int32_t> inf((size_t)d.T, 0);
                if (hipMemcpyAsync(inf.data(), plan->fold_info[par], sizeof(int32_t) * inf.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess) {
                    revs::set_error("revs_plan_chain_fold_run: reading the pivot counts failed");
                    return REVS_ELAUNCH;
                }
                st->pivots = 0;
                for (int32_t v : inf) st->pivots += v < 0 ? -v : v;
            }
            return REVS_OK;
        }
        if (fwords) {                         // this iteration's sweep stands: its status bits join the sticky word
            *(volatile unsigned int *)plan->flags_host |= fwords[word_k];
            fwords[word_k] = 0u;
        }
        double *y_old = st->y;
        st->y = st->y_trial;
        st->y_trial = st->y_spare;
        st->y_spare = y_old;
        st->use_y = nsum > 0;
        st->sup0 = -1;
        std::swap(st->p_sch, st->p_sch_alt);
        std::swap(st->gamma, st->gamma_alt);
        std::swap(st->p_est, st->p_est_new);
        if (ybuf) { std::swap(st->pdhg_dual, st->pdhg_dual_new); plan->d.pdhg_dual = st->pdhg_dual; }
        if (spec) {                           // (state k + 1 is current; the unjudged sweep read it and wrote the third set)
            std::swap(st->p_sch_alt, st->p_sch_3);
            std::swap(st->gamma_alt, st->gamma_3);
            std::swap(st->p_est_new, st->p_est_3);
            if (ybuf) std::swap(st->pdhg_dual_new, st->pdhg_dual_3);
            swept = true;
        }
        st->s_out = nullptr;                  // (schedules are written by the call's first iteration only)
        st->c_out = nullptr;
        ++*kept_steps;
        par ^= 1;
#ifdef REVS_TUNING
        static const bool no_pipe = getenv("REVS_FOLD_NO_PIPE") != nullptr;
#else
        constexpr bool no_pipe = false;
#endif
        have_k1 = !no_pipe;
        if (redo > 0) {                       // (the caller books this iteration's extra Newton steps: it is the call's last)
            st->redone = redo;
            break;
        }
    }
    plan->fold_ready = have_k1;
    plan->fold_par = par;
    st->resume = have_k1 ? 1 : 0;
#ifdef REVS_KV_STAMPS
    {
        std::vector<double> h(32 * (size_t)d.T);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(h.data(), plan->fold_sh[1] + mt, sizeof(double) * h.size(), hipMemcpyDeviceToHost);
        int worst = 0;
        for (int t = 0; t < d.T; ++t)
            if (h[32 * t + 20] - h[32 * t] > h[32 * worst + 20] - h[32 * worst]) worst = t;
        // 0 start | 1-6 rows | 7-10 selection | 11-16 model | 17 step | 18-20 shifts: microseconds since the slot's start
        fprintf(stderr, "[kv stamps, us since start] slowest slot %d:", worst);
        for (int i = 1; i <= 20; ++i) fprintf(stderr, " %d:%.1f", i, (h[32 * worst + i] - h[32 * worst]) * 0.01);
        fprintf(stderr, " | violated %g support %g room %g | fast body at %.1f, list read %.1f", h[32 * worst + 24], h[32 * worst + 25], h[32 * worst + 26],
                (h[32 * worst + 27] - h[32 * worst]) * 0.01, (h[32 * worst + 28] - h[32 * worst]) * 0.01);
        fprintf(stderr, " | prologue: round-1 loads issued %.1f, LDS cleared %.1f, list in %.1f, gathers issued %.1f, multipliers in %.1f, rows of R requested %.1f",
                (h[32 * worst + 21] - h[32 * worst]) * 0.01, (h[32 * worst + 22] - h[32 * worst]) * 0.01, (h[32 * worst + 23] - h[32 * worst]) * 0.01,
                (h[32 * worst + 29] - h[32 * worst]) * 0.01, (h[32 * worst + 30] - h[32 * worst]) * 0.01, (h[32 * worst + 31] - h[32 * worst]) * 0.01);
        fprintf(stderr, "\n[kv stamps, mean over slots]            ");
        for (int i = 1; i <= 20; ++i) {
            double acc = 0;
            for (int t = 0; t < d.T; ++t) acc += (h[32 * t + i] - h[32 * t]) * 0.01;
            fprintf(stderr, " %d:%.1f", i, acc / d.T);
        }
        fprintf(stderr, "\n");
    }
#endif
    return REVS_OK;
}
