/*
 * revs_admm_ops.h -- the operator QP's building blocks in librevs_admm.so (same library, same conventions
 * as revs_admm.h): the launches that revs_plan_newton_solve / revs_plan_chain_fold_run /
 * revs_plan_stream_run_blocks are made of.  NOT part of the drop-in boundary: a reference-side
 * binding needs revs_admm.h only.  They are exported because revs_admm_amd's Python driver issues them one by
 * one on its general paths (operator_admm.py: the ADMM forms of the operator QP; operator_newton.py: the chain
 * issued in phases, the Python Newton loop kept for comparison) and because the kernel-level parity tests
 * (tests/test_gpu_newton.py, test_gpu_operator.py) call each of them against its numpy restatement.  The reports'
 * launches close the file: revs_net_node_sums / revs_net_report (one schedule), revs_net_study (S schedules, pooled),
 * revs_net_node_sums_many (the node sums of an ensemble's S scenarios from its own layout into revs_net_study's input)
 * and revs_net_across (per node and per line, the statistics across the scenarios of a group), then the bill and the
 * convergence report, revs_rule_schedule: the schedules nobody optimised, for the reports to be pointed at,
 * revs_load_profile: the demand curve of any of them -- load per slot, peaks and diversity, by class of residence -- and
 * revs_charge_report: what the chargers do, per EV and per slot, revs_net_headroom: how much more charging
 * every node could take in every slot, and what limits it, revs_net_losses: what the feeder loses carrying a
 * schedule, per line, per node at the margin, per slot and per day, revs_xf_report: what a schedule does to the
 * service transformers -- load ratio, top-oil and hot-spot temperature per slot, loss of insulation life per day -- and
 * revs_flex_report: how much of the charging can still be moved, up and down, per EV, node and slot.  revs_net_powerflow
 * (beside the other tree reports) solves the nonlinear branch-flow equations that all of them linearise.
 */
#ifndef REVS_ADMM_OPS_H
#define REVS_ADMM_OPS_H

#include "revs_admm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- operator ("Utility") side -------------------------------------------
 * lpsolver.py:163-238:  min (kappa/2)|g - g0|^2  s.t.  g >= 0,
 *                        vlo <= R (A g) <= vhi   per slot,
 * g0 = (P_est + P_sch)/2 - G/kappa, A = home->node aggregation, R the LinDistFlow
 * sensitivity matrix of the constrained nodes (compute_Rmat, lpsolver.py:17-26).
 * Solved by ADMM in OSQP form with the KKT matrix applied through the
 * eigendecomposition D^1/2 R D^1/2 = Q L Q^T (D = diag(n_m); voltage row m is scaled by
 * sqrt(n_m), which keeps the operator matrix symmetric), so rho can be re-tuned per
 * slot without refactoring.  All operator arithmetic is double (the QP is ill conditioned:
 * cond(R)^2 ~ 5e7 on the 121144 feeder); the two (concatenated) products with Q per inner
 * iteration run on v_mfma_f64_16x16x4_f64.
 */

/* C[m][n] (+)= At^T * B on the matrix cores.  At is stored k-major (double
 * At[k][lda], element At[kk][i] = A[i][kk]); B is double[k][ldb]; C double[m][ldc].
 * n is small (T, up to 192).  accumulate != 0 adds into C.  f64 uses
 * v_mfma_f64_16x16x4_f64, f32 v_mfma_f32_16x16x4_f32 (exact f32 fma chain). */
int revs_gemm_tn_f64(int32_t m, int32_t n, int32_t k, const double *At, int32_t lda,
                     const double *B, int32_t ldb, double *C, int32_t ldc,
                     int32_t accumulate, void *stream);
int revs_gemm_tn_f32(int32_t m, int32_t n, int32_t k, const float *At, int32_t lda,
                     const float *B, int32_t ldb, float *C, int32_t ldc,
                     int32_t accumulate, void *stream);
/* C = At^T B with dense leading dimensions, K cut over `ksplit` groups of workgroups:
 * C holds ksplit partial slabs of m*n doubles (see _x2). */
int revs_gemm_tn_f64_split(int32_t m, int32_t n, int32_t k, const double *At, const double *B,
                           double *C, int32_t ksplit, void *stream);
/* [C0 | C1] = At^T [B0 | B1]: one product whose right-hand side and result are each the
 * horizontal concatenation of two double[k][T] / double[m][T] arrays (2T <= 192), so
 * the matrix is streamed once for both.  With the voltage rows scaled by sqrt(n_m) the
 * operator's matrix D^1/2 R D^1/2 = Q L Q^T is symmetric and one inner iteration is
 *   [ta | tb] = Q^T [rhat | w]   and   [va | usa] = Q [a | sa]
 * -- two launches instead of four products.  ksplit / slabs as for _x2. */
int revs_gemm_tn_f64_cat(int32_t m, int32_t T, int32_t k, const double *At, const double *B0,
                         const double *B1, double *C0, double *C1, int32_t ksplit,
                         void *stream);
/* Two independent products of the same shape in ONE launch (dense leading
 * dimensions lda = m, ldb = ldc = n, no accumulate): C0 = At0^T B0, C1 = At1^T B1.
 * ksplit (1..8) cuts K over ksplit groups of workgroups so a small m still fills the
 * chip; group s writes its PARTIAL product to slab s, i.e. C0 and C1 must each hold
 * ksplit slabs of m*n doubles and the product is the sum of the slabs (the
 * revs_op_node_* consumers add them, in slab order). */
int revs_gemm_tn_f64_x2(int32_t m, int32_t n, int32_t k, const double *At0, const double *B0,
                        double *C0, const double *At1, const double *B1, double *C1,
                        int32_t ksplit, void *stream);

/* Segmented home->node aggregation: out[node][t] = scale[node] * sum over the
 * homes of that node of in[home][t].  Homes are sorted by node; node_ptr is the
 * CSR offset array int64[m+1].  scale may be NULL (=1).  Deterministic. */
int revs_aggregate_f64(int32_t m, int32_t T, const int64_t *node_ptr,
                       const double *in_home, const double *scale, double *out_node,
                       void *stream);
int revs_aggregate_f32(int32_t m, int32_t T, const int64_t *node_ptr,
                       const float *in_home, float *out_node, void *stream);

/* Doubles of scratch revs_dual_bound (revs_admm.h) needs for n_homes residences (0: bad size). */
int64_t revs_dual_bound_scratch(int64_t n_homes, int32_t T);

/* revs_dual_bound for the S scenarios of an ensemble (revs_admm_amd/ensemble.py) in ONE launch plus a
 * finalize, on the ensemble's own layout: homes revs_home_t[n_res][S] (record res S + s), node_of int32[n_res] shared by
 * the scenarios, d / y / load_node double[m][S T] (scenario s: columns s T + t), scale DEVICE double[S] (one scale per
 * scenario; the host cannot see its sign: the caller keeps it >= 0), out device double[S][4].  out[s] = what
 * revs_dual_bound writes for scenario s alone -- {residences' part, LOAD part, row part, residences with empty rows}
 * of L_s(scale[s] y_s), d_s = R y_s, relaxed or integral -- BIT FOR BIT what that call gives on contiguous copies of the
 * scenario's records and columns with the same scale, and the same bits from call to call: grid (T + nhb) x S, column
 * s of the grid being the single call's workgroups over the same residences, their partials in scratch[s], summed per
 * scenario in the single call's order.  d and y: both or neither (NULL: no multipliers); load_node may be NULL;
 * n_res == 0: the slot-wise terms only (out[s][1] = sum c . load_node_s).  No p_node output.  Enqueues only.
 * REVS_EINVAL before any launch: T outside 1..REVS_MAX_T, S < 1, S T > REVS_ENS_MAX_COLS, n_res < 0, m <= 0, a null
 * cost / scale / scratch / out, null homes / node_of with n_res > 0, d without y or y without d, vlo > vhi, more than
 * 2^31 workgroups per scenario.  scratch: double[revs_dual_bound_many_scratch] = S revs_dual_bound_scratch(n_res, T)
 * (0: bad size). */
int64_t revs_dual_bound_many_scratch(int64_t n_res, int32_t S, int32_t T);
int revs_dual_bound_many(int64_t n_res, int32_t S, int32_t T, const float *cost, const revs_home_t *homes,
                         const int32_t *node_of, int32_t m, const double *d, const double *y, const double *load_node,
                         const double *scale, double vlo, double vhi, int32_t integral, double *scratch, double *out,
                         void *stream);

/* g0 = (P_est + P_sch)/2 - G/kappa : the unconstrained minimiser of the Utility
 * objective (lpsolver.py:196-207).  float in, double out. */
int revs_op_g0(int64_t n_homes, int32_t T, const float *p_est, const float *p_sch,
               const float *gamma, float kappa, double *g0, void *stream);

/* Operator ADMM state.  Per home and slot ONE double s_b = z_b + y_b is kept
 * (z_b = max(s_b,0) and y_b = min(s_b,0) are complementary); per node z_v, y_v.
 * Cold start: s_b = max(g0,0); z_v = clip(cx, vlo, vhi), y_v = 0, w = rho_v z_v
 * (cx = C_v x for that start, formed by the driver). */
int revs_op_init_home(int64_t n_homes, int32_t T, const double *g0, double *sb, void *stream);
int revs_op_init_node(int32_t m, int32_t T, const double *cx, const double *rho_v,
                      const double *bound_scale, double vlo, double vhi, double *zv, double *yv,
                      double *w, void *stream);

/* Home pass of one inner iteration (sb, g0 double[n][T]; rho_b double[T];
 * c = kappa + rho_b[t]; node m owns homes node_ptr[m]..node_ptr[m+1]-1):
 *   z = max(s_b,0), y = min(s_b,0)
 *   if xc != NULL (double[m][T], node correction from revs_op_node_update):
 *       xt  = (kappa g0 + rho_b z - y) / c + inv_sqrt_n[m] xc[m]      x-update
 *       u   = alpha xt + (1-alpha) z + y/rho_b
 *       z   = max(u,0), y = rho_b min(u,0), s_b = z + y
 *       if res != NULL (double[8][T], see revs_op_node_update; needs cty_node =
 *       V S U^T y_v, double[m][T]): rows 1,2,5,6,7 get the per-slot maxima of
 *       |xt - z|, |kappa (xt-g0) + C^T y|, |xt|, |C^T y|, |kappa g0|
 *   rhat[m] = inv_sqrt_n[m] * sum_homes (kappa g0 + rho_b z - y)
 * With homes sharded over GPUs rhat is this rank's partial sum: all-reduce it. */
int revs_op_home_pass(int32_t m, int32_t T, const int64_t *node_ptr,
                      const double *inv_sqrt_n, double *sb, const double *g0,
                      const double *xc, const double *rho_b, double kappa, double alpha,
                      double *rhat, const double *cty_node, double *res, void *stream);

/* revs_op_node_update (below) followed by revs_op_home_pass, in ONE launch: the workgroup
 * of node m first updates row m of (xc, z_v, y_v, w) from the products va, usa (nslab
 * slabs each) and the current rhat, then runs the home pass with that xc.  No residuals
 * in this form: the checking iteration of a block uses the two separate calls. */
int revs_op_home_pass_fused(int32_t m, int32_t T, const int64_t *node_ptr,
                            const double *inv_sqrt_n, double *sb, const double *g0,
                            const double *rho_b, double kappa, double alpha, double *rhat,
                            int32_t nslab, const double *va, const double *usa,
                            const double *rho_v, const double *bound_scale, double vlo,
                            double vhi, double *xc, double *zv, double *yv, double *w,
                            void *stream);

/* Node passes (double[m][T]; s double[m] singular values; rho_v, rho_b double[T]):
 *   revs_op_node_w:      w  = rho_v z_v - y_v
 *   revs_op_row_scale:   out = s (per row) * in
 *   revs_op_node_scale:  a  = (ta + s tb) / (c + rho_v s^2),  sa = s a
 *                        with ta = V^T rhat, tb = U^T w from revs_gemm_tn_f64_x2, each
 *                        given as nslab K-split slabs (double[nslab][m][T]) that are summed
 *   revs_op_node_update: (va, usa as nslab slabs, like ta/tb)
 *                        xc = va - rhat/c            (va = V a)
 *                        h  = alpha usa + (1-alpha) z_v   (usa = U sa = C_v xt)
 *                        z_v = clip(h + y_v/rho_v, b vlo, b vhi); y_v += rho_v (h - z_v)
 *                        (b = bound_scale[m], or 1 when NULL: row m of the voltage block
 *                        is stored scaled by sqrt(n_m), see below)
 *                        w = rho_v z_v - y_v
 *                        if res != NULL: rows 0,3,4 get max|usa - z_v|, |usa|, |z_v|
 * res is double[8][T], must be ZERO before the checking iteration (maxima are merged
 * with atomicMax) and feeds the driver's stopping test and per-slot rho update. */
int revs_op_node_w(int32_t m, int32_t T, const double *zv, const double *yv,
                   const double *rho_v, double *w, void *stream);
int revs_op_row_scale(int32_t m, int32_t T, const double *s, const double *in, double *out,
                      void *stream);
int revs_op_node_scale(int32_t m, int32_t T, int32_t nslab, const double *ta, const double *tb,
                       const double *s, const double *rho_v, const double *rho_b,
                       double kappa, double *a, double *sa, void *stream);
int revs_op_node_update(int32_t m, int32_t T, int32_t nslab, const double *va,
                        const double *rhat, const double *usa, const double *rho_v,
                        const double *rho_b, const double *bound_scale, double kappa,
                        double alpha, double vlo, double vhi,
                        double *xc, double *zv, double *yv, double *w, double *res,
                        void *stream);

/* ---- node-space fast path of the operator QP ------------------------------------
 * While no residence is pushed to g = 0 the problem collapses to the M constrained nodes:
 * g = g0 + A~^T d, cost (kappa/2)|d|^2, rows b vlo <= Rs (p0 + d) <= b vhi, p0 = A~ g0,
 * Rs = D^1/2 R D^1/2 = Q L Q^T.  ADMM on (x = p0 + d, z = Rs x) in the eigenbasis needs two
 * T-column products per iteration, no home-space traffic and no communication; per OUTER
 * iteration the ranks exchange only p0 (sum) and gmin (min).  The driver accepts the
 * answer iff slack = gmin + isn d >= 0 everywhere, else it runs the general path above.
 *
 *   revs_op_node_prep      p0[m] = isn[m] sum_i g0_i, gmin[m] = min_i g0_i (double[m][T]),
 *                          g0 = (P_est + P_sch)/2 - G/kappa from the float state;
 *                          g0_out (double[n][T]) or NULL.  preclamp != 0 uses max(g0, 0):
 *                          an exact presolve when R >= 0 entrywise and vlo <= 0 (only upper
 *                          rows can bind, so every node shift is <= 0 and a residence with
 *                          g0 < 0 sits at zero whatever the voltage rows do)
 *   revs_op_nodefast_feas   the operator's voltage check proper: v0 = Rs p0 (nslab slabs of
 *                           Q (l ph0)) against the bounds; cx = v0; stats (double[2], ZERO on
 *                           entry): [0] = largest row violation (0 <=> g0 already respects
 *                           every voltage row), [1] = max(0, -min gmin) (> 0 <=> some
 *                           residence has g0 < 0).  Both 0 <=> the answer is g0 itself.
 *                           stats is MERGED, not overwritten: each entry becomes the maximum of
 *                           what it held (>= 0) and of the call's value, like res
 *   revs_op_nodefast_scale  xh = (kappa ph0 + l wh)/(kappa + rho_v l^2), sx = l xh
 *                           (wh = Q^T w as nslab slabs, ph0 = Q^T p0)
 *   revs_op_nodefast_update z_v, y_v, w from zt = Q sx (nslab slabs); res rows 0,3,4
 *   revs_op_nodefast_dualres res rows 2,5,6,7 from yh = Q^T y_v (nslab slabs), in the
 *                           eigenbasis: max |kappa (xh - ph0) + l yh|, |xh|, |l yh|, kappa|ph0|
 *                           (row 5 without kappa, as in revs_op_home_pass: the driver scales
 *                           it); res is required and merged by maximum
 *   revs_op_nodefast_finish d = Q xh - p0 (x as nslab slabs), slack = gmin + isn d;
 *                           stats (double[2], ZERO on entry) = {max(0, -min slack), max|p0|},
 *                           merged by maximum like that of revs_op_nodefast_feas
 *   revs_op_node_apply      P_est_i = max(g0_i + isn[m] d[m], 0) as float (g0 as in prep)   */
int revs_op_node_prep(int32_t m, int32_t T, const int64_t *node_ptr, const double *inv_sqrt_n,
                      const float *p_est, const float *p_sch, const float *gamma, double kappa,
                      int32_t preclamp, double *p0, double *gmin, double *g0_out, void *stream);
int revs_op_nodefast_feas(int32_t m, int32_t T, int32_t nslab, const double *v0,
                          const double *bound_scale, const double *gmin, double vlo, double vhi,
                          double *cx, double *stats, void *stream);
int revs_op_nodefast_scale(int32_t m, int32_t T, int32_t nslab, const double *wh,
                           const double *ph0, const double *lam, const double *rho_v,
                           double kappa, double *xh, double *sx, void *stream);
int revs_op_nodefast_update(int32_t m, int32_t T, int32_t nslab, const double *zt,
                            const double *rho_v, const double *bound_scale, double alpha,
                            double vlo, double vhi, double *zv, double *yv, double *w,
                            double *res, void *stream);
int revs_op_nodefast_dualres(int32_t m, int32_t T, int32_t nslab, const double *xh,
                             const double *ph0, const double *lam, const double *yh,
                             double kappa, double *res, void *stream);
int revs_op_nodefast_finish(int32_t m, int32_t T, int32_t nslab, const double *x,
                            const double *p0, const double *gmin, const double *inv_sqrt_n,
                            double *d, double *slack, double *stats, void *stream);
int revs_op_node_apply(int32_t m, int32_t T, const int64_t *node_ptr, const double *inv_sqrt_n,
                       const float *p_est, const float *p_sch, const float *gamma, double kappa,
                       int32_t preclamp, const double *d, float *p_est_new, void *stream);

/* P_est = max(s_b, 0) as float: the operator's answer handed to the homes
 * (U_obj.g_opt, lpsolver.py:236-237, 259). */
int revs_op_export(int64_t n_homes, int32_t T, const double *sb, float *p_est, void *stream);

/* ---- dual Newton path of the operator QP (the default) --------------------------
 * Utility.solve (lpsolver.py:163-238) through its dual.  With y (double[m][T]) the
 * multipliers of the voltage rows, every residence of node m answers
 *     g_i = max(g0_i - d_m, 0),   d = R^T y / kappa,
 * so the dual function of slot t is
 *     D_t(y) = -(kappa/2) sum_i g_i^2 - sum_m max(vhi y_m, vlo y_m)   (+ a constant),
 * concave and C^1 with piecewise-linear gradient dD/dy_m = (R p)_m - b_m, p = A g,
 * b_m = vhi / vlo for an upper / lower row.  Each Newton iteration solves the
 * sign-constrained quadratic model on a candidate set of at most REVS_DUAL_AMAX (128) rows per
 * slot (rows with y != 0 plus the most violated ones) with generalised Hessian
 * K = R_F N R_F^T / kappa (N_m = residences of node m not clamped at zero) by block
 * principal pivoting, then takes an Armijo step on D_t.  The slots are independent
 * problems that share R and run side by side.  Per evaluation the ranks exchange pnq
 * (one all-reduce of 3 m T doubles); everything else is replicated and deterministic.
 *
 *   revs_op_dual_eval    d = (sum of the nslab slabs of R^T y)/kappa, or 0 when dsl is NULL;
 *                        g0 = (P_est + P_sch)/2 - G/kappa from the float state;
 *                        pnq[0] = p (node sums of g), pnq[1] = N (free residences),
 *                        pnq[2] = -(kappa/2) sum g^2 (double[3][m][T]); P_est_new = g (float)
 *                        when p_est_new != NULL
 *   revs_op_dual_select  v = sum of the nslab slabs of R p; per slot t: candidate rows
 *                        (cand_idx int64[T][AMAX], cand_cnt int32[T], -1 when more than AMAX
 *                        rows carry a multiplier), cand_val double[T][3][AMAX] = sign (+1
 *                        upper row, -1 lower row), gradient v - b, current y; every entry behind the
 *                        list (all AMAX of a slot flagged -1) is padding: index 0, sign 1, gradient 0,
 *                        y 0 -- here and in revs_op_dual_select_big; kadd beyond the room: what fits;
 *                        stats double[T][8]: [0] largest |v - b| over rows with y != 0 and
 *                        bound violation over the others, [1] D_t, [2] rows with y != 0,
 *                        [3] violated rows with y = 0 ([4] is left to revs_op_dual_step),
 *                        [5] = seq, written last behind a system-scope fence: when stats is
 *                        pinned host memory the host may poll it instead of an event.
 *                        vfull double[m][T] receives v; viol double[m][T] and partial
 *                        double[revs_op_dual_blocks(m)][T][4] are workspace.
 *   revs_op_dual_model   the model of every slot: K = R_F N R_F^T / kappa over its candidates
 *                        (R double[m][m] row-major, n_free = pnq[1]; accumulated as nks
 *                        column slabs k_slabs double[T][nks][AMAX][AMAX], summed in order
 *                        into k_full double[T][AMAX][AMAX]), then its maximiser over the sign
 *                        constraints by block principal pivoting in LDS: yhat double[T][AMAX];
 *                        info int32[T] = pivots (negative: limit hit)
 *   revs_op_dual_step    y_trial = y at the candidates moved by alpha[t] towards yhat (all
 *                        other entries of y_trial must already equal y);
 *                        lin_out[8 t] = gradient . (y_trial - y)                         */
/* Columns of one launch.  The slots are independent problems, so S scenarios of one feeder (same residences on the same
 * nodes, state float[n][S][T]) are ONE operator problem of S T columns (revs_admm_amd/ensemble.py): every
 * entry point of this section that takes T takes up to REVS_ENS_MAX_COLS of them -- the home pass and the row pass of the
 * dense form (revs_op_dual_eval, _eval_rows, revs_op_dual_rows / _select) walk tiles of 256 columns with a second grid
 * dimension beyond 256, the others are one workgroup per column.  Up to 256 columns every launch is what it was.  The
 * dense products keep their own limit (n <= 192 columns): beyond it revs_op_dual_evaluate needs the feeder as a tree
 * (revs_op_dual_evaluate_tree).  The kernels of the ADMM forms above and the folded chain stay at 256 columns; the ADMM
 * forms as a solver need the dense products, hence 192. */
#define REVS_ENS_MAX_COLS 1024
int revs_op_dual_eval(int32_t m, int32_t T, const int64_t *node_ptr, const float *p_est,
                      const float *p_sch, const float *gamma, int32_t nslab, const double *dsl,
                      double kappa, double *pnq, float *p_est_new, void *stream);
/* revs_op_dual_eval with d = R^T y / kappa taken from the few rows of R that carry a
 * multiplier instead of the slabs of a dense product: sup_idx int64[T][AMAX] / sup_cnt
 * int32[T] (all >= 0) list, per slot, rows that include every row with y != 0 -- e.g. the
 * candidate lists of the selection that produced or last judged this y. */
int revs_op_dual_eval_rows(int32_t m, int32_t T, const int64_t *node_ptr, const float *p_est,
                           const float *p_sch, const float *gamma, const double *R,
                           const int64_t *sup_idx, const int32_t *sup_cnt, const double *y,
                           double kappa, double *pnq, float *p_est_new, void *stream);
int32_t revs_op_dual_blocks(int32_t m);
int revs_op_dual_select(int32_t m, int32_t T, int32_t nslab, const double *vsl,
                        const double *pnq, const double *y, double vlo, double vhi,
                        int32_t kadd, double *vfull, double *viol, double *partial,
                        int64_t *cand_idx, int32_t *cand_cnt, double *cand_val, double *stats,
                        double seq, void *stream);
/* The first kernel of revs_op_dual_select alone (the selection left to
 * revs_agent_step_select); zero_out double[m][T] or NULL is cleared on the way. */
int revs_op_dual_rows(int32_t m, int32_t T, int32_t nslab, const double *vsl, const double *pnq,
                      const double *y, double vlo, double vhi, double *vfull, double *viol,
                      double *partial, double *zero_out, void *stream);
/* v_slabs = R p (Rt = R^T row-major, p double[m][T]) as `ksplit` K-split slabs AND the row
 * bookkeeping of revs_op_dual_rows in one launch: the last K-split workgroup of every
 * 32-row tile sums the tile's slabs and writes vfull, viol, partial (here
 * double[(m + 31) / 32][T][4]: pass that block count to revs_agent_step_select as
 * sel_nblk; the dual-value terms come from pnq[2]) and clears its rows of zero_out (NULL, or
 * a double[m][T] array other than p, which every workgroup reads to the end).  counters:
 * uint32[(m + 31) / 32], zero before the first use, left zero.  T <= 32. */
int revs_op_dual_product_rows(int32_t m, int32_t T, const double *Rt, const double *p,
                              const double *pnq, const double *y, double vlo, double vhi,
                              int32_t ksplit,
                              double *v_slabs, double *vfull, double *viol, double *partial,
                              double *zero_out, uint32_t *counters, void *stream);
int revs_op_dual_model(int32_t m, int32_t T, const double *R, const double *n_free,
                       const int64_t *cand_idx, const int32_t *cand_cnt, const double *cand_val,
                       double kappa, double delta, int32_t max_pivots, int32_t nks,
                       double *k_slabs, double *k_full, double *yhat, int32_t *info,
                       void *stream);
/* One evaluation as a single host call: phase bit 0 = [R^T y into d_slabs when use_y,]
 * revs_op_dual_eval; phase bit 1 = R p into v_slabs (Rt = R^T, row-major) and
 * revs_op_dual_select -- product and row bookkeeping as ONE launch when tile_counters
 * (uint32[(m + 31) / 32], zero before the first use, left zero) is given and T <= 32, see
 * revs_op_dual_product_rows (`partial` then holds (m + 31) / 32 blocks);
 * with phase bit 2 (value 4) the selection kernel is left to revs_agent_step_select.
 * A driver that shards residences runs phase 1, all-reduces pnq, then phase 2. */
int revs_op_dual_evaluate(int32_t phase, int32_t m, int32_t T, const int64_t *node_ptr,
                          const float *p_est, const float *p_sch, const float *gamma,
                          const double *R, const double *Rt, const double *y, int32_t use_y,
                          double kappa, double vlo, double vhi, int32_t kadd, int32_t ksplit,
                          double *d_slabs, double *v_slabs, double *pnq, float *p_est_new,
                          double *vfull, double *viol, double *partial, int64_t *cand_idx,
                          int32_t *cand_cnt, double *cand_val, double *stats, double seq,
                          uint32_t *tile_counters, void *stream);
/* revs_op_dual_model for slots with at most 8 candidates each (the caller knows the counts
 * from the stats: rows with y != 0 plus the violated rows admitted), Gram matrix and pivoting
 * in one small kernel.  A slot with more than 8 candidates is left unmoved and flagged
 * info = -999.  k_full as in revs_op_dual_model (top-left block written). */
int revs_op_dual_model_small(int32_t m, int32_t T, const double *R, const double *n_free,
                             const int64_t *cand_idx, const int32_t *cand_cnt,
                             const double *cand_val, double kappa, double delta,
                             int32_t max_pivots, double *k_full, double *yhat, int32_t *info,
                             void *stream);
int revs_op_dual_step(int32_t T, const int64_t *cand_idx, const int32_t *cand_cnt,
                      const double *cand_val, const double *yhat, const double *alpha,
                      double *y_trial, double *lin_out, void *stream);
/* revs_op_dual_step with alpha_t decided on the device from the stats of the evaluation the
 * model was built on: alpha_t = 1 if stats_prev[8 t] / scale > eps (rows of slot t not yet
 * within tolerance), else 0 -- what a driver that had read those stats would pass.  Lets a
 * driver enqueue evaluation, model, step and the next evaluation without reading anything in
 * between (operator_newton.py: the binding steady state).  y (double[m][T]) != NULL: y_trial = y is
 * copied by the same launch before the candidates are written (else the caller has done so). */
int revs_op_dual_step_pending(int32_t T, const int64_t *cand_idx, const int32_t *cand_cnt,
                              const double *cand_val, const double *yhat,
                              const double *stats_prev, double scale, double eps,
                              const double *y, int32_t m,
                              double *y_trial, double *lin_out, void *stream);
/* The selection of revs_op_dual_select (after revs_op_dual_rows / _product_rows; arguments as
 * revs_agent_step_select's), revs_op_dual_model_small on the lists it builds and
 * revs_op_dual_step_pending (y_trial = y, then the full step in the slots whose rows this
 * selection finds beyond eps; lin_out as there) in ONE launch, one workgroup per slot.  A
 * slot with more than 8 candidates gets info = -999 (and an unchanged y_trial column), as
 * from revs_op_dual_model_small: the caller then runs the general model. */
int revs_op_dual_select_model_step(int32_t m, int32_t T, const double *sel_partial, int32_t sel_nblk,
                                   const double *y, double vlo, double vhi, int32_t kadd,
                                   const double *vfull, const double *viol, int64_t *cand_idx,
                                   int32_t *cand_cnt, double *cand_val, double *stats, double seq,
                                   const double *R, const double *n_free, double kappa, double delta,
                                   int32_t max_pivots, double *k_full, double *yhat, int32_t *info,
                                   double scale, double eps, double *y_trial, double *lin_out,
                                   void *stream);
/* ---- the same evaluation behind the tree form of R p (see "the feeder as a tree" below) ----
 * On a radial feeder v = R p is three prefix sums over the nodes in DFS preorder: one workgroup per
 * slot computes its slot's voltages in O(nodes) and judges its rows on the spot -- no 33 MB matrix
 * stream, no K-split slabs, one block of partial sums per slot (the selection then runs with
 * sel_nblk = 1).  Same outputs as revs_op_dual_rows / revs_op_dual_select (rows of nodes without
 * residences have no position in the tree: their v, violation and multiplier stay zero).
 * revs_op_dual_rows_tree: pnq = the node sums p | N | q of the home pass; zero_out: an array (not
 * pnq) cleared on the way, or NULL; with_select != 0: the candidate selection of every slot in the
 * same launch (else the caller runs it: revs_agent_step_select with sel_nblk = 1) -- the slot's rows then reach
 * the selection through LDS where 3 m doubles fit beside the tree's scan buffer (m <= ~4 000), and vfull / viol
 * are scratch of the call: NOT written.
 * revs_op_dual_evaluate_tree: revs_op_dual_evaluate with phase bit 1 done this way (phase bit 0 --
 * the product R^T y for the home pass's shifts, when use_y -- is unchanged).
 * revs_op_dual_tree_select_model_step: rows, selection, small model and step of every slot in ONE
 * launch (revs_op_dual_select_model_step with the rows in front; n_free = pnq + m T). */
int revs_op_dual_rows_tree(int32_t m, int32_t T, const revs_tree_t *tree_host, const double *pnq,
                           const double *y, double vlo, double vhi, int32_t kadd, double *vfull,
                           double *viol, double *partial, double *zero_out, int64_t *cand_idx,
                           int32_t *cand_cnt, double *cand_val, double *stats, double seq,
                           int32_t with_select, void *stream);
int revs_op_dual_evaluate_tree(int32_t phase, int32_t m, int32_t T, const int64_t *node_ptr,
                               const float *p_est, const float *p_sch, const float *gamma,
                               const double *R, const revs_tree_t *tree_host, const double *y,
                               int32_t use_y, double kappa, double vlo, double vhi, int32_t kadd,
                               int32_t ksplit, double *d_slabs, double *pnq, float *p_est_new,
                               double *vfull, double *viol, double *partial, int64_t *cand_idx,
                               int32_t *cand_cnt, double *cand_val, double *stats, double seq,
                               void *stream);
int revs_op_dual_tree_select_model_step(int32_t m, int32_t T, const revs_tree_t *tree_host,
                                        const double *pnq, const double *y, double vlo, double vhi,
                                        int32_t kadd, double *vfull, double *viol, double *partial,
                                        int64_t *cand_idx, int32_t *cand_cnt, double *cand_val,
                                        double *stats, double seq, const double *R, double kappa,
                                        double delta, int32_t max_pivots, double *k_full, double *yhat,
                                        int32_t *info, double scale, double eps, double *y_trial,
                                        double *lin_out, void *stream);
/* Host only (no GPU work): the acceptance test of such a chained iteration on the two stats
 * blocks (double[T][8], as revs_op_dual_select writes them; s1[8 t + 4] = the step kernel's
 * linear term) -- returns 1 iff the driver's own checks (operator_newton.py:
 * AdmmEngine._operator_solve_newton) would find: evaluation 0 not yet within eps, at most 8
 * candidates per slot (the small model), the row-wise/dense choice `chain_few` right, the
 * Armijo test passed by the full step in every pending slot, and evaluation 1 within eps.
 * Then *nsup_sum / *nsup_max = total / largest number of multipliers per slot in s1.  Any
 * other outcome returns 0 and is left to the driver's general loop. */
int revs_newton_chain_accept(int32_t T, const double *s0, const double *s1, double scale, double eps,
                             int32_t amax, int32_t kadd, int32_t chain_few, int32_t *nsup_sum,
                             int32_t *nsup_max);

/* ---- the folded chain's operator launch on its own (csrc/newton_kernels.hip: op_chain_kv_kernel) -------------
 * What revs_plan_chain_fold_run issues between two sweeps, for the kernel tests to call in isolation
 * (tests/test_gpu_chain_kv.py).  One side = one evaluation judged by the tree form: its node sums pnq (es = 1: planar
 * double[3][m][T] = p | N | q, the evaluation kernel's; es = 4: double[T][m][4] = {p, N, q, 0} per slot and node,
 * slot-major, the folded sweep's), the multipliers y double[m][T], scratch for the rows (vfull, viol double[m][T],
 * partial double[T][4]: the two sides run in ONE launch and need separate scratch), the candidate lists and the stats
 * block its selection fills (as revs_op_dual_select's), tagged `seq`.
 *   e1: rows, selection, small model and step into y_trial (revs_op_dual_tree_select_model_step's outputs: k_full, yhat,
 *       info, y_trial; lin_out[8 t] the linear term), then the shifts of the trial: sh_a / sh_b [t * m + node] (slot-major)
 *       = (R^T y_trial)[node][t] / kappa, summed over the slot's list in list order (sh_a) and over the rows that carry a
 *       multiplier in ascending row order (sh_b: the order the next selection would list them in; equal to sh_a bit for
 *       bit where the two orders agree).  A slot with more than 8 candidates: info = -999, y_trial's column = y's.
 *   e2 (has_e2 != 0): rows and selection only, by the first T workgroups (the verdict of the trial before); e1's stats
 *       then get their tag by a plain store.  fwd_src / fwd_dst (both or neither; has_e2 only): double[T][8] blocks,
 *       entries 0..3 of every slot copied from src to dst in front of e2's tag.  clr0 / clr1: double[4 m T] arrays
 *       cleared by the verdict half (NULL: none; ignored without e2).
 *   prev_cidx / prev_ccnt (NULL: unknown -- every column of y is gathered): the candidate lists of the launch whose step
 *       produced e1.y (= e2.y).
 * What the kernel relies on and does NOT check:
 *   list padding       the previous lists are what a selection leaves, padding included (index 0 beyond the count, all
 *                      of a slot flagged -1): lanes 0..7 of a slot's wavefronts read prev_cidx[t][lane] and y at that
 *                      row whatever the count is.
 *   support on the list  every row of e1.y (and e2.y) with a multiplier is on its slot's previous list, when one is
 *                      given: the slot's multipliers are read through the list alone.
 *   sh_b               holds m T + 32 T doubles (a tuning build writes its stamps behind the shifts).
 *   untouched rows     rows without a position in the tree (y = 0 there) are not written in y_trial.
 * tree: the 256 x 8 shape (at most REVS_TREE_SWEEP_MAX nodes); m <= REVS_CHAIN_FOLD_MAX_M; T <= 256. */
typedef struct {
    const double *pnq, *y;
    double *vfull, *viol, *partial;
    int64_t *cand_idx;
    int32_t *cand_cnt;
    double *cand_val, *stats;
    double seq;
    int32_t es, reserved;
} revs_chain_kv_side_t;
typedef struct {
    int32_t m, T, kadd, has_e2;
    const revs_tree_t *tree;
    double vlo, vhi, kappa, delta, scale, eps;
    int32_t max_pivots, reserved;
    revs_chain_kv_side_t e1, e2;
    const double *R;
    double *k_full, *yhat;
    int32_t *info;
    double *y_trial, *lin_out;
    double *clr0, *clr1;
    double *sh_a, *sh_b;
    const int64_t *prev_cidx;
    const int32_t *prev_ccnt;
    const double *fwd_src;
    double *fwd_dst;
} revs_chain_kv_t;
int revs_op_chain_kv(const revs_chain_kv_t *c, void *stream);

/* ---- the model problem beyond REVS_DUAL_AMAX rows per slot (csrc/newton_big.hip) ------------------------------
 * The dual Newton path above holds REVS_DUAL_AMAX = 128 candidate rows per slot (its factor lives in LDS).  The reference
 * hands Gurobi every row (lpsolver.py:183-194); a slot with 129 ... REVS_DUAL_AMAX_BIG binding rows stays on the Newton
 * path through these three launches -- lists, Gram slabs, Hessian and factor in global memory (cand_idx
 * int64[T][BIG], cand_cnt int32[T] (-1: more rows with a multiplier than BIG), cand_val double[T][3][BIG] = sign |
 * gradient | current multiplier, k_slabs double[T][nks][BIG][BIG], k_full / l_factor double[T][BIG][BIG] each,
 * yhat double[T][BIG], info int32[T]: pivoting rounds, negative when the limit was hit, -998 for a slot flagged -1):
 *   revs_op_dual_select_big  the rows with y != 0 in row order + the `kadd` most violated rows without one (ties to the
 *                            lower row), from the multipliers and the row arrays vfull / viol ([m][T]) an evaluation by
 *                            the dense path (revs_op_dual_evaluate) left
 *   revs_op_dual_model_big   K_t = R_F N_t R_F^T / kappa and the LCP u >= 0, K'u - c >= 0, u.(K'u - c) = 0 by block
 *                            principal pivoting (same regularisation, tolerances and rule as revs_op_dual_model)
 *   revs_op_dual_step_big    y_trial = y, then y + alpha[t] (yhat - y) on slot t's listed rows; lin_out[8 t] = gradient . step */
#define REVS_DUAL_AMAX_BIG 512
int revs_op_dual_select_big(int32_t m, int32_t T, const double *y, const double *vfull, const double *viol, double vlo,
                            double vhi, int32_t kadd, int64_t *cand_idx, int32_t *cand_cnt, double *cand_val, void *stream);
int revs_op_dual_model_big(int32_t m, int32_t T, const double *R, const double *n_free, const int64_t *cand_idx,
                           const int32_t *cand_cnt, const double *cand_val, double kappa, double delta, int32_t max_pivots,
                           int32_t nks, double *k_slabs, double *k_full, double *l_factor, double *yhat, int32_t *info,
                           void *stream);
int revs_op_dual_step_big(int32_t T, const int64_t *cand_idx, const int32_t *cand_cnt, const double *cand_val,
                          const double *yhat, const double *alpha, const double *y, int32_t m, double *y_trial,
                          double *lin_out, void *stream);

/* ---- network report: line flows, line loading and node voltages of a home profile -------------------------------
 * What the reference draws for every result (drawing.py:29-78, compute_flows / compute_voltage), from the feeder as
 * a tree (revs_tree_t, revs_admm.h) instead of the inverse of the incidence matrix:
 *   flow[e][t]    = power through the line from tree node e to its parent = sum of g over the residences in e's subtree
 *   loading[e][t] = |flow| / rating[e]                      (NaN where the line has no rating)
 *   volt[n][t]    = sqrt(vset^2 - (R g)[n][t]) at EVERY tree node; NaN where the radicand is negative (the collapse of
 *                   LinDistFlow under an impossible load: numpy gives the reference the same NaN), never a trap
 * and per slot one revs_net_summary_t for loading (over the rated lines) and one for volt (over the masked nodes):
 * the numbers of the reference's box plots (matplotlib.cbook.boxplot_stats: quartiles by numpy.percentile's linear
 * interpolation, whiskers at the farthest datum within 1.5 IQR of the box, fliers beyond them) and the operator's
 * first questions.  Order statistics are exact.  NaNs are counted and left out of the statistics.
 *
 * revs_net_node_sums: node_g[m][t] = sum over the homes of node m (node_ptr: CSR offsets int64[m + 1], homes sorted by
 * node) of (double) load[h][t] + (double) p[h][t]; load may be NULL (p alone).  One accumulator per (node, slot), the
 * homes in ascending index: the same bits from call to call, and -- residences sharded with every node's homes on
 * one rank -- after the all-reduce (which then adds exact zeros) the same bits for any number of ranks.
 *
 * revs_net_report: one workgroup per slot, every tree shape up to REVS_TREE_MAX.  Device arrays by preorder position
 * (tree->n entries): rating (double; <= 0: unrated, left out of loading; NULL: no line is rated), node_mask (uint8, 0:
 * left out of the voltage summary; NULL: every node), node_of_pos (int32: the caller's index of the node at that
 * position, outside 0..n_out-1: a padding position, nothing is written for it; NULL: the position itself).  node_g
 * double[m][T].  Outputs, each may be NULL but not all: flow_out, loading_out, volt_out double[n_out][T] in the
 * caller's node order, summary_out revs_net_summary_t[2][T] ([0]: loading, [1]: volt).  Reads nothing else and writes
 * nothing else.  REVS_EINVAL: T outside 1..REVS_MAX_T, a null tree or node_g, a tree over REVS_TREE_MAX or not padded,
 * n_out outside 1..tree->n, vset not finite, vmin > vmax, every output NULL. */
typedef struct {
    double min, q1, median, q3, max;   /* of the `count` values summarised (NaN when count == 0) */
    double whisker_lo, whisker_hi;     /* the farthest values within 1.5 (q3 - q1) of the box */
    double worst_value;                /* loading: the largest; volt: the voltage of worst_index */
    int32_t count;                     /* values summarised: rated lines / masked nodes, NaNs left out */
    int32_t n_fliers;                  /* values beyond the whiskers */
    int32_t n_violations;              /* loading > 1; volt outside [vmin, vmax] */
    int32_t n_nan;                     /* rated lines / masked nodes whose value is a NaN */
    int32_t worst_index;               /* caller's index of the line of largest loading / of the node farthest outside
                                        * (or nearest to the edge of) [vmin, vmax]; the lowest on ties; -1: count == 0 */
    int32_t reserved[3];
} revs_net_summary_t;                  /* 96 bytes */
int revs_net_node_sums(int32_t m, int32_t T, const int64_t *node_ptr, const float *load, const float *p,
                       double *node_g, void *stream);
int revs_net_report(int32_t m, int32_t T, const revs_tree_t *tree_host, const double *node_g, const double *rating,
                    const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out, double vset, double vmin,
                    double vmax, double *flow_out, double *loading_out, double *volt_out,
                    revs_net_summary_t *summary_out, void *stream);

/* ---- study report: the network report of S schedules on one feeder, and box-plot numbers pooled over groups ---------
 * What the reference publishes is an ensemble (seeds x adoption x method): box plots pooled over all schedules of a
 * group, and per schedule and slot the number of nodes at or below a voltage band.  Quantiles do not compose, so the
 * pooled numbers are selected on the device from the keys of every schedule of the group.
 *
 * revs_net_study: revs_net_report's kernel on a T x S grid -- scenario s reads node_g[s] (double[S][m][T]) and writes
 * flow_out / loading_out / volt_out[s] (double[S][n_out][T]) and summary_out[s] (revs_net_summary_t[S][2][T]): bit for
 * bit what revs_net_report gives for that schedule alone.  tree, rating, node_mask, node_of_pos, n_out, vset, vmin,
 * vmax: as there, shared by every scenario.  In the same workgroup:
 *   band_count_out int32[S][T][B]: the number of masked nodes with volt <= band[b] (cumulative, any order of the
 *                  thresholds, a NaN voltage is never counted); band: HOST array of B <= 8 finite thresholds
 *   pooled_out     revs_net_pooled_t[G][2][T] ([0]: loading, [1]: volt): the summary rule over the multiset of all
 *                  values of the scenarios with group[s] == g.  group: HOST array int32[S] in -1 .. G-1 (-1: in no
 *                  pool).  A second launch on the same stream selects the order statistics exactly (digit-wise radix
 *                  select over the keys the first launch staged in `scratch`, revs_net_study_scratch bytes).  A pool of
 *                  one scenario equals that scenario's revs_net_summary_t in every shared field.  Worst ties: the
 *                  lowest scenario, then the lowest caller-side index.
 * Any output may be NULL, not all.  Reads nothing else; writes the outputs and the scratch.  REVS_EINVAL, before any
 * launch: every case of revs_net_report; S outside 1..REVS_STUDY_MAX_S; G outside 0..S; B outside 0..8; a group id
 * outside -1..G-1; a threshold that is not finite; band / group NULL where B / G > 0; pooled_out without scratch (or
 * with G == 0); every output NULL.
 * revs_net_study_scratch: 2 S T tree_n 8 bytes (keys [quantity][slot][scenario][position]); 0 for a bad size. */
#define REVS_STUDY_MAX_S 4096
#define REVS_STUDY_MAX_BANDS 8
typedef struct {
    double min, q1, median, q3, max;   /* as revs_net_summary_t, over the pool */
    double whisker_lo, whisker_hi;
    double worst_value;
    int32_t count;
    int32_t n_fliers;
    int32_t n_violations;
    int32_t n_nan;
    int32_t worst_index;               /* caller's index of the worst line / node, in scenario worst_scenario */
    int32_t worst_scenario;            /* -1: count == 0 */
    int32_t reserved[2];
} revs_net_pooled_t;                   /* 96 bytes */
int64_t revs_net_study_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_study(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const double *node_g,
                   const double *rating, const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out,
                   double vset, double vmin, double vmax, const int32_t *group, int32_t G, const double *band,
                   int32_t B, double *flow_out, double *loading_out, double *volt_out,
                   revs_net_summary_t *summary_out, revs_net_pooled_t *pooled_out, int32_t *band_count_out,
                   void *scratch, void *stream);

/* revs_net_node_sums_many: revs_net_node_sums for the S scenarios of an ensemble in one launch, on the ensemble's own
 * layout and straight into revs_net_study's input.  load (may be NULL) and p are float[n][S][T] -- element (i, s, t) at
 * (i S + s) T + t, a residence's S T floats contiguous -- node_ptr as there (shared by the scenarios), node_g
 * double[S][m][T]: node_g[s][node][t] = sum over the residences i of the node of (double) load[i][s][t] + (double)
 * p[i][s][t].  One thread per (node, column s T + t), one accumulator from +0.0, the residences in ascending index, the
 * widened pair added first: scenario s's slice carries the bits revs_net_node_sums gives on contiguous copies of
 * scenario s's rows, and the same bits from call to call; a node without residences gives 0.0.  Writes S m T doubles
 * from node_g on and nothing else: a caller that fills one study buffer from several ensembles passes
 * node_g + s0 m T.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S, T outside 1..REVS_MAX_T, m outside
 * 1..65535 (the report's limit), m S T >= 2^31, a null node_ptr, p or node_g. */
int revs_net_node_sums_many(int32_t S, int32_t m, int32_t T, const int64_t *node_ptr, const float *load, const float *p,
                            double *node_g, void *stream);

/* ---- study report, per node and per line: statistics of every cell ACROSS the scenarios of a group ------------------
 * The records above summarise over the feeder; these say WHERE: for every node (line) n and slot t, the box-plot numbers
 * of values[s][n][t] over the scenarios s of group g, how many of them violate [lo, hi] and how many reach each band.
 * Quantiles do not compose: they are selected exactly from all members' values of the cell (csrc/across_kernels.hip).
 *
 * values: device double[S][n_out][T], revs_net_study's volt_out (lo = vmin, hi = vmax, sense = -1) or loading_out
 * (lo = -inf, hi = 1, sense = +1); any double is allowed, -0.0 orders and is reported as +0.0.  group / G / band / B as
 * revs_net_study's (HOST arrays), keep: device uint8[n_out] or NULL (every cell).  One cell's record, over the members
 * of the group in ascending scenario index: a NaN counts in n_nan and is left out of everything else; min .. max are
 * numpy.percentile's (linear, rank (count - 1) e / 4, the roundings of the other summaries); mean is the sum from +0.0
 * in that order divided by count; worst_scenario has the largest max(lo - v, v - hi), the lowest scenario on ties;
 * band_count[b] members have v <= band[b] (sense < 0) or v >= band[b] (sense > 0), entries b >= B are 0.  With
 * count == 0 every double is a NaN, worst_scenario -1 and the other integers 0; a cell with keep[n] == 0 gets that
 * record with n_nan 0 too.  Every byte of every output is written.  An INFINITY among a cell's values follows
 * numpy.percentile as well: all five of min .. max are interpolated as a + (b - a) t, min and max with t = 0, so a
 * statistic whose neighbour (or itself) is infinite is a NaN although count > 0 -- a lone +inf gives five NaNs,
 * {1, +inf} gives min = max = NaN.  For finite values min and max are the smallest and the largest value themselves.
 *   slot_out      revs_net_across_t[G][n_out][T]: the record of values[s][n][t]
 *   daily_out     revs_net_across_t[G][n_out]: the record of the members' daily extremes d_s = min over t (sense < 0) /
 *                 max over t (sense > 0) of values[s][n][t], a NaN if any slot is one (numpy.min / numpy.max) -- written
 *                 once into `scratch` as double[S][n_out] and summarised by the same kernel as its T = 1 case
 *   exposure_out  int32[G][n_out]: the (member, slot) pairs with v < lo or v > hi: the sum over t of slot_out's
 *                 n_violations
 * Any output may be NULL, not all.  Reads values and keep, writes the outputs and the scratch.  REVS_EINVAL before any
 * launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; n_out outside 1..65535; S n_out T >= 2^31; G outside
 * 1..S; group NULL; a group id outside -1..G-1; B outside 0..8; band NULL with B > 0; a threshold that is not finite;
 * sense not -1 / +1; lo > hi or a NaN in either; values NULL; every output NULL; daily_out or exposure_out without a
 * 16-byte aligned scratch of revs_net_across_scratch bytes (8 S n_out; 0 for a bad size). */
#define REVS_ACROSS_MAX_BANDS 8
typedef struct {
    double min, q1, median, q3, max;  /* over the group's non-NaN values of the cell; numpy.percentile, linear
                                         (NaN beside an infinite value, as numpy's: see above) */
    double mean;                      /* sum in ascending scenario order from +0.0, divided by count */
    int32_t count, n_nan;             /* group members with a value / with a NaN */
    int32_t n_violations;             /* members with v < lo or v > hi */
    int32_t worst_scenario;           /* largest max(lo - v, v - hi); the lowest scenario on ties; -1: count == 0 */
    int32_t band_count[8];            /* members with v <= band[b] (sense < 0) or v >= band[b] (sense > 0); rest 0 */
} revs_net_across_t;                  /* 96 bytes */
int64_t revs_net_across_scratch(int32_t S, int32_t n_out);
int revs_net_across(int32_t S, int32_t n_out, int32_t T, const double *values, const uint8_t *keep, const int32_t *group,
                    int32_t G, double lo, double hi, int32_t sense, const double *band, int32_t B,
                    revs_net_across_t *slot_out, revs_net_across_t *daily_out, int32_t *exposure_out, void *scratch,
                    void *stream);

/* ---- bill report: what a schedule costs each residence, and its deviation from a baseline schedule ------------------
 * The reference's last result figure: per residence C = sum over t of P_res[t] COST[t] for two schedules and
 * dev = 100 (C2 - C1) / C1.  Here for S schedules at once, from the state on the device (csrc/bill_kernels.hip).
 *
 * revs_bill_rows: bill[s][i] = sum over t of tariff[t] * (double) g[s stride_s + i stride_i + t], ONE double accumulator
 * from +0.0, the slots ascending, product and sum rounded separately (no fused multiply-add): the bits of the numpy loop
 * acc = acc + c[t] * g[:, t], whatever S, the layout and the thread that holds the row.  g: device float (g_f64 = 0: an
 * ensemble's P_sch, float[n][S][T], stride_s = T, stride_i = S T) or double (g_f64 = 1: a study buffer double[S][n][T],
 * stride_s = n T, stride_i = T); strides in elements.  tariff: device double[T].  bill: device double[S][n], S n
 * doubles written from the pointer on and nothing else: a caller fills one buffer from several ensembles through
 * bill + s0 n.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; n < 1 or
 * S n >= 2^31; a null g, tariff or bill; g_f64 not 0 / 1; strides under which rows overlap -- accepted are exactly
 * stride_i >= T && stride_s >= n stride_i, or stride_s >= T && stride_i >= S stride_s. */
int revs_bill_rows(int32_t S, int64_t n, int32_t T, const void *g, int32_t g_f64, int64_t stride_s, int64_t stride_i,
                   const double *tariff, double *bill, void *stream);

/* revs_bill_study: deviations from a baseline row and box-plot records per scenario and pooled over groups.
 *   dev[s][i] = (100 (bill[s][i] - bill[b][i])) / bill[b][i], b = base[s] (HOST int32[S]; -1: a row of NaN), every
 *   operation rounded on its own in that order: numpy's 100*(C2-C1)/C1; a zero baseline bill gives what IEEE gives.
 *   dev_out: device double[S][n], or NULL (the deviations then live in `scratch` only).
 *   summary_out[s][q] (revs_bill_summary_t[S][2]; q = 0: bill, 1: dev): the record of scenario s's rows with
 *   keep[s][i] != 0 (device uint8[S][n]; NULL keeps every row); worst_scenario is s.
 *   pooled_out[g][q] ([G][2]): the same rule over the multiset of all kept values of the scenarios with group[s] == g
 *   (HOST int32[S] in -1..G-1, as revs_net_study's).  A pool of one scenario equals that scenario's record in every field.
 * A record: a kept value that is not finite counts in n_nan and is left out of everything else.  Quartiles are selected
 * exactly (digit-wise radix select over the values' ordered bit patterns, no sort) and interpolated as
 * numpy.percentile's, with the roundings of the other summaries; min and max are the smallest and the largest value;
 * whiskers and fliers as revs_net_summary_t's; -0.0 orders and is reported as +0.0.  worst_*: the largest value, ties to
 * the lowest scenario, then the lowest caller-side index index_of_row[i] (device int32[n]; NULL: i).  total: a sum in a
 * fixed tree order, the same bits from call to call.  With count == 0 every statistic is a NaN, both indices -1 and the
 * counts 0.  reserved0 is 0.
 * A fixed sequence of launches on one stream (deviations, then one selection workgroup per (member set, quantity)); no
 * grid-wide barrier.  Any output may be NULL, not all.  Reads bill, keep and index_of_row; writes the outputs and the
 * scratch.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; n < 1 or S n >= 2^31; bill NULL; base NULL
 * or an entry outside -1..S-1; G outside 0..S; group NULL with G > 0; a group id outside -1..G-1; pooled_out with
 * G == 0; summary_out or pooled_out without a 16-byte aligned scratch of revs_bill_study_scratch bytes (8 S n; 0 for a
 * bad size); every output NULL. */
typedef struct {
    double min, q1, median, q3, max;   /* numpy.percentile, linear, over the values summarised */
    double whisker_lo, whisker_hi;     /* farthest values within 1.5 (q3 - q1) of the box */
    double total;                      /* sum of the values summarised */
    double reserved0;
    int32_t count, n_nan;              /* kept values that are finite / that are not */
    int32_t n_fliers, n_above;         /* beyond the whiskers / > 0.0 */
    int32_t worst_index, worst_scenario; /* caller's index and scenario of the largest value; -1: count == 0 */
} revs_bill_summary_t;                 /* 96 bytes */
int64_t revs_bill_study_scratch(int32_t S, int64_t n);
int revs_bill_study(int32_t S, int64_t n, const double *bill, const int32_t *base, const uint8_t *keep,
                    const int32_t *index_of_row, const int32_t *group, int32_t G, double *dev_out,
                    revs_bill_summary_t *summary_out, revs_bill_summary_t *pooled_out, void *scratch, void *stream);

/* ---- convergence report: per-iteration and per-residence statistics of the residual history -------------------------
 * The reference's solve_ADMM returns diff[h][k], every residence's residual at every iteration, and plot_convergence
 * draws it.  Here from the history where the streaming launches leave it (csrc/convergence_kernels.hip), for one run or
 * the S scenarios of an ensemble.
 *
 * hist: device float, K rows with a row stride of ld elements; element (k, i, s) -- row k, residence i, scenario s -- at
 * k ld + i S + s: the ensemble's [n][S] sweep layout, with S = 1 the single engine's float[K][n].  keep: device
 * uint8[S][n], the residences of scenario s the records cover (NULL: all).  index: device int32[n], the caller-side
 * index reported for row i (NULL: i).  groups: HOST int32[S] in -1..G-1, as revs_bill_study's.
 *   iter_rec[s][k] (revs_bill_summary_t[S][K]): the record of the kept hist[k][i][s], widened to double (exact), under
 *   revs_bill_study's rules -- a kept value that is not finite counts in n_nan and is left out; quartiles selected
 *   exactly (digit-wise radix select over the floats' ordered bit patterns, four 8-bit digits, no sort) and interpolated
 *   as numpy.percentile's, no fused multiply-add; whiskers and fliers as revs_net_summary_t's; -0.0 orders and is
 *   reported as +0.0; with count == 0 every statistic a NaN, both indices -1, the counts 0 -- except that n_above counts
 *   the values > eps.  worst_index: the largest value, ties to the lowest caller-side index; worst_scenario = s.
 *   total: a sum in a fixed tree order, the same bits from call to call.
 *   pool_rec[g][k] ([G][K]): the same record over all kept values of the scenarios with groups[s] == g; the worst entry
 *   is the largest value, then the lowest scenario, then the lowest index; total is the members' totals added in scenario
 *   order.  A pool of one scenario repeats that scenario's record byte for byte.
 *   res_rec[s][i] (revs_conv_res_t[S][n], every residence, kept or not): a row is ABOVE when !(x <= eps), so a NaN is
 *   above.  n_above: the rows above; settle: 1 + the last row above (0: never above; K: the last row is above, not
 *   settled within the history); max: the largest value that is no NaN, -0.0 as +0.0 (NaN: none); worst_iteration: its
 *   first row (-1: none); last: hist[K-1]; reserved: 0.
 *   run_rec[s] (revs_conv_run_t[S]): with m[k] = iter_rec[s][k].max, converged_at is the first row k0 with m[k] <= eps
 *   for all of k0 .. k0 + patience - 1, all below K, else -1 (AdmmEngine.run's stopping rule; a row with an empty
 *   sample is not within eps); last_above the last row with !(m[k] <= eps), or -1; n_unsettled / n_never the kept
 *   residences with settle == K / settle == 0 -- both -1 when res_rec is NULL.
 *   settle_rec[s] (revs_bill_summary_t[S]): the record over (double) settle of the kept residences, n_above those with
 *   settle > 0, worst_index the caller-side index of the largest settle (ties: the lowest); exact in every field.
 * res_rec, run_rec and settle_rec may be NULL: that output is skipped, the others are the same bytes.  A fixed sequence
 * of launches on one stream (a selection workgroup per (row, block of 8 scenarios), one per (row, block of 4 groups), a
 * thread per column over the rows, a workgroup per scenario); no grid-wide barrier, no floating-point atomics.  Reads
 * hist, keep, index; writes the outputs and the scratch (revs_conv_report_scratch bytes, 16-byte aligned: integer
 * histograms of settle, 4 S (K + 1) + 8 S bytes rounded up; <= 0 for sizes the report refuses).
 * REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; n < 1; K < 1; S n >= 2^31; ld < n S; patience < 1; eps
 * negative or a NaN; a null hist, iter_rec or scratch; G outside 0..REVS_STUDY_MAX_S (a pool without members has
 * empty records); G > 0 without groups or without pool_rec; a group
 * id outside -1..G-1. */
typedef struct {
    float max, last;                   /* the largest residual that is no NaN; the last row's */
    int32_t settle, n_above;           /* 1 + the last row above eps; the rows above eps */
    int32_t worst_iteration, reserved; /* the first row that holds max, -1: none; 0 */
} revs_conv_res_t;                     /* 24 bytes */
typedef struct {
    int32_t converged_at, last_above;  /* first row of `patience` rows within eps, -1: none; last row above, -1: none */
    int32_t n_unsettled, n_never;      /* kept residences with settle == K / settle == 0; -1 without res_rec */
} revs_conv_run_t;                     /* 16 bytes */
int64_t revs_conv_report_scratch(int32_t S, int64_t n, int32_t K, int32_t G);
int revs_conv_report(int32_t S, int64_t n, int32_t K, const float *hist, int64_t ld, const uint8_t *keep,
                     const int32_t *index, const int32_t *groups, int32_t G, double eps, int32_t patience,
                     revs_bill_summary_t *iter_rec, revs_bill_summary_t *pool_rec, revs_conv_res_t *res_rec,
                     revs_conv_run_t *run_rec, revs_bill_summary_t *settle_rec, void *scratch, void *stream);

/* ---- rule schedules: what a charger does when nobody schedules it ----------------------------------------------------
 * The "before" of the reference's study (test-altered-profile.py:35-46: constant charger power from the arrival slot on,
 * laid over the base load), in closed form from the residence records (csrc/rule_kernels.hip).
 *
 * homes revs_home_t[rows]; load, p_out, g_out float[rows][T]; soc_out float[rows][T + 1]; status_out int32[rows]; all
 * contiguous.  A row is one (residence, scenario) record: an ensemble's float[n][S][T] is rows = n S as it stands.  Any
 * output may be NULL (not wanted: it then costs nothing), not all four; load may be NULL only if g_out is.
 *
 * Per row, the record's fields widened to double, every double operation rounded on its own:
 *   ws = clamp(start, 0, T), we = clamp(end, 0, T), W = max(we - ws, 0); window position j = t - ws.
 *   ev == 0: p = 0, soc = 0 (all T + 1 entries), g = load, status 0.
 *   Own rows empty (nmax < 0, or integral and nmin > nmax): p = 0, soc[t] = initial, status 1.
 *   integral != 0 (on/off charger): k = nmin (REVS_FILL_TARGET) or nmax (REVS_FILL_FULL) as the record holds them,
 *     on = min(k, W); ASAP: positions j < on at `rating`; ALAP: positions j >= W - on; status 1 iff on < nmin.
 *   integral == 0 (continuous charger): E_lo = (max(0.9, initial) - initial) capacity, E_hi = (1.0 - initial) capacity,
 *     E = E_lo / E_hi by the fill, D = min(E, rating W), status 1 iff D < E_lo.
 *     ASAP / ALAP: kf = min(floor(D / rating), W) (0 where rating <= 0), rem = D - kf rating (0 where kf == W, and
 *       where the rounded quotient reached an integer from below: never a negative power);
 *       ASAP: j < kf at `rating`, j == kf at (float) rem; ALAP: j >= W - kf at `rating`, j == W - kf - 1 at (float) rem.
 *     EVEN: (float)(D / W) at every window position (W > 0).
 *   soc[0] = initial, soc[t] = (float)(initial + E_before(t) / capacity), E_before(t) the energy of the slots before t
 *     in closed form -- (full slots before t) rating, plus rem once the partial slot lies before t; EVEN: (window slots
 *     before t) (D / W) -- no scan.  g[t] = load[t] + p[t], one float addition.
 * Status bit 1 carries the sweep's "no solution" meaning: the EV leaves below the state of charge the model demands.
 * Enqueues only (capturable); the same bits from call to call.  REVS_EINVAL before any launch: rows < 1 (or rows T
 * beyond one launch's grid), T outside 1..REVS_MAX_T, null homes, an unknown policy or fill, REVS_RULE_EVEN with
 * integral != 0, every output NULL, g_out without load. */
#define REVS_RULE_ASAP  0   /* charge from the first window slot on: uncontrolled */
#define REVS_RULE_ALAP  1   /* finish in the last window slot: last-minute         */
#define REVS_RULE_EVEN  2   /* the same power in every window slot: trickle (continuous chargers only) */
#define REVS_FILL_TARGET 0  /* deliver what the model demands: s_T >= 0.9 (nmin slots / E_lo) */
#define REVS_FILL_FULL   1  /* charge to 100 %                         (nmax slots / E_hi) */
int revs_rule_schedule(int64_t rows, int32_t T, const revs_home_t *homes, const float *load, int32_t policy, int32_t fill,
                       int32_t integral, float *p_out, float *soc_out, float *g_out, int32_t *status_out, void *stream);

/* ---- load-profile report: demand per slot, peaks and diversity of a schedule, by class of residence ----------------
 * The reference's demand curve (test-altered-profile.py:25-57: the residences' load per slot, with and without EVs),
 * from a schedule where it lies on the device (csrc/load_profile_kernels.hip).
 *
 * g: device float; element (residence i, scenario s, slot t) at i stride_i + s stride_s + t, strides in elements,
 * accepted under exactly revs_bill_rows' rule (an ensemble's float[n][S][T]: stride_s = T, stride_i = S T; one engine:
 * S = 1).  cls: device uint8[S][n]; cls[s][i] < C is the class of residence i in scenario s, any other value leaves it
 * out of every set.  Q = C + 1 sets: set q < C is class q, set C every residence with a class.  cls = NULL needs C = 0:
 * every residence is in the one set.  index_of_row: device int32[n] in 0..2^31 - 2, the caller-side index of row i
 * (NULL: i).  groups: HOST int32[S] in -1..G-1, as revs_bill_study's.
 *   slot_rec[s][q][t] (revs_bill_summary_t[S][Q][T]): the record over the set's values at slot t, widened to double, by
 *   revs_conv_report's iter_rec rules -- a value that is not finite counts in n_nan and is left out; quartiles selected
 *   exactly (radix select over the floats' ordered keys) and interpolated as numpy.percentile's, no fused multiply-add;
 *   whiskers and fliers as revs_net_summary_t's; -0.0 orders and is reported as +0.0; n_above counts the values > above
 *   (any double but a NaN); worst_index: the largest value, ties to the lowest caller-side index; worst_scenario = s;
 *   total: a sum in a fixed order, the same bits from call to call; an empty set: NaN statistics, indices -1, counts 0;
 *   reserved0 is 0.
 *   peak_rec[s][q] ([S][Q]): the same record over x_i = max over t of g[i][s][t], each residence's own daily peak; a
 *   row that holds a value that is not finite gives a NaN and counts in n_nan.
 *   day_rec[s][q] (revs_profile_day_t[S][Q]): from A[t] = slot_rec[s][q][t].total over the slots with count > 0, by the
 *   formulas beside the fields; a function of the records the same call computes, whether they are asked for or not.
 *   Where no slot holds a value the doubles are NaN, the slot indices -1 and slots 0.
 *   pool_slot_rec[gid][q][t] / pool_peak_rec[gid][q] ([G][Q][T] / [G][Q]): the same rules over the multiset of all member
 *   scenarios' values; total: the members' totals added in scenario order; the worst entry: the largest value, then the
 *   lowest scenario, then the lowest index.  A pool of one scenario repeats that scenario's record byte for byte.
 * Any output may be NULL, not all; the others are the same bytes.  Reads g, cls, index_of_row; writes the outputs and the
 * scratch.  A fixed sequence of launches on one stream, the residences split over workgroups (integer histograms merged
 * through integer atomics, partial sums folded in a fixed order); no grid-wide barrier, no floating-point atomics; the
 * call only enqueues.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; n < 1 or
 * S n >= 2^31; C outside 0..REVS_PROFILE_MAX_CLASSES; cls and C disagreeing about NULL / 0; strides revs_bill_rows would
 * refuse; above a NaN; a null g; G outside 0..S; groups NULL with G > 0; a group id outside -1..G-1; a pool output with
 * G == 0; a null or misaligned (16 bytes) scratch; every output NULL.  scratch: revs_load_profile_scratch bytes (<= 0
 * for sizes the report refuses).  revs_load_profile_chunk: the residences one workgroup of a walk owns. */
#define REVS_PROFILE_MAX_CLASSES 4
typedef struct {
    double peak, valley;              /* largest / smallest slot total of the set's aggregate profile */
    double energy;                    /* sum over t of those totals, t ascending from +0.0 (kW x slots) */
    double load_factor;               /* (energy / slots) / peak, each operation rounded on its own */
    double sum_peaks;                 /* peak_rec's total: the residences' own daily peaks added up */
    double diversity;                 /* sum_peaks / peak */
    int32_t peak_slot, valley_slot;   /* earliest slot on ties; -1: no slot holds a value */
    int32_t slots, reserved;          /* slots with count > 0; 0 */
} revs_profile_day_t;                 /* 64 bytes */
int32_t revs_load_profile_chunk(void);
int64_t revs_load_profile_scratch(int32_t S, int64_t n, int32_t T, int32_t C, int32_t G);
int revs_load_profile(int32_t S, int64_t n, int32_t T, const float *g, int64_t stride_s, int64_t stride_i,
                      const uint8_t *cls, int32_t C, const int32_t *index_of_row,
                      const int32_t *groups, int32_t G, double above,
                      revs_bill_summary_t *slot_rec, revs_bill_summary_t *peak_rec, revs_profile_day_t *day_rec,
                      revs_bill_summary_t *pool_slot_rec, revs_bill_summary_t *pool_peak_rec,
                      void *scratch, void *stream);

/* ---- charging report: what the chargers do, per EV and per slot ---------------------------------------------------
 * The second of the three arrays every solver entry of the reference returns (ev_schedule; AdmmEngine.S, an ensemble's
 * float[n][S][T], the p of revs_rule_schedule), read where it lies (csrc/charge_kernels.hip).
 *
 * p: device float; element (residence i, scenario s, slot t) at i stride_i + s stride_s + t, strides in elements,
 * accepted under exactly revs_bill_rows' rule.  homes: device revs_home_t[n][S], the record of (i, s) at i S + s.
 * tariff: device double[T], or NULL: every cost is then a NaN.
 *
 * Per row, the record's fields widened to double, every operation rounded on its own, no fused multiply-add:
 *   ws = clamp(start, 0, T), we = clamp(end, 0, T) (revs_rule_schedule's window).
 *   slot t is ON iff (double) p[t] > on_frac * (double) rating (a NaN is off); FULL iff on and p[t] >= rating.
 *   energy = sum over all T slots of (double) p[t], one accumulator from +0.0, t ascending; cost = sum of
 *   tariff[t] * (double) p[t] in the same way (revs_bill_rows' rule); soc_end = (float)(initial + energy / capacity).
 *   n_on, n_full: the counts; first_on, last_on: slot indices, -1 when never on; sessions: the on slots whose
 *   predecessor is off (or t == 0); wait = first_on - ws (it may be negative), -1 when never on; n_outside: the on slots
 *   with t < ws or t >= we.  flags: bit 0 ev != 0; bit 1 under target, max(0.9, initial) - (initial + energy / capacity)
 *   > short_tol; bit 2 some p[t] is not finite (the doubles are then what IEEE gives).
 *   row_rec is [S][n].  A row with ev == 0 gets zeros, -1 in first_on, last_on and wait, flags 0, whatever p holds (its
 *   p is not read).
 * slot_rec[s][t] ([S][T]) counts over the rows with ev != 0: n_ev (the same in every slot), n_plugged (ws <= t < we),
 *   n_on, n_full, n_starts (sessions that begin at t); power: the sum of (double) p[t] in a fixed order, the same bits
 *   from call to call.
 * day_rec[s] ([S]), a function of the records above whether or not they are asked for: peak_power / peak_power_slot
 *   and peak_on / peak_on_slot by a scan from slot 0 that moves on `>` only (the earliest slot wins ties; a NaN power
 *   never wins, one at slot 0 stays); both slots -1 without an EV; energy: the slots' power added, t ascending from
 *   +0.0; coincidence = peak_on / n_ev (NaN without an EV); cost: the EV rows' costs added in a fixed order; n_under /
 *   n_never / n_interrupted / n_outside: the EV rows with flags bit 1 / n_on == 0 / sessions > 1 / n_outside > 0.
 * hist: int32[S][3][T + 1] over the EV rows: [0] of n_on, [1] of wait (rows never on or with a negative wait are not
 *   counted), [2] of sessions.
 * val_out: double[4][S][n]: energy, cost, (double) soc_end, (double) wait; a NaN where the row is no EV, where flags
 *   bit 2 is set, and for wait where the charger is never on.  keep_out: uint8[S][n], 1 for EV rows without bit 2.  The
 *   two are what revs_bill_study (base = -1) takes: the box-plot records come from that selection.
 * Any output may be NULL, not all; the others are the same bytes.  Reads p, homes, tariff; writes the outputs and the
 * scratch.  A thread owns a row and walks its slots in chunks of revs_charge_report_chunk() staged through LDS; the
 * scenario is grid.y.  Slot counts: wavefront ballots, LDS counters, one global integer atomic per (workgroup, slot,
 * counter); power and cost: per-workgroup partials in the scratch, folded in a fixed order by a second kernel (32 runs
 * of consecutive workgroups, then the runs in order); a third derives the day records.  No floating-point atomics, no grid-wide barrier, a fixed sequence of launches on one
 * stream; the call only enqueues.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; T outside
 * 1..REVS_MAX_T; n < 1 or S n >= 2^31; strides revs_bill_rows would refuse; a null p or homes; on_frac or short_tol
 * negative or a NaN; a null or misaligned (16 bytes) scratch; every output NULL.  scratch: revs_charge_report_scratch
 * bytes (<= 0 for sizes the report refuses). */
typedef struct {
    double energy, cost;
    float soc_end, reserved0;
    int32_t n_on, n_full, first_on, last_on, sessions, wait, n_outside, flags;
    int32_t reserved[2];
} revs_charge_row_t;                  /* 64 bytes */
typedef struct {
    int32_t n_ev, n_plugged, n_on, n_full, n_starts, reserved;
    double power;
} revs_charge_slot_t;                 /* 32 bytes */
typedef struct {
    double peak_power, energy, coincidence, cost;
    int32_t peak_on, peak_on_slot, peak_power_slot, n_ev, n_under, n_never, n_interrupted, n_outside;
} revs_charge_day_t;                  /* 64 bytes */
int32_t revs_charge_report_chunk(void);
int64_t revs_charge_report_scratch(int32_t S, int64_t n, int32_t T);
int revs_charge_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                       const revs_home_t *homes, const double *tariff, double on_frac, double short_tol,
                       revs_charge_row_t *row_rec, revs_charge_slot_t *slot_rec, revs_charge_day_t *day_rec,
                       int32_t *hist, double *val_out, uint8_t *keep_out, void *scratch, void *stream);

/* ---- headroom report: spare charger power per node and slot (csrc/headroom_kernels.hip) -------------
 * How much more constant power x node i could draw in slot t before something it affects reaches its limit: the nodal
 * hosting capacity, in closed form on the tree.  Positions j = 0 .. tree->n - 1 are feeder_tree's preorder positions.
 * Host-prepared per position (feeder.headroom_aux), DEVICE arrays in a HOST struct:
 *   parent_pos int32[n]  position of j's parent, -1 when j hangs off the substation
 *   wc double[n]         wc[j] = (parent_pos[j] >= 0 ? wc[parent_pos[j]] : 0.0) + w[j], one forward loop in preorder:
 *                        wc[lca(i, j)] = R[i][j]
 *   jump uint16[n_jump][n]  jump[r][j] = position of j's 2^(r + 1)-th ancestor, 0xFFFF: none; n_jump = the smallest count
 *                        with 2^(n_jump + 1) > the forest's depth (roots at depth 0; 0 and a NULL jump for depth <= 1): the
 *                        two passes below take n_jump + 1 rounds instead of one per level
 * Per (scenario s, slot t), with drop and flow what revs_net_report's scans give at every position (the same bits):
 *   slack of a limit node (limit_mask[j] != 0; NULL: every position with a row)   s[j] = drop_max - drop[j]
 *   A[a] = min of s[j] over the limit nodes in a's subtree (+inf: none);  B[a] = rating[a] - flow[a] where rating[a] > 0
 *   headroom x[i] = max(0, min over the ancestors-or-self a of i of { A[a] / wc[a] where wc[a] > 0, B[a] where rated }),
 *                   +inf when no term exists; IEEE double operations, minima exact
 *   limiter: the shallowest a that attains the minimum (before the clamp), its voltage term before its thermal one:
 *            limiter_out = node_of_pos[a] | kind << 30, kind 0 voltage ("the subtree below a holds the node that reaches
 *            the limit first") / 1 thermal ("the line above a"); -1: unlimited (or a limiter without a caller-side index)
 * A slot whose node_g holds a non-finite value at a row of the tree: every headroom a NaN, every limiter -1, the summary
 * count 0 and n_nan = the nodes summarised; drop_out / flow_out are what the scans give.  (Finite injections whose drops
 * overflow are outside the contract.)
 *   headroom_out double[S][n_out][T], limiter_out int32[S][n_out][T], drop_out / flow_out double[S][n_out][T]
 *   summary_out revs_net_summary_t[S][T] over the positions with out_mask != 0 (NULL: all) and a caller-side index: the
 *                box-plot record of the finite headrooms (a second launch, box_select64); +inf values are left out and
 *                counted in reserved[0], NaNs in n_nan; n_violations = values < need; worst_value = the smallest headroom,
 *                worst_index = the lowest caller-side index that attains it
 *   day_out     revs_headroom_day_t[S][n_out]: over the slots that are no NaN, the smallest headroom, its earliest slot
 *                and the number of slots with x < need; all NaN: min NaN, slot -1
 * rating, node_of_pos, n_out: as revs_net_report's.  Any output may be NULL, not all.  Enqueues only (up to three
 * launches on `stream`): capturable, no allocation, no synchronisation.  REVS_EINVAL before any launch: S outside
 * 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; m outside 1..65535; a null node_g; a tree over REVS_TREE_MAX, not padded or
 * NULL; n_out outside 1..tree->n; a null aux, parent_pos or wc; n_jump outside 0..REVS_HEADROOM_MAX_JUMP, a NULL jump with
 * n_jump > 0; drop_max or need not finite, need < 0; every output NULL; summary_out or day_out without a 16-byte aligned
 * scratch of revs_net_headroom_scratch bytes (8 S T tree_n: the headrooms by position; 0 for a bad size). */
#define REVS_HEADROOM_MAX_JUMP 13
typedef struct {
    const int32_t *parent_pos;
    const double *wc;
    const uint16_t *jump;
    int32_t n_jump;
} revs_headroom_aux_t;
typedef struct {
    double min;                       /* the day's smallest headroom (NaN: every slot is one) */
    int32_t slot;                     /* its earliest slot; -1 */
    int32_t n_short;                  /* slots with x < need */
} revs_headroom_day_t;                /* 16 bytes */
int64_t revs_net_headroom_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_headroom(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const revs_headroom_aux_t *aux_host,
                      const double *node_g, const double *rating, const uint8_t *limit_mask, const uint8_t *out_mask,
                      const int32_t *node_of_pos, int32_t n_out, double drop_max, double need, double *headroom_out,
                      int32_t *limiter_out, double *drop_out, double *flow_out, revs_net_summary_t *summary_out,
                      revs_headroom_day_t *day_out, void *scratch, void *stream);

/* ---- loss report: line losses, marginal loss per node, energy and cost (csrc/losses_kernels.hip) ------
 * What the feeder loses carrying a schedule: a closed form on top of the network report's scans.  Positions j = 0 ..
 * tree->n - 1 are feeder_tree's preorder positions.  Per (scenario s, slot t), every operation an IEEE double operation
 * rounded on its own (no fused multiply-add), with flow[j] and drop[j] what revs_net_report's scans give at every position
 * (the same bits), inj[j] the gathered node sum (+0.0 at a position without a row), w[j] = tree->w[j] = 2 r[j], and
 * vset2 = vset vset formed by the caller:
 *   den[j]  = vset2 - drop[j]
 *   loss[j] = ((0.5 w[j]) flow[j]) flow[j] / den[j]    power lost on the line above j (the receiving-end form of the
 *                                                      branch-flow loss r P^2 / v); a zero-resistance line loses 0
 *   c[j]    = (w[j] flow[j]) / den[j]
 *   mlf[i]  = sum of c[a] over the ancestors-or-self a of i: the extra loss per extra unit drawn at i with den held fixed
 *             (dimensionless), computed in the drop scan's form -- the prefix of c in preorder minus the prefix of c in
 *             end-order below cle -- so its bits depend on the launch shape; it is within 2 n 2^-53 sum |c| of any order
 * Bad slot: a row's injection is not finite, or den[j] > 0 fails at a position with a caller-side index (the collapse
 * that revs_net_report shows as a NaN voltage).  Then every loss, every mlf and every double of the slot record is a NaN
 * (all four class_total included), mlf_max_index -1, n_bad 1, the summary has count 0 and n_nan = the lines summarised;
 * drop_out / flow_out are what the scans give.  One flag for the workgroup; nothing traps.
 * Sums over positions (total, delivered, class_total[k]): each is the root of ONE fixed binary tree -- the values laid out
 * by position, +0.0 where the position is padding, masked out or not of class k, the array padded with +0.0 to the next
 * power of two, then level by level x[i] = x[2i] + x[2i + 1] -- so the bits depend neither on the launch shape nor on
 * the order of the scans.
 *   total          sum of loss over the lines with line_mask[j] != 0 (NULL: all) and a caller-side index
 *   delivered      sum of inj
 *   class_total[k] sum of loss over the positions with line_class[j] == k (uint8 per position), k < C <= 4; NULL: C = 0
 * Outputs, any may be NULL, not all:
 *   loss_out, mlf_out, drop_out, flow_out   double[S][n_out][T] in the caller's node order (node_of_pos, n_out as
 *                  revs_net_report's)
 *   summary_out    revs_net_summary_t[S][T]: the box-plot record of the losses of the lines with line_mask and a
 *                  caller-side index (a second launch, box_select64 and the rules of boxplot.h); NaNs are left out and
 *                  counted in n_nan; worst_value = the largest loss, worst_index = the lowest caller-side index that
 *                  attains it; n_violations = lines with loss > loss_max (kW; +inf allowed)
 *   slot_out       revs_loss_slot_t[S][T]: total, delivered, class_total (entries k >= C are 0), mlf_max = the largest
 *                  mlf over the positions with node_mask[j] != 0 (NULL: all) and a caller-side index, mlf_max_index the
 *                  lowest index that attains it (-1 and a NaN mlf_max when there is none), n_bad
 *   line_day_out   revs_loss_line_day_t[S][n_out]: energy = the line's losses summed from +0.0 in ascending slot order,
 *                  then multiplied once by slot_hours; peak / peak_slot = the largest loss and its earliest slot; a bad
 *                  slot makes energy and peak NaN and peak_slot -1
 *   day_out        revs_loss_day_t[S]: energy, delivered, class_energy[4] by the same rule over the slot totals; cost =
 *                  the sum from +0.0 in slot order of the rounded products total[t] cost[t], multiplied once by
 *                  slot_hours (cost: DEVICE double[T]; NULL: a NaN); peak / peak_slot = the largest slot total and its
 *                  earliest slot (NaN / -1 with a bad slot); n_bad_slots; top_index[8] / top_energy[8] = the eight
 *                  summarised lines (line_mask, caller-side index) of largest day energy in descending order, NaNs left
 *                  out, ties to the lowest caller index, unused entries -1 / NaN
 * Enqueues only (up to four launches on `stream`): capturable, no allocation, no synchronisation.  REVS_EINVAL before any
 * launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; m outside 1..65535; a null node_g; a tree over
 * REVS_TREE_MAX, not padded or NULL; n_out outside 1..tree->n; vset2 or slot_hours not finite and > 0; loss_max not > 0
 * (+inf allowed, a NaN refused); C outside 0..4; line_class NULL with C > 0; every output NULL; summary_out, line_day_out
 * or day_out without a 16-byte aligned scratch of revs_net_losses_scratch bytes (8 S T tree_n: the losses by position,
 * + 64 S T: the slot records, + 8 S tree_n: the lines' day energies; 0 for a bad size). */
typedef struct {
    double total;                     /* kW lost on the summarised lines */
    double delivered;                 /* sum of the injections */
    double class_total[4];            /* kW lost per class of line; entries >= C are 0 */
    double mlf_max;                   /* the largest marginal loss factor over the masked nodes */
    int32_t mlf_max_index;            /* the lowest caller-side index that attains it; -1 */
    int32_t n_bad;                    /* 1: a bad slot, every double above a NaN */
} revs_loss_slot_t;                   /* 64 bytes */
typedef struct {
    double energy;                    /* (sum over the slots of loss) slot_hours */
    double peak;                      /* the largest loss of the day */
    int32_t peak_slot;                /* its earliest slot; -1 with a bad slot */
    int32_t reserved;
} revs_loss_line_day_t;               /* 24 bytes */
typedef struct {
    double energy, delivered;         /* (sum over the slots of total / delivered) slot_hours */
    double class_energy[4];
    double cost;                      /* (sum over the slots of total[t] cost[t]) slot_hours; NaN without cost */
    double peak;                      /* the largest slot total */
    double top_energy[8];             /* day energies of the lines top_index, descending; NaN: unused */
    int32_t top_index[8];             /* caller-side indices; -1: unused */
    int32_t peak_slot;
    int32_t n_bad_slots;
    int32_t reserved[6];
} revs_loss_day_t;                    /* 192 bytes */
int64_t revs_net_losses_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_losses(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const double *node_g,
                    const uint8_t *line_mask, const uint8_t *node_mask, const uint8_t *line_class, int32_t C,
                    const int32_t *node_of_pos, int32_t n_out, double vset2, double slot_hours, double loss_max,
                    const double *cost, double *loss_out, double *mlf_out, double *drop_out, double *flow_out,
                    revs_net_summary_t *summary_out, revs_loss_slot_t *slot_out, revs_loss_line_day_t *line_day_out,
                    revs_loss_day_t *day_out, void *scratch, void *stream);

/* ---- attribution report: who causes the watched node's voltage drop (csrc/attribution_kernels.hip) ------
 * drop = R g and R[j][i] = wc[lca(i, j)] (revs_headroom_aux_t), so node i contributes wc[lca(i, j*)] g[i] to the drop at a
 * watched node j*.  Positions j = 0 .. tree->n - 1 are feeder_tree's preorder positions; a is an ancestor-or-self of j iff
 * a <= j < end[a] (the pack's field).  Per (scenario s, slot t), every operation an IEEE double operation rounded on its
 * own (no fused multiply-add), with inj[i] the gathered node sum of node_g (+0.0 at a position without a row), ev[i] the
 * same gather of node_ev (double[S][m][T], the EV part of the injections; all +0.0 when node_ev is NULL) and drop the
 * bits of revs_net_report's scans:
 *   watch j*     watch_pos >= 0: that position in every slot.  watch_pos = -1: among the positions with limit_mask != 0
 *                (NULL: every position with a row) and a caller-side index, the one of largest drop, ties to the lowest
 *                caller-side index.  No candidate: watch = -1, every output of the slot is +0.0 and every count 0 (the
 *                summary's included).
 *   sens[i]      = wc[lca(i, j*)] = R[j*][i]; +0.0 when i and j* share no ancestor.  A selection: no rounding.  (wc must
 *                not decrease down a path: w >= 0.)
 *   contrib[i]   = sens[i] inj[i],  ev_contrib[i] = sens[i] ev[i]
 *   excess       = max(0, drop[j*] - drop_max)
 *   relief[i]    = excess / sens[i] where sens[i] > 0 (+inf where sens[i] = 0 and excess > 0; 0 when excess = 0): the cut
 *                at node i alone that brings j* back to the limit.  Not an output: it enters n_can.
 * Sums over positions: each the root of ONE fixed binary tree exactly as the loss report's (values by position, +0.0 at
 * padding, padded to the next power of two, x[i] = x[2i] + x[2i + 1]):
 *   total = sum of contrib (NOT forced to equal drop[j*]: they differ by rounding), ev_total = sum of ev_contrib,
 *   class_total[k] = sum of contrib over the positions with class_of_pos[j] == k (uint8 per position), k < C <= 4.
 * Counts over the positions with out_mask != 0 (NULL: all), a caller-side index and sens > 0:
 *   n_reach  how many there are;  n_big  those with contrib > frac drop[j*] (the product rounded once);
 *   n_can    those with excess > 0 and relief[i] <= ev[i].
 * Bad slot: a non-finite injection (node_g or node_ev) at a row of the tree.  Then every double of the slot is a NaN
 * (sens, contrib, ev_contrib, the slot record), watch = -1, n_bad = 1, the other counts 0, the summary has count 0 and
 * n_nan = the nodes summarised; drop_out is what the scans give.  One flag for the workgroup; nothing traps.
 * Outputs, any may be NULL, not all:
 *   sens_out, contrib_out, ev_contrib_out, drop_out   double[S][n_out][T] in the caller's node order (node_of_pos, n_out
 *                as revs_net_report's)
 *   slot_out     revs_attr_slot_t[S][T]; top_value / top_index = the eight nodes counted in n_reach of largest
 *                contribution, descending, ties to the lowest caller-side index, NaNs left out, unused entries NaN / -1
 *   summary_out  revs_net_summary_t[S][T]: the box-plot record of contrib over the n_reach nodes (box_select64 and the rules
 *                of boxplot.h); worst_value / worst_index = the largest contribution and the lowest caller-side index that
 *                attains it; n_violations = n_big; reserved[0] = the positions with out_mask and a caller-side index whose
 *                sens is 0
 *   day_out      revs_attr_day_t[S][n_out]: sum / ev_sum = the node's contrib / ev_contrib summed from +0.0 in ascending
 *                slot order over the slots with excess > 0; peak / peak_slot = its largest contrib over the slots that are
 *                not bad and the earliest such slot (NaN / -1: every slot is bad); n_big = the slots in which it counted
 *                in n_big
 * Enqueues only (up to three launches on `stream`): capturable, no allocation, no synchronisation.  REVS_EINVAL before any
 * launch: every case of revs_net_headroom's list that applies (S, T, m, node_g, the tree, n_out, the aux struct, drop_max
 * not finite, every output NULL); watch_pos outside -1..tree->n - 1; frac not finite or < 0; C outside 0..4; class_of_pos
 * NULL with C > 0; ev_contrib_out without node_ev; slot_out, summary_out or day_out without a 16-byte aligned scratch of
 * revs_net_attribution_scratch bytes (17 S T tree_n: contrib and ev_contrib by position and one flag byte per cell,
 * + 192 S T: the slot records; 0 for a bad size). */
typedef struct {
    double drop_watch;                /* drop[j*] */
    double excess;                    /* max(0, drop_watch - drop_max) */
    double total;                     /* sum of contrib */
    double ev_total;                  /* sum of ev_contrib */
    double class_total[4];            /* sum of contrib per class; entries >= C are 0 */
    double top_value[8];              /* the eight largest contributions, descending; NaN: unused */
    int32_t top_index[8];             /* their caller-side indices; -1: unused */
    int32_t watch;                    /* caller-side index of j*; -1 */
    int32_t n_reach;
    int32_t n_big;
    int32_t n_can;
    int32_t n_bad;                    /* 1: a bad slot, every double above a NaN */
    int32_t reserved[3];
} revs_attr_slot_t;                   /* 192 bytes */
typedef struct {
    double sum;                       /* sum over the slots with excess > 0 of contrib */
    double ev_sum;                    /* ... of ev_contrib */
    double peak;                      /* the largest contrib of the day */
    int32_t peak_slot;                /* its earliest slot; -1 */
    int32_t n_big;                    /* slots in which the node counted in n_big */
} revs_attr_day_t;                    /* 32 bytes */
int64_t revs_net_attribution_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_attribution(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const revs_headroom_aux_t *aux_host,
                         const double *node_g, const double *node_ev, const uint8_t *limit_mask, const uint8_t *out_mask,
                         const uint8_t *class_of_pos, int32_t C, const int32_t *node_of_pos, int32_t n_out,
                         int32_t watch_pos, double drop_max, double frac, double *sens_out, double *contrib_out,
                         double *ev_contrib_out, double *drop_out, revs_attr_slot_t *slot_out,
                         revs_net_summary_t *summary_out, revs_attr_day_t *day_out, void *scratch, void *stream);

/* ---- risk report: undervoltage odds under forecast error (csrc/risk_kernels.hip) -----------------------
 * The node sums are a forecast.  With independent zero-mean errors of variance s2[i] at the rows (node_var) and K shared
 * factors of unit variance with loadings beta_k[i] (node_common), the linear model drop = R g gives
 *   Var(drop[j]) = sum_i R[j][i]^2 s2[i] + sum_k ((R beta_k)[j])^2
 * and, with R[j][i] = wc[lca(i, j)] (revs_headroom_aux_t), the first term is the sum over j's ancestors-or-self a of
 * w2[a] Q[a], Q the subtree sums of s2 and w2[a] = wc[a]^2 - wc[parent(a)]^2.  Positions j = 0 .. tree->n - 1 are
 * feeder_tree's preorder positions.  Inputs, DEVICE arrays unless said otherwise:
 *   node_var     double[S][m][T]  variance of the independent error of each row's node sum; NULL: all +0.0
 *   node_common  double[K][S][m][T], K in 0..REVS_RISK_MAX_COMMON: the loadings of the shared factors; NULL with K = 0
 *   w2           double[tree->n]  per position w[j] (2.0 wc[j] - w[j]), the subtraction and the product each rounded once,
 *                +0.0 at padding positions (feeder.risk_weights, from aux_host's wc)
 *   z_max        (by value) the standard deviations of margin a node must keep, finite and >= 0: a node is at risk when
 *                z < z_max.  For a probability p_max it is the standard normal's quantile at 1 - p_max.
 * Per (scenario s, slot t), every operation one IEEE double operation rounded on its own (no fused multiply-add), drop
 * the bits of revs_net_report's scans, "flow scan" and "drop scan" those scans on other inputs:
 *   var_ind[j] = max(0, drop scan with w2 in place of w of (flow scan of the gathered node_var))      (+0.0 for a -0.0)
 *   c_k[j]     = drop scan of node_common[k]: exactly the drop's code path
 *   var[j]     = (var_ind[j] + c_0[j] c_0[j]) + c_1[j] c_1[j]          k ascending, the product, then the sum
 *   sd[j]      = sqrt(var[j]), correctly rounded
 *   slack[j]   = drop_max - drop[j]
 *   z[j]       = slack[j] / sd[j]; where sd[j] = 0: +inf when slack[j] >= 0, -inf when slack[j] < 0
 *   drop_q[j]  = drop[j] + z_max sd[j]     the drop that is exceeded with probability p_max (the "secure" drop)
 *   prob[j]    = 0.5 erfc(z[j] 0.70710678118654752)     P(drop + error > drop_max) for Gaussian errors; erfc is the
 *                device library's: a few ulp, not correctly rounded
 * var_ind's and c_k's bits depend on the launch shape as the drop's do; var_ind is within 2 n 2^-53 sum |w2 Q| of any order.
 * Bad slot: a non-finite node_g, node_var or node_common at a row of the tree, or a negative node_var.  Then every double
 * of the slot is a NaN (sd, z, prob, drop_q, the slot record), n_bad = 1, the counts 0, z_min_index -1, the summary has
 * count 0 and n_nan = the positions summarised; drop_out is what the scans give.  One flag for the workgroup; nothing
 * traps.
 * The covered positions of the slot record and the summary: limit_mask != 0 (NULL: every position with a row), out_mask
 * != 0 (NULL: all) and a caller-side index.  Outputs, any may be NULL, not all:
 *   sd_out, z_out, prob_out, drop_q_out, drop_out   double[S][n_out][T] in the caller's node order (node_of_pos, n_out as
 *                revs_net_report's)
 *   slot_out     revs_risk_slot_t[S][T] over the covered positions: expected = the sum of prob, the root of ONE fixed
 *                binary tree exactly as the loss report's (values by position, +0.0 where not covered, padded to the next
 *                power of two, x[i] = x[2i] + x[2i + 1]); n_risky = positions with z < z_max; n_det = positions with drop >
 *                drop_max (what revs_net_report counts); z_min and z_min_index (ties to the lowest caller-side index), sd_at
 *                / drop_at = sd and drop there; sd_max; none covered: the four doubles NaN, the index -1, expected +0.0
 *   summary_out  revs_net_summary_t[S][T]: the box-plot record of drop_q over the covered positions (a second launch,
 *                box_select64 and the rules of boxplot.h); n_violations = positions with drop_q > drop_max; worst_value /
 *                worst_index = the largest drop_q and the lowest caller-side index that attains it
 *   day_out      revs_risk_day_t[S][n_out], every node with a caller-side index, over the slots that are not bad: prob_max
 *                and its earliest slot, z_min, n_risky = the slots with z < z_max, expected_slots = the sum of prob from
 *                +0.0 in ascending slot order; every slot bad: NaN, -1, NaN, 0, +0.0
 * Enqueues only (up to three launches on `stream`): capturable, no allocation, no synchronisation.  REVS_EINVAL before any
 * launch: every case of revs_net_headroom's list that applies (S, T, m, node_g, the tree, n_out, the aux struct, drop_max
 * not finite, every output NULL); K outside 0..REVS_RISK_MAX_COMMON; node_common NULL with K > 0; a NULL w2; z_max not
 * finite or < 0; summary_out or day_out without a 16-byte aligned scratch of revs_net_risk_scratch bytes (24 S T tree_n:
 * drop_q, prob and z by position; 0 for a bad size). */
#define REVS_RISK_MAX_COMMON 2
typedef struct {
    double expected;                  /* sum of prob: the expected number of covered nodes below the limit */
    double z_min;                     /* the smallest margin in standard deviations */
    double sd_at;                     /* sd at z_min_index */
    double drop_at;                   /* drop at z_min_index */
    double sd_max;                    /* the largest sd */
    int32_t n_risky;                  /* positions with z < z_max */
    int32_t n_det;                    /* positions with drop > drop_max */
    int32_t z_min_index;              /* the lowest caller-side index that attains z_min; -1 */
    int32_t n_bad;                    /* 1: a bad slot, every double above a NaN */
    int32_t reserved[2];
} revs_risk_slot_t;                   /* 64 bytes */
typedef struct {
    double prob_max;                  /* the day's largest prob (NaN: every slot is bad) */
    double z_min;                     /* the day's smallest z */
    double expected_slots;            /* sum over the slots of prob */
    int32_t prob_max_slot;            /* the earliest slot of prob_max; -1 */
    int32_t n_risky;                  /* slots with z < z_max */
} revs_risk_day_t;                    /* 32 bytes */
int64_t revs_net_risk_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_risk(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const revs_headroom_aux_t *aux_host,
                  const double *node_g, const double *node_var, const double *node_common, int32_t K, const double *w2,
                  const uint8_t *limit_mask, const uint8_t *out_mask, const int32_t *node_of_pos, int32_t n_out,
                  double drop_max, double z_max, double *sd_out, double *z_out, double *prob_out, double *drop_q_out,
                  double *drop_out, revs_risk_slot_t *slot_out, revs_net_summary_t *summary_out, revs_risk_day_t *day_out,
                  void *scratch, void *stream);

/* ---- price report: nodal prices, congestion rent and line value from the voltage rows' multipliers
 * (csrc/price_kernels.hip) ---------------------------------------------------------------------------------
 * The first report of the dual side.  y are the signed multipliers of the voltage rows vlow^2 - vset^2 <= R g <= vhigh^2 -
 * vset^2 in the operator's convention (y > 0 where the upper row binds: load pulls R g up, so prices rise downstream of
 * a congested line), s the scale of L(s y).  With R = sum_e w_e 1_sub(e) 1_sub(e)^T, d = R y is the network report's two
 * scans on y, and g^T R y = sum_e w_e P_e Y_e.  Positions j = 0 .. tree->n - 1 are feeder_tree's preorder positions.
 * node_g and node_y are DEVICE double[S][m][T]; node_y is gathered through the tree's src exactly as node_g is (a
 * multiplier of a row the tree does not carry is dropped).  scale: DEVICE double[S], NULL: 1.0.  cost: DEVICE double[T].
 * Per (scenario, slot t), every operation an IEEE double operation rounded on its own (no fused multiply-add), w[j] =
 * tree->w[j] = 2 r[j]:
 *   inj, mu    the gathered node_g / node_y (+0.0 at a position without a row)
 *   flow, drop revs_net_report's bits on node_g
 *   Y[j]       the flow scan of mu: the bits revs_net_report's flow gives when fed node_y            -> line_y_out
 *   d[j]       the drop scan of w[j] Y[j]: the bits revs_net_report's drop gives when fed node_y
 *   cong[j]    s d[j]                                                                               -> cong_out
 *   mlf[j]     with_loss != 0: revs_net_losses' mlf at the same vset2 (its bits; den = vset2 - drop, c = (w flow) / den,
 *              the path sums of c in the drop scan's form); else +0.0
 *   lossp[j]   cost[t] mlf[j]                                                                       -> lossp_out
 *   price[j]   (cost[t] + lossp[j]) + cong[j]                                                       -> price_out
 *   rent[j]    ((w[j] Y[j]) flow[j]) s + 0.0: what the line above j collects (the last addition makes a zero
 *              rent +0.0 whatever the flow's sign; w = 0 gives +0.0)                                 -> rent_out
 * Bad slot: a gathered inj or mu is not finite; the scenario's s is not finite or not >= 0; with_loss and den[j] > 0
 * fails at a position with a caller-side index.  Then every price, cong, lossp, rent and every double of the slot record
 * is a NaN, the indices are -1, n_priced and n_rows are 0, n_bad is 1, and the summary has count 0 and n_nan = the nodes
 * summarised; drop_out, flow_out and line_y_out are what the scans give.  One flag for the workgroup; nothing traps.
 * Sums over positions: each the root of ONE fixed binary tree exactly as the loss report's.
 * Outputs, any may be NULL, not all:
 *   price_out, cong_out, lossp_out, line_y_out, rent_out, drop_out, flow_out   double[S][n_out][T] in the caller's node
 *                  order (node_of_pos, n_out as revs_net_report's)
 *   summary_out    revs_net_summary_t[S][T]: the box-plot record of price over the nodes with node_mask[j] != 0 (NULL: all)
 *                  and a caller-side index (a second launch, box_select64 and the rules of boxplot.h); worst_value = the
 *                  largest price, worst_index the lowest caller-side index that attains it; n_violations = nodes with
 *                  price > price_cap (+inf allowed)
 *   slot_out       revs_price_slot_t[S][T]: delivered = sum of inj; energy_pay = cost[t] delivered; loss_pay = sum of
 *                  inj lossp and cong_pay = sum of inj cong over the masked nodes (node_mask, caller-side index);
 *                  rent_total = sum of rent over the lines with line_mask[j] != 0 (NULL: all) and a caller-side index;
 *                  price_max, price_min, cong_max over the masked nodes, each with the lowest caller-side index that
 *                  attains it (NaN / -1 when there is none); n_priced = masked nodes with cong != 0; n_rows = positions
 *                  with mu != 0; n_bad
 *   node_day_out   revs_price_node_day_t[S][n_out]: paid = the sum from +0.0 in ascending slot order of the rounded
 *                  products inj price, multiplied once by slot_hours; cong_paid by the same rule on inj cong; peak_price /
 *                  peak_slot = the largest price and its earliest slot; a bad slot makes the doubles NaN and the slot -1
 *   line_day_out   revs_loss_line_day_t[S][n_out], the loss report's layout and rule on rent: energy = the day's rent
 *   day_out        revs_price_day_t[S]: the four payments by the same rule over the slot records; peak_price = the largest
 *                  slot price_max, peak_slot its earliest slot, peak_index that slot's price_max_index (NaN / -1 with a
 *                  bad slot); n_bad_slots; n_cong_slots = slots with n_rows > 0; top_index[8] / top_rent[8] = the eight
 *                  summarised lines of largest day rent in descending order, NaNs left out, ties to the lowest caller
 *                  index, unused entries -1 / NaN
 * Enqueues only (up to four launches on `stream`): capturable, no allocation, no synchronisation.  REVS_EINVAL before any
 * launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; m outside 1..65535; a null node_g, node_y or cost; a tree
 * over REVS_TREE_MAX, not padded or NULL; n_out outside 1..tree->n; with_loss and vset2 not finite and > 0; slot_hours not
 * finite and > 0; a NaN price_cap; every output NULL; summary_out, node_day_out, line_day_out or day_out without a 16-byte
 * aligned scratch of revs_net_prices_scratch bytes (32 S T tree_n: price, rent, inj price and inj cong by position, + 96 S T:
 * the slot records, + 8 S tree_n: the lines' day rents; 0 for a bad size).  A call with the scratch also parks the flows
 * and lossp of each (scenario, slot) in its rent and inj price cells until they are overwritten: the same results from
 * fewer registers. */
typedef struct {
    double delivered;                 /* sum of the injections */
    double energy_pay;                /* cost[t] delivered */
    double loss_pay;                  /* sum of inj lossp over the masked nodes */
    double cong_pay;                  /* sum of inj cong over the masked nodes */
    double rent_total;                /* sum of rent over the summarised lines */
    double price_max, price_min;      /* over the masked nodes */
    double cong_max;
    int32_t price_max_index;          /* the lowest caller-side index that attains each; -1 */
    int32_t price_min_index;
    int32_t cong_max_index;
    int32_t n_priced;                 /* masked nodes with cong != 0 */
    int32_t n_rows;                   /* positions with mu != 0 */
    int32_t n_bad;                    /* 1: a bad slot, every double above a NaN */
    int32_t reserved[2];
} revs_price_slot_t;                  /* 96 bytes */
typedef struct {
    double paid;                      /* (sum over the slots of inj price) slot_hours */
    double cong_paid;                 /* (sum over the slots of inj cong) slot_hours */
    double peak_price;                /* the largest price of the day */
    int32_t peak_slot;                /* its earliest slot; -1 with a bad slot */
    int32_t reserved;
} revs_price_node_day_t;              /* 32 bytes */
typedef struct {
    double energy_pay, loss_pay;      /* (sum over the slots of the slot record's field) slot_hours */
    double cong_pay, rent_total;
    double peak_price;                /* the largest slot price_max */
    double top_rent[8];               /* day rents of the lines top_index, descending; NaN: unused */
    int32_t top_index[8];             /* caller-side indices; -1: unused */
    int32_t peak_slot, peak_index;
    int32_t n_bad_slots;
    int32_t n_cong_slots;             /* slots with n_rows > 0 */
    int32_t reserved[2];
} revs_price_day_t;                   /* 160 bytes */
int64_t revs_net_prices_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_prices(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const double *node_g,
                    const double *node_y, const double *scale, const double *cost, const uint8_t *line_mask,
                    const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out, double vset2, int32_t with_loss,
                    double slot_hours, double price_cap, double *price_out, double *cong_out, double *lossp_out,
                    double *line_y_out, double *rent_out, double *drop_out, double *flow_out,
                    revs_net_summary_t *summary_out, revs_price_slot_t *slot_out, revs_price_node_day_t *node_day_out,
                    revs_loss_line_day_t *line_day_out, revs_price_day_t *day_out, void *scratch, void *stream);

/* ---- power-flow report: branch-flow voltages, losses and the linear model's error (csrc/powerflow_kernels.hip, DESIGN.md
 * 3.22) ------------------------------------------------------------------------------------------------------------------
 * The nonlinear branch-flow (DistFlow) equations of the radial feeder, which the linear model v^2 = vset^2 - R g of every
 * other report approximates, solved per (scenario s, slot t) by a fixed-point iteration over the network report's two
 * scans.  Positions j = 0 .. tree->n - 1 are feeder_tree's preorder positions; every operation is an IEEE double
 * operation rounded on its own (no fused multiply-add).  w[j] = tree->w[j] = 2 r[j]; xw[j] = 2 x[j] (DEVICE double[tree->n]
 * by position, 16-byte aligned, or NULL: active power only); inj[j] the gathered node sum (+0.0 without a row);
 * qinj[j] = tan_phi inj[j] (with xw only).  P[j], Q[j]: the receiving-end flows on the line above j; u[j]: the squared
 * voltage at j.
 *   cur[j] = (P[j] P[j] + Q[j] Q[j]) / u[j]      (without xw: (P[j] P[j]) / u[j])
 *   lp[j]  = (0.5 w[j]) cur[j]                   lq[j] = (0.5 xw[j]) cur[j]
 *   P[j]   = (the flow scan of inj + lp at j) - lp[j]        Q[j] = (the flow scan of qinj + lq at j) - lq[j]
 *   u[j]   = vset2 - the path scan at j of the terms ((w P + xw Q) + 0.5 (w lp + xw lq)), each product rounded, the sums
 *            in the order written
 * Pass 0 takes lp = lq = 0 and adds nothing for them: without xw its P and vset2 - u are revs_net_report's flow and drop
 * (the same bits); with xw its u is the linear model with the reactive term xw Q.  Pass k >= 1 forms cur, lp, lq from pass
 * k - 1's P, Q, u and runs the scans again.  The loop ends behind the first pass k >= 1 with max |u_new - u_old| <= tol vset2
 * over the positions with a caller-side index (iters = k, status 0), or behind pass max_iter (status 3).  loss_out is the
 * lp the last pass used: P, Q, u satisfy the flow and voltage equations with it, and it is cur of the pass before.
 * status per (s, t): 0 converged; 1 a row's injection is not finite; 2 collapse, u[j] > 0 fails at a position with a
 * caller-side index in some pass (pass 0 included); 3 max_iter reached.  With status != 0 every value of volt_out,
 * flow_out, loss_out and qflow_out of the slot is a NaN, every double of its slot record a NaN, its indices -1 and its
 * counts 0, and the summary has count 0; volt_lin_out stays what pass 0 gives.  One flag per workgroup; nothing traps.
 * Sums over positions: each the root of ONE fixed binary tree exactly as the loss report's.
 *   volt_out = sqrt(u), volt_lin_out = sqrt(pass 0's u) (a NaN where that is negative), flow_out = P, loss_out = lp,
 *   qflow_out = Q (needs xw): double[S][n_out][T] in the caller's node order, any may be NULL
 *   summary_out    revs_net_summary_t[S][T]: the box-plot record of volt over the positions with node_mask[j] != 0
 *                  (NULL: all) and a caller-side index; n_violations = nodes with volt < vmin; worst_value / worst_index
 *                  = the lowest voltage and the lowest caller index that attains it
 *   slot_out       revs_pf_slot_t[S][T]: loss_total / qloss_total = the sums of lp / lq over the positions with a
 *                  caller-side index, delivered = the sum of inj, supplied = delivered + loss_total; over the masked
 *                  nodes volt_min / volt_min_index, err_max / err_index = the largest volt_lin - volt (both: the lowest
 *                  index on ties), n_below (volt < vmin), n_below_lin (volt_lin < vmin), n_missed (volt < vmin and not
 *                  volt_lin < vmin); iters, status
 *   node_day_out   revs_pf_node_day_t[S][n_out]: over the slots whose voltage is no NaN the lowest and its earliest slot
 *                  (NaN / -1: none), slots_below, slots_missed
 *   day_out        revs_pf_day_t[S]: energy_lost / energy_delivered = the slots' loss_total / delivered summed from +0.0
 *                  in slot order, multiplied once by slot_hours (a NaN with a bad slot); cost = the sum of the rounded
 *                  products loss_total[t] cost[t], times slot_hours (cost: DEVICE double[T]; NULL: a NaN); the day's
 *                  lowest voltage with its earliest slot and that slot's node; the slots' counts added; iters_max;
 *                  n_bad_slots = slots with status != 0
 * Enqueues only (up to four launches on `stream`): capturable, no allocation, no synchronisation.  The state of the
 * iteration lives in the scratch, so every call needs it.  REVS_EINVAL before any launch: the tree and size checks of
 * revs_net_losses; vset2, slot_hours or tol not finite and > 0; vmin not finite; max_iter outside 1..REVS_PF_MAX_ITER;
 * tan_phi not finite; tan_phi != 0 with xw == NULL; xw not 16-byte aligned; qflow_out without xw; every output NULL; a
 * null or not 16-byte aligned scratch of revs_net_powerflow_scratch bytes (6 x 8 S T tree_n: u, then the voltages staged
 * by position; pass 0's voltages; P; Q; lp; lq, + 80 S T: the slot records; 0 for a bad size). */
#define REVS_PF_MAX_ITER 64
typedef struct {
    double loss_total, qloss_total;   /* kW / kvar lost on the lines */
    double delivered, supplied;       /* sum of inj; delivered + loss_total */
    double volt_min;                  /* the lowest voltage over the masked nodes */
    double err_max;                   /* the largest volt_lin - volt over the masked nodes */
    int32_t volt_min_index, err_index;
    int32_t n_below, n_below_lin;     /* masked nodes below vmin by branch flow / by the linear model */
    int32_t n_missed;                 /* below by branch flow and not by the linear model */
    int32_t iters;                    /* passes behind pass 0 */
    int32_t status;                   /* 0 converged, 1 not finite, 2 collapse, 3 max_iter */
    int32_t reserved;
} revs_pf_slot_t;                     /* 80 bytes */
typedef struct {
    double volt_min;                  /* the day's lowest voltage at the node */
    int32_t slot;                     /* its earliest slot; -1 */
    int32_t slots_below, slots_missed;
    int32_t reserved;
} revs_pf_node_day_t;                 /* 24 bytes */
typedef struct {
    double energy_lost, energy_delivered;     /* (sum over the slots of loss_total / delivered) slot_hours */
    double cost;                      /* (sum over the slots of loss_total[t] cost[t]) slot_hours; NaN without cost */
    double volt_min;                  /* the day's lowest voltage */
    int32_t volt_min_slot, volt_min_index;
    int32_t n_below, n_below_lin, n_missed;   /* node-slots */
    int32_t iters_max, n_bad_slots;
    int32_t reserved;
} revs_pf_day_t;                      /* 64 bytes */
int64_t revs_net_powerflow_scratch(int32_t S, int32_t T, int32_t tree_n);
int revs_net_powerflow(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree_host, const double *node_g,
                       const double *xw, double tan_phi, const uint8_t *node_mask, const int32_t *node_of_pos,
                       int32_t n_out, double vset2, double vmin, double tol, int32_t max_iter, double slot_hours,
                       const double *cost, double *volt_out, double *volt_lin_out, double *flow_out, double *loss_out,
                       double *qflow_out, revs_net_summary_t *summary_out, revs_pf_slot_t *slot_out,
                       revs_pf_node_day_t *node_day_out, revs_pf_day_t *day_out, void *scratch, void *stream);

/* ---- transformer report: loading, hot-spot and loss of life of the service transformers (csrc/transformer_kernels.hip,
 * DESIGN.md 3.17) --------------------------------------------------------------------------------------------------------
 * K transformers, each serving a list of rows of the node sums node_g (double[S][m][T], revs_net_node_sums' layout):
 * xf_ptr int32[K + 1] and xf_rows int32[nnz] in CSR form, rows ascending within a transformer, a row in at most one list
 * (rows in no list are ignored); rated_kw double[K] = rated kVA x power factor; ambient double[T] in deg C -- all DEVICE
 * arrays.  It needs no feeder tree.  One thermal model per call (IEEE C57.91 Clause 7: top-oil and winding rises that
 * follow their ultimate values exponentially, Arrhenius ageing), every value a parameter.  Per (scenario, transformer k,
 * slot t), every operation that is no pow / exp one IEEE double operation rounded on its own (no fused multiply-add):
 *   load  = g[row][t] summed from +0.0 over k's rows in list order
 *   ratio = |load| / rated_kw[k]
 *   u_to  = dto_r pow((ratio ratio loss_ratio + 1) / (loss_ratio + 1), n)         the ultimate top-oil rise
 *   u_w   = dhs_r pow(ratio ratio, m)                                             the ultimate winding rise over top oil
 *   `substeps` sub-steps of slot_hours / substeps each:
 *       x = u_to + (x - u_to) decay_to;  y = u_w + (y - u_w) decay_w;  hot = (ambient[t] + x) + y;
 *       acc += exp(aging_B / (theta_ref + 273) - aging_B / (hot + 273))           (acc from +0.0)
 *   top_oil[t] = x, hot_spot[t] = hot of the last sub-step, faa[t] = acc / substeps
 * decay_to = exp(-slot_hours / (substeps tau_to)) and decay_w likewise are formed by the caller (decay_w = 0: the winding
 * follows at once).  cyclic = 0: x = to0, y = w0 before slot 0.  cyclic = 1 (the day repeats): the T substeps sub-steps
 * run once from x = y = 0 while aN = the product of the decay_to (awN: of the decay_w) is multiplied up from 1.0; the
 * real pass starts from x_end / (1 - aN), y_end / (1 - awN).  The state is sampled at the end of each sub-step.
 * A transformer is BAD in a scenario when a row of its list is not finite in some slot, its rated_kw is not finite and
 * > 0, or a listed row lies outside 0..m-1 (such a row is never read and adds nothing to load): load and ratio keep their
 * per-slot values, top_oil / hot_spot / faa and every double of its day record are NaN, its counts 0 and its slots -1.
 * A transformer without rows has load 0 and is valid.  xf_ptr entries are clamped to 0..nnz.
 *   load_out, ratio_out, top_oil_out, hot_out, faa_out   double[S][K][T]
 *   xf_day_out     revs_xf_day_t[S][K]: peak_ratio / peak_hot and their earliest slots; energy_kwh = the |load| summed
 *                  from +0.0 in slot order, times slot_hours once; age_hours = the faa summed likewise, times slot_hours;
 *                  lol_percent = 100 age_hours / normal_life_hours; feqa = age_hours / (T slot_hours); n_over_slots =
 *                  slots with ratio > over_ratio, n_hot_slots = slots with hot_spot > hot_limit
 *   sum_ratio_out, sum_hot_out   revs_net_summary_t[S][T]: the box-plot record over the K transformers of the ratios
 *                  (n_violations: ratio > over_ratio) and of the hot-spots (n_violations: hot > hot_limit), NaNs counted
 *                  in n_nan and left out; worst_value the largest value, worst_index the lowest transformer that has it
 *   fleet_out      revs_xf_fleet_t[S]: n_xf = K; n_nan = transformers whose lol_percent is a NaN; n_overloaded / n_hot /
 *                  n_aging = transformers with n_over_slots > 0 / n_hot_slots > 0 / feqa > 1; lol_sum, energy_kwh and the
 *                  sum behind feqa_mean = (sum of age_hours) / ((K T) slot_hours) are each the root of one binary tree
 *                  over the day records' values by transformer index, padded with +0.0 to a power of two (the values are
 *                  >= +0.0 or NaN, so a padding zero changes no bit; a NaN record makes them NaN); lol_max = top_lol[0];
 *                  top_index[8] / top_lol[8] = the eight transformers of largest lol_percent in descending order, NaNs
 *                  left out, ties to the lowest index, unused entries -1 / NaN
 * Every output may be NULL.  Enqueues only (up to four launches on `stream`): capturable, no allocation, no
 * synchronisation.  REVS_EINVAL before any launch: S outside 1..REVS_STUDY_MAX_S; T outside 1..REVS_MAX_T; m or K outside
 * 1..65535; nnz outside 0..m; a null node_g, xf_ptr, rated_kw, ambient or model, a null xf_rows with nnz > 0; a model
 * value that is not finite, dto_r, dhs_r, loss_ratio, n, m, aging_B or normal_life_hours not > 0, theta_ref not > -273;
 * substeps outside 1..16; a decay outside [0, 1); slot_hours not finite and > 0; cyclic not 0 or 1; to0 or w0 not finite
 * with cyclic = 0; over_ratio or hot_limit a NaN; every output NULL; sum_ratio_out, sum_hot_out or fleet_out without a
 * 16-byte aligned scratch of revs_xf_report_scratch bytes (16 S T K: the ratios and hot-spots by slot, + 64 S K: the day
 * records; 0 for a bad size). */
typedef struct {
    double dto_r;                     /* top-oil rise over ambient at rated load, K (55) */
    double dhs_r;                     /* winding hot-spot rise over top oil at rated load, K (25) */
    double loss_ratio;                /* load loss / no-load loss at rated load (5) */
    double n;                         /* top-oil exponent (0.8) */
    double m;                         /* winding exponent (0.8) */
    double aging_B;                   /* Arrhenius constant, K (15000) */
    double theta_ref;                 /* hot-spot at which the ageing factor is 1, deg C (110) */
    double normal_life_hours;         /* insulation life at theta_ref, h (180000) */
} revs_xf_model_t;                    /* 64 bytes */
typedef struct {
    double peak_ratio;                /* the largest load ratio of the day */
    double peak_hot;                  /* the largest hot-spot, deg C */
    double energy_kwh;                /* (sum over the slots of |load|) slot_hours */
    double age_hours;                 /* (sum over the slots of faa) slot_hours: insulation life used */
    double lol_percent;               /* 100 age_hours / normal_life_hours */
    double feqa;                      /* age_hours / (T slot_hours): the equivalent ageing factor */
    int32_t peak_ratio_slot;          /* the earliest slot of peak_ratio; -1: a bad transformer */
    int32_t peak_hot_slot;
    int32_t n_over_slots;             /* slots with ratio > over_ratio */
    int32_t n_hot_slots;              /* slots with hot_spot > hot_limit */
} revs_xf_day_t;                      /* 64 bytes */
typedef struct {
    double lol_sum;                   /* sum of lol_percent over the transformers */
    double lol_max;                   /* the largest lol_percent (NaN: none) */
    double energy_kwh;                /* sum of energy_kwh */
    double feqa_mean;                 /* (sum of age_hours) / ((n_xf T) slot_hours) */
    double top_lol[8];                /* lol_percent of the transformers top_index, descending; NaN: unused */
    int32_t top_index[8];             /* -1: unused */
    int32_t n_xf;
    int32_t n_nan;                    /* bad transformers: their day records are NaN */
    int32_t n_overloaded;             /* transformers with n_over_slots > 0 */
    int32_t n_hot;                    /* transformers with n_hot_slots > 0 */
    int32_t n_aging;                  /* transformers with feqa > 1 */
    int32_t reserved[3];
} revs_xf_fleet_t;                    /* 160 bytes */
int64_t revs_xf_report_scratch(int32_t S, int32_t T, int32_t K);
int revs_xf_report(int32_t S, int32_t m, int32_t T, int32_t K, int32_t nnz, const double *node_g, const int32_t *xf_ptr,
                   const int32_t *xf_rows, const double *rated_kw, const double *ambient, const revs_xf_model_t *model,
                   double slot_hours, int32_t substeps, double decay_to, double decay_w, int32_t cyclic, double to0,
                   double w0, double over_ratio, double hot_limit, double *load_out, double *ratio_out,
                   double *top_oil_out, double *hot_out, double *faa_out, revs_net_summary_t *sum_ratio_out,
                   revs_net_summary_t *sum_hot_out, revs_xf_day_t *xf_day_out, revs_xf_fleet_t *fleet_out, void *scratch,
                   void *stream);

/* ---- flexibility report: up and down reserve per EV, node and slot (csrc/flex_kernels.hip) ----------
 * How much of a schedule's charging can still be moved, where and when, without a car leaving under target: a closed
 * form of the charger power (revs_charge_report's p, strides and homes, under the same rules) and the records.
 * Energy is in kW x slots (soc[t + 1] = soc[t] + p[t] / capacity).
 *
 * Per row (residence i, scenario s) with ev != 0, the record's fields widened to double, every double operation rounded
 * on its own, no fused multiply-add, every comparison with a NaN false, min2(a, b) = (b < a) ? b : a:
 *   ws = clamp(start, 0, T), we = clamp(end, 0, T), W = max(we - ws, 0) (revs_rule_schedule's window);
 *   r = rating, c = capacity, i0 = initial, tgt = (i0 > 0.9) ? i0 : 0.9;
 *   E_lo = (tgt - i0) c, E_hi = (1.0 - i0) c (revs_rule_schedule's expressions);
 *   done(t) = sum of (double) p[u], u < t: one accumulator from +0.0, u ascending; energy = done(T);
 *   A(t) = (double) max(we - max(t + 1, ws), 0) r: what full-rate charging in the window slots after t can still deliver.
 * For a window slot ws <= t < we, d = (double) p[t]:
 *   up[t], the largest extra power in slot t that leaves the state of charge at or below 1 after the slot:
 *     m = min2(r - d, (E_hi - done(t)) - d);  up = (m > 0) ? ((m < r) ? m : r) : 0
 *   down[t], the largest cut in slot t after which full-rate charging in every later window slot still reaches the target:
 *     m = ((done(t) + d) + A(t)) - E_lo;  q = (d < r) ? d : r;  down = (m > 0 && q > 0) ? min2(q, m) : 0
 *   integral != 0 (on/off chargers), with the m and q above:
 *     up = (up >= r) ? r : 0;  down = (d > on_frac r && m >= d && q > 0) ? q : 0
 * Outside the window both are 0.  By construction 0 <= up, down <= r and neither is a NaN for any finite r: a NaN, +-inf
 * or negative power only sets the flag.
 *
 * row_rec [S][n]: up_energy, down_energy: the sums over t ascending from +0.0; n_up, n_down: the slots with a value > 0;
 *   laxity = (double) W - E_lo / r: the slots of freedom the car has at all (r <= 0: what IEEE gives); ready: the
 *   smallest t in 0..T for which tgt - (i0 + done(t) / c) > short_tol is false (the charging report's under-target test
 *   along the day), -1: none; slack = we - ready (it may be negative), 0 when ready == -1.  flags: bit 0 ev != 0; bit 1
 *   ready == -1; bit 2 some p[t] is not finite; bit 3 E_lo > (double) W r (cannot be served whatever the schedule);
 *   bit 4 ready > we.  A row with ev == 0 gets zeros, ready = -1, flags 0; its p is not read.
 * slot_rec[s][t] ([S][T]) over the EV rows: n_plugged (ws <= t < we), n_up, n_down (rows with a value > 0), up, down:
 *   sums in a fixed order, the same bits from call to call.
 * day_rec[s] ([S]), a function of the slot and row records of the same call whether or not they are asked for:
 *   up_energy, down_energy: the slots' sums added, t ascending from +0.0; peak_up / peak_up_slot, peak_down /
 *   peak_down_slot by a scan from slot 0 that moves on `>` only, both slots -1 without an EV; n_ev, n_never_ready (bit
 *   1), n_unservable (bit 3), n_late (bit 4), n_rigid (EV rows with n_up == 0 && n_down == 0).
 * hist: int32[S][2][T + 1]: [0] of ready (rows with ready >= 0), [1] of slack (rows with ready >= 0 and 0 <= slack <= T).
 * node_up, node_down: double[S][m][T], asked for together and with node_ptr: device int64[m + 1], CSR offsets of the
 *   rows sorted by node (node_ptr[0] = 0, node_ptr[m] = n, ascending; rows outside are left out).  Node j, slot t: the
 *   sum of revs_q36(up[t]) over the node's rows (rounding to a multiple of 2^-36; numpy: (x + 98304.0) - 98304.0 and a
 *   plain sum).  Every addition is exact while ratings stay below 2^15 kW and a node's sum below 2^17 kW, so any order
 *   of summation gives the same bits; beyond, the result is unspecified.  A node without rows gets +0.0.
 * val_out: double[4][S][n]: up_energy, down_energy, (double) slack, laxity; a NaN where the row is no EV or flags bit 2
 *   is set, and for slack where ready == -1.  keep_out: uint8[S][n], 1 for EV rows without bit 2.  The two are what
 *   revs_bill_study (base = -1) takes: the box-plot records come from that selection.
 * Any output may be NULL, not all; the others are the same bytes.  Reads p, homes, node_ptr; writes the outputs and the
 * scratch.  A thread owns a row and walks its slots in chunks of revs_flex_report_chunk() staged through LDS, done(t) in
 * a register: one pass over p; the scenario is grid.y.  Slot counts: wavefront ballots, LDS counters, one global integer
 * atomic per (workgroup, slot, counter); slot sums: per-workgroup partials in the scratch, folded in a fixed order by a
 * second kernel; a third derives the day records.  Node sums: LDS accumulators over the consecutive rows of a node, one
 * global f64 add per (workgroup, node, slot) into the zeroed output -- the only floating-point atomics, all exact.  No
 * grid-wide barrier, a fixed sequence of launches and memsets on one stream; the call only enqueues.  REVS_EINVAL
 * before any launch: everything revs_charge_report refuses; one node output without the other; a node output without
 * node_ptr or with m < 1; m S T >= 2^31.  scratch: revs_flex_report_scratch bytes (<= 0 for sizes the report refuses). */
typedef struct {
    double up_energy, down_energy, laxity, energy;
    int32_t ready, slack, n_up, n_down, flags;
    int32_t reserved[3];
} revs_flex_row_t;                    /* 64 bytes */
typedef struct {
    int32_t n_plugged, n_up, n_down, reserved;
    double up, down;
} revs_flex_slot_t;                   /* 32 bytes */
typedef struct {
    double up_energy, down_energy, peak_up, peak_down;
    int32_t peak_up_slot, peak_down_slot, n_ev, n_never_ready, n_unservable, n_late, n_rigid, reserved;
} revs_flex_day_t;                    /* 64 bytes */
int32_t revs_flex_report_chunk(void);
int64_t revs_flex_report_scratch(int32_t S, int64_t n, int32_t T);
int revs_flex_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                     const revs_home_t *homes, int32_t integral, double on_frac, double short_tol,
                     const int64_t *node_ptr, int32_t m,
                     revs_flex_row_t *row_rec, revs_flex_slot_t *slot_rec, revs_flex_day_t *day_rec, int32_t *hist,
                     double *node_up, double *node_down, double *val_out, uint8_t *keep_out,
                     void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REVS_ADMM_OPS_H */
