// The power-flow report (include/revs_admm_ops.h, "power-flow report"): the nonlinear branch-flow
// (DistFlow) equations of the radial feeder solved per slot and scenario by a fixed-point iteration over the tree
// reports' two scans -- true voltages, flows and losses, and beside them the linear model's voltages, cell by cell.
//
//   revs_net_powerflow   net_pf_kernel<NT, IPT, HAS_Q>, the four shapes of tree_shape(), on revs_net_study's T x S grid;
//                        then pf_summary_kernel (one workgroup per (slot, scenario), box_select64 over the staged
//                        voltages), pf_node_day_kernel (one thread per (scenario, position)) and pf_day_kernel (one
//                        thread per scenario: the slot loops)
//
// One workgroup per (slot, scenario).  Pass 0 is the network report's flow and drop scans (net_scans.h: the same bits
// without xw).  Every later pass forms cur, lp and lq from the state the pass before left, runs the flow scan on
// inj + lp (and on qinj + lq with xw), then the path scan on the voltage terms.  The state -- P, Q, u, lp, lq, one double
// a position each -- lives in the caller's scratch between the scans, in every shape: a thread reads back only the
// positions it wrote itself, so no barrier guards it, and the scans keep the registers they have in the sibling kernels
// (the 1024-thread shapes have 128 a thread; the scan buffer alone takes 128 KB of LDS in the 1024 x 16 shape).
//
// The loop's exit is one decision per workgroup: the flags through __syncthreads_or and the largest |u_new - u_old|
// through LDS behind that barrier, read by every thread alike.  No thread leaves a pass early; max_iter bounds the loop.
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"       // pair_tree, arg_better, wave_argmax
#include "net_scans.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

struct PfArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const double *xw;             // per position, or NULL (HAS_Q false)
    const uint8_t *node_mask;     // per position, or NULL (every node)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t m, T, n_out, max_iter;
    int32_t P;                    // threads that hold leaves of the fixed tree
    double vset2, vmin, thr, tan_phi;     // thr = tol vset2
    double *volt, *volt_lin, *flow, *loss, *qflow;     // [S][n_out][T], or NULL
    revs_pf_slot_t *slot;         // [S][T], or NULL
    revs_pf_slot_t *slot_scr;     // [S][T] in the scratch, or NULL
    double *sP, *sQ, *sU, *sLP, *sLQ, *sVL;            // [S][T][n] by position: the state; sU ends as the staged voltages
};

constexpr int kPfSums = 3;         // delivered, loss_total, qloss_total
constexpr int kPfRedDoubles = kPfSums * 16 + 2 * 16 + 16 + 24 + 16;    // sums, arg values, arg indices, counts, |du|

inline size_t pf_lds_bytes(int n) { return (tree_lds_doubles_even(n) + kPfRedDoubles) * sizeof(double); }

// the larger of two, a NaN winning over everything
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// Everything below rounds each operation on its own (the contract's IEEE operations): no product is fused into a sum.
#pragma clang fp contract(off)

template <int NT, int IPT, bool HAS_Q>
__global__ __launch_bounds__(NT) void net_pf_kernel(PfArgs A0) {
    extern __shared__ double pf_lds[];
    double *lds = pf_lds;
    PfArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T, st = ((int64_t)sc * T + t) * n;
        A.g += (int64_t)sc * A.m * T;
        if (A.volt) A.volt += arr;
        if (A.volt_lin) A.volt_lin += arr;
        if (A.flow) A.flow += arr;
        if (A.loss) A.loss += arr;
        if (A.qflow) A.qflow += arr;
        A.sP += st; A.sQ += st; A.sU += st; A.sLP += st; A.sLQ += st; A.sVL += st;
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *sred = lds + net_lds_doubles<NT, IPT>();               // [kPfSums][16]
    double *mred = sred + kPfSums * 16;                             // [2][16]
    int *ired = reinterpret_cast<int *>(mred + 32);                 // [2][16]
    int *cred = ired + 32;                                          // [3][16]
    double *dred = reinterpret_cast<double *>(cred + 48);           // [16]
    const double nan = __builtin_nan("");
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) lds[1] = 0.0;                                     // base[-1]

    double deliv = 0.0;                                             // this thread's subtree of the sum of inj
    bool bad = false;
    int status = 0, iters = 0;
    for (int pass = 0;; ++pass) {                                   // (every branch on pass, status and the flags is uniform)
        double a[IPT];
        unsigned se[IPT];
        // ---- the active flows: the subtree sums of inj + lp, less the line's own lp
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, &bad);     // (A's fields, not locals: net_scans.h)
        if (pass == 0) {
            deliv = pair_tree<IPT>(a);
        } else if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) {
                const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + j0 + i);
                const TreeD2 pv = *reinterpret_cast<const TreeD2 *>(A.sP + j0 + i);
                const TreeD2 uv = *reinterpret_cast<const TreeD2 *>(A.sU + j0 + i);
                TreeD2 xv = TreeD2{{0.0, 0.0}}, qv = TreeD2{{0.0, 0.0}};
                if constexpr (HAS_Q) {
                    xv = *reinterpret_cast<const TreeD2 *>(A.xw + j0 + i);
                    qv = *reinterpret_cast<const TreeD2 *>(A.sQ + j0 + i);
                }
                TreeD2 lp, lq;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    double sq = pv.v[e] * pv.v[e];
                    if constexpr (HAS_Q) { const double qq = qv.v[e] * qv.v[e]; sq = sq + qq; }
                    const double cur = sq / uv.v[e];
                    lp.v[e] = (0.5 * wv.v[e]) * cur;
                    lq.v[e] = HAS_Q ? (0.5 * xv.v[e]) * cur : 0.0;
                    a[i + e] = a[i + e] + lp.v[e];
                }
                *reinterpret_cast<TreeD2 *>(A.sLP + j0 + i) = lp;
                if constexpr (HAS_Q) *reinterpret_cast<TreeD2 *>(A.sLQ + j0 + i) = lq;
            }
        }
        NET_CHUNK_FENCE();
        net_flow_scan<NT, IPT>(act, lds, se, a);
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) {
                if (pass > 0) {
                    const TreeD2 lp = *reinterpret_cast<const TreeD2 *>(A.sLP + j0 + i);
                    a[i] = a[i] - lp.v[0]; a[i + 1] = a[i + 1] - lp.v[1];
                }
                *reinterpret_cast<TreeD2 *>(A.sP + j0 + i) = TreeD2{{a[i], a[i + 1]}};
            }
        }
        NET_CHUNK_FENCE();
        // ---- the reactive flows, likewise on qinj + lq; then the active ones back for the voltage terms
        if constexpr (HAS_Q) {
            net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, nullptr);
#pragma unroll
            for (int i = 0; i < IPT; ++i) a[i] = A.tan_phi * a[i];
            if (pass > 0 && act) {
#pragma unroll
                for (int i = 0; i < IPT; i += 2) {
                    const TreeD2 lq = *reinterpret_cast<const TreeD2 *>(A.sLQ + j0 + i);
                    a[i] = a[i] + lq.v[0]; a[i + 1] = a[i + 1] + lq.v[1];
                }
            }
            net_flow_scan<NT, IPT>(act, lds, se, a);
            if (act) {
#pragma unroll
                for (int i = 0; i < IPT; i += 2) {
                    if (pass > 0) {
                        const TreeD2 lq = *reinterpret_cast<const TreeD2 *>(A.sLQ + j0 + i);
                        a[i] = a[i] - lq.v[0]; a[i + 1] = a[i + 1] - lq.v[1];
                    }
                    *reinterpret_cast<TreeD2 *>(A.sQ + j0 + i) = TreeD2{{a[i], a[i + 1]}};
                    const TreeD2 pv = *reinterpret_cast<const TreeD2 *>(A.sP + j0 + i);
                    a[i] = pv.v[0]; a[i + 1] = pv.v[1];
                }
            }
            NET_CHUNK_FENCE();
        }
        // ---- the voltage terms w P + xw Q + 0.5 (w lp + xw lq), their path sums, u = vset2 - them
        net_times_w<IPT>(tr, act, jl, a);
        if ((HAS_Q || pass > 0) && act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) {
                TreeD2 xv = TreeD2{{0.0, 0.0}};
                if constexpr (HAS_Q) {
                    xv = *reinterpret_cast<const TreeD2 *>(A.xw + j0 + i);
                    const TreeD2 qv = *reinterpret_cast<const TreeD2 *>(A.sQ + j0 + i);
                    const double x0 = xv.v[0] * qv.v[0], x1 = xv.v[1] * qv.v[1];
                    a[i] = a[i] + x0; a[i + 1] = a[i + 1] + x1;
                }
                if (pass > 0) {
                    const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + j0 + i);
                    const TreeD2 lp = *reinterpret_cast<const TreeD2 *>(A.sLP + j0 + i);
                    double h0 = wv.v[0] * lp.v[0], h1 = wv.v[1] * lp.v[1];
                    if constexpr (HAS_Q) {
                        const TreeD2 lq = *reinterpret_cast<const TreeD2 *>(A.sLQ + j0 + i);
                        const double g0 = xv.v[0] * lq.v[0], g1 = xv.v[1] * lq.v[1];
                        h0 = h0 + g0; h1 = h1 + g1;
                    }
                    h0 = 0.5 * h0; h1 = 0.5 * h1;
                    a[i] = a[i] + h0; a[i + 1] = a[i + 1] + h1;
                }
            }
        }
        NET_CHUNK_FENCE();
        net_path_scan<NT, IPT>(tr, act, jl, lds, a);
        double dmax = 0.0;
        bool coll = false;
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; i += 2) {
                const double u0 = A.vset2 - a[c + i], u1 = A.vset2 - a[c + i + 1];
                coll |= (nd[i] >= 0 && !(u0 > 0.0)) || (nd[i + 1] >= 0 && !(u1 > 0.0));
                if (pass == 0) {
                    const double l0 = sqrt(u0), l1 = sqrt(u1);      // (a NaN where the radicand is negative)
                    if (A.volt_lin && nd[i] >= 0) A.volt_lin[(int64_t)nd[i] * T + t] = l0;
                    if (A.volt_lin && nd[i + 1] >= 0) A.volt_lin[(int64_t)nd[i + 1] * T + t] = l1;
                    if (act) *reinterpret_cast<TreeD2 *>(A.sVL + j0 + c + i) = TreeD2{{l0, l1}};
                } else if (act) {
                    const TreeD2 uo = *reinterpret_cast<const TreeD2 *>(A.sU + j0 + c + i);
                    if (nd[i] >= 0) dmax = nan_max(dmax, fabs(u0 - uo.v[0]));
                    if (nd[i + 1] >= 0) dmax = nan_max(dmax, fabs(u1 - uo.v[1]));
                }
                if (act) *reinterpret_cast<TreeD2 *>(A.sU + j0 + c + i) = TreeD2{{u0, u1}};
            }
            NET_CHUNK_FENCE();
        }
        // ---- the workgroup's one decision
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) dmax = nan_max(dmax, __shfl_xor(dmax, o));
        if (lane == 0) dred[wave] = dmax;
        const bool anybad = __syncthreads_or(bad ? 1 : 0) != 0;      // (its barrier: every read of F is done, dred is written)
        const bool anycoll = __syncthreads_or(coll ? 1 : 0) != 0;
        double dm = dred[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) dm = nan_max(dm, dred[w]);
        if (anybad) { status = 1; break; }
        if (anycoll) { status = 2; break; }
        if (pass > 0) {
            iters = pass;
            if (dm <= A.thr) break;
            if (pass >= A.max_iter) { status = 3; break; }
        }
    }
    // ---- the arrays out, the voltages staged by position; this thread's leaves of the sums, its extremes and counts
    const bool ok = status == 0;
    double hl[IPT / kNetChunk], hq[IPT / kNetChunk];               // the chunks' subtrees of the sums of lp and lq
    double bvv = 0.0, bev = 0.0;
    int bvi = -1, bei = -1, cnt[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long nm = net_load_bytes(A.node_mask, jl + c);
        double xl[kNetChunk], xq[kNetChunk];
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) {
            const int j = jl + c + i;
            const bool on = ok && nd[i] >= 0;
            const double v = on ? sqrt(A.sU[j]) : nan;
            const double p = on ? A.sP[j] : nan;
            const double lp = on ? A.sLP[j] : nan;                  // (ok: at least one pass behind pass 0 has written it)
            double q = nan, lq = on ? 0.0 : nan;
            if constexpr (HAS_Q) {
                if (on) { q = A.sQ[j]; lq = A.sLQ[j]; }
            }
            xl[i] = on ? lp : 0.0;
            xq[i] = on ? lq : 0.0;
            if (nd[i] >= 0) {
                const int64_t at = (int64_t)nd[i] * T + t;
                if (A.volt) A.volt[at] = v;
                if (A.flow) A.flow[at] = p;
                if (A.loss) A.loss[at] = lp;
                if constexpr (HAS_Q) { if (A.qflow) A.qflow[at] = q; }
            }
            if (on && ((nm >> (8 * i)) & 0xFFull) != 0ull) {
                const double vl = A.sVL[j], err = vl - v;
                arg_better(bvv, bvi, -v, nd[i]);
                if (err == err) arg_better(bev, bei, err, nd[i]);
                const bool below = v < A.vmin, below_lin = vl < A.vmin;
                cnt[0] += below ? 1 : 0; cnt[1] += below_lin ? 1 : 0; cnt[2] += (below && !below_lin) ? 1 : 0;
            }
            if (act) A.sU[j] = ok ? sqrt(A.sU[j]) : nan;           // (positions without a caller-side index included)
        }
        hl[c / kNetChunk] = pair_tree<kNetChunk>(xl);
        hq[c / kNetChunk] = pair_tree<kNetChunk>(xq);
        NET_CHUNK_FENCE();
    }
    if (!A.slot && !A.slot_scr) return;                             // (uniform)
    // ---- the fixed tree above the threads: lanes by an xor butterfly, then the wavefronts' roots level by level
    double root[kPfSums] = {deliv, pair_tree<IPT / kNetChunk>(hl), pair_tree<IPT / kNetChunk>(hq)};
    const int P = A.P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if (o < P) {                                                // (uniform)
#pragma unroll
            for (int q = 0; q < kPfSums; ++q) root[q] += __shfl_xor(root[q], o);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) cnt[q] += __shfl_xor(cnt[q], o);
    }
    wave_argmax(bvv, bvi);
    wave_argmax(bev, bei);
    const int W = P > 64 ? P / 64 : 1;
    if (lane == 0) {
        if (wave < W) {
#pragma unroll
            for (int q = 0; q < kPfSums; ++q) sred[q * 16 + wave] = root[q];
        }
        mred[wave] = bvv; ired[wave] = bvi;
        mred[16 + wave] = bev; ired[16 + wave] = bei;
#pragma unroll
        for (int q = 0; q < 3; ++q) cred[q * 16 + wave] = cnt[q];
    }
    __syncthreads();
    if (tid < kPfSums) {
        double *r = sred + tid * 16;
        for (int w = W; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    } else if (tid == 64 || tid == 65) {
        const int k = (tid - 64) * 16;
        double v = mred[k];
        int ix = ired[k];
        for (int w = 1; w < NT / 64; ++w) arg_better(v, ix, mred[k + w], ired[k + w]);
        mred[k] = v; ired[k] = ix;
    } else if (tid >= 128 && tid < 131) {
        int *r = cred + (tid - 128) * 16;
        int s = 0;
        for (int w = 0; w < NT / 64; ++w) s += r[w];
        r[0] = s;
    }
    __syncthreads();
    if (tid == 0) {
        revs_pf_slot_t r;
        r.delivered = ok ? sred[0] : nan;
        r.loss_total = ok ? sred[16] : nan;
        r.qloss_total = ok ? sred[32] : nan;
        r.supplied = ok ? sred[0] + sred[16] : nan;
        const int vi = ok ? ired[0] : -1, ei = ok ? ired[16] : -1;
        r.volt_min = vi >= 0 ? -mred[0] : nan;
        r.volt_min_index = vi;
        r.err_max = ei >= 0 ? mred[16] : nan;
        r.err_index = ei;
        r.n_below = ok ? cred[0] : 0; r.n_below_lin = ok ? cred[16] : 0; r.n_missed = ok ? cred[32] : 0;
        r.iters = iters; r.status = status; r.reserved = 0;
        if (A.slot) A.slot[(size_t)sc * T + t] = r;
        if (A.slot_scr) A.slot_scr[(size_t)sc * T + t] = r;
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged voltages over the nodes with node_mask
constexpr int kPfSumNT = 256;
struct PfSumArgs {
    const double *stage;          // [S][T][n]
    const uint8_t *mask;          // node_mask per position, or NULL
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T]
    int32_t T, n, n_out;
    double vmin;
};

__global__ __launch_bounds__(kPfSumNT) void pf_summary_kernel(PfSumArgs A) {
    __shared__ BoxSelect<kPfSumNT> sh;
    constexpr int NT = kPfSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf();
    auto walk = [&](auto f) {
        net_for_each<NT>(row, A.n, A.nop, A.n_out, A.mask, [&](double v, int nd, int) { f(box_key(v), nd >= 0 && v == v, v, 0, nd); });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, below vmin
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        if (ok) {
            s[2] += v < A.vmin ? 1.0 : 0.0;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v);
        }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 3, true>(s, sh.red);
    block_reduce_multi<NT, 2, false>(x, sh.red);
    const int kcnt = (int)s[0];
    revs_net_summary_t r;
    const double nan = __builtin_nan("");
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.worst_value = nan;
    r.count = kcnt; r.n_fliers = 0; r.n_violations = (int)s[2]; r.n_nan = (int)s[1];
    r.worst_index = -1;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    revs_net_summary_t *out = A.out + (size_t)sc * A.T + t;
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    // ---- the selection; in its neighbour walk the worst node: the lowest caller-side index with the lowest voltage
    double wi[1] = {ninf};
    const BoxFigures b = box_select64(sh, kcnt, walk, [&](unsigned long long, bool ok, double v, int, int nd) {
        if (ok && -v == x[0]) wi[0] = fmax(wi[0], -(double)nd);
    });
    block_reduce_multi<NT, 1, false>(wi, sh.red);
    if (tid == 0) {
        r.min = -x[0]; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo; r.whisker_hi = b.whi;
        r.n_fliers = b.n_fliers;
        r.worst_value = -x[0]; r.worst_index = (int)-wi[0];
        *out = r;
    }
}

// ---- the day of one (scenario, node): over the slots whose voltage is no NaN the lowest and its earliest slot, the
// slots below vmin and those of them the linear model passes
__global__ void pf_node_day_kernel(const double *stage, const double *lin, const int32_t *nop, revs_pf_node_day_t *out,
                                   int S, int T, int n, int n_out, double vmin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * n) return;
    const int sc = idx / n, j = idx - sc * n;
    const int nd = nop ? nop[j] : j;
    if (nd < 0 || nd >= n_out) return;
    revs_pf_node_day_t r;
    r.volt_min = __builtin_nan(""); r.slot = -1; r.slots_below = 0; r.slots_missed = 0; r.reserved = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t at = ((int64_t)sc * T + t) * n + j;
        const double v = stage[at], vl = lin[at];
        if (v != v) continue;
        if (r.slot < 0 || v < r.volt_min) { r.volt_min = v; r.slot = t; }
        const bool below = v < vmin;
        r.slots_below += below ? 1 : 0;
        r.slots_missed += (below && !(vl < vmin)) ? 1 : 0;
    }
    out[(int64_t)sc * n_out + nd] = r;
}

// ---- the day of one scenario: the slot records walked in slot order by one thread
__global__ void pf_day_kernel(const revs_pf_slot_t *slot, const double *cost, revs_pf_day_t *out, int S, int T, double slot_hours) {
    const int sc = blockIdx.x * blockDim.x + threadIdx.x;
    if (sc >= S) return;
    const revs_pf_slot_t *s = slot + (size_t)sc * T;
    double e = 0.0, d = 0.0, co = 0.0;
    revs_pf_day_t r;
    r.volt_min = __builtin_nan(""); r.volt_min_slot = -1; r.volt_min_index = -1;
    r.n_below = r.n_below_lin = r.n_missed = r.iters_max = r.n_bad_slots = r.reserved = 0;
    for (int t = 0; t < T; ++t) {
        const double tot = s[t].loss_total;
        e = e + tot; d = d + s[t].delivered;
        if (cost) { const double pr = tot * cost[t]; co = co + pr; }
        if (s[t].volt_min_index >= 0 && (r.volt_min_slot < 0 || s[t].volt_min < r.volt_min)) {
            r.volt_min = s[t].volt_min; r.volt_min_slot = t; r.volt_min_index = s[t].volt_min_index;
        }
        r.n_below += s[t].n_below; r.n_below_lin += s[t].n_below_lin; r.n_missed += s[t].n_missed;
        r.iters_max = s[t].iters > r.iters_max ? s[t].iters : r.iters_max;
        r.n_bad_slots += s[t].status != 0 ? 1 : 0;
    }
    r.energy_lost = e * slot_hours; r.energy_delivered = d * slot_hours;
    r.cost = cost ? co * slot_hours : __builtin_nan("");
    out[sc] = r;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_powerflow_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (!net_scratch_sizes_ok(S, T, tree_n)) return 0;
    return 6 * (int64_t)S * T * tree_n * (int64_t)sizeof(double) + (int64_t)S * T * (int64_t)sizeof(revs_pf_slot_t);
}

extern "C" int revs_net_powerflow(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                                  const double *xw, double tan_phi, const uint8_t *node_mask, const int32_t *node_of_pos,
                                  int32_t n_out, double vset2, double vmin, double tol, int32_t max_iter, double slot_hours,
                                  const double *cost, double *volt_out, double *volt_lin_out, double *flow_out,
                                  double *loss_out, double *qflow_out, revs_net_summary_t *summary_out,
                                  revs_pf_slot_t *slot_out, revs_pf_node_day_t *node_day_out, revs_pf_day_t *day_out,
                                  void *scratch, void *stream) {
    static_assert(sizeof(revs_pf_slot_t) == 80 && sizeof(revs_pf_node_day_t) == 24 && sizeof(revs_pf_day_t) == 64, "");
    const char *who = "revs_net_powerflow";
    TreeArgs tr;
    int rc = net_tree_checks(who, S, m, T, tree, node_g, " node_g", n_out, &tr);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(vset2 - vset2 == 0.0 && vset2 > 0.0, "%s: vset2 must be finite and > 0", who);
    REVS_REQUIRE(slot_hours - slot_hours == 0.0 && slot_hours > 0.0, "%s: slot_hours must be finite and > 0", who);
    REVS_REQUIRE(tol - tol == 0.0 && tol > 0.0, "%s: tol must be finite and > 0", who);
    REVS_REQUIRE(vmin - vmin == 0.0, "%s: vmin must be finite", who);
    REVS_REQUIRE(max_iter >= 1 && max_iter <= REVS_PF_MAX_ITER, "%s: max_iter=%d outside 1..%d", who, (int)max_iter,
                 REVS_PF_MAX_ITER);
    REVS_REQUIRE(tan_phi - tan_phi == 0.0, "%s: tan_phi must be finite", who);
    REVS_REQUIRE(tan_phi == 0.0 || xw, "%s: tan_phi != 0 needs xw", who);
    REVS_REQUIRE(!xw || ((uintptr_t)xw & 15) == 0, "%s: xw must be 16-byte aligned", who);
    REVS_REQUIRE(!qflow_out || xw, "%s: qflow_out needs xw", who);
    REVS_REQUIRE(volt_out || volt_lin_out || flow_out || loss_out || qflow_out || summary_out || slot_out || node_day_out ||
                     day_out, "%s: every output is NULL", who);
    // (the state of the iteration lives in the scratch: every call needs it, a staged record or not)
    rc = net_scratch_checks(who, true, scratch, "the iteration's state and summary_out / node_day_out / day_out need",
                            "revs_net_powerflow_scratch");
    if (rc != REVS_OK) return rc;
    const size_t cells = (size_t)S * T * tr.n;
    double *base = (double *)scratch;
    PfArgs A;
    A.tr = tr;
    A.g = node_g; A.xw = xw; A.node_mask = node_mask; A.nop = node_of_pos;
    A.m = m; A.T = T; A.n_out = n_out; A.max_iter = max_iter; A.P = net_leaf_threads(tr.n);
    A.vset2 = vset2; A.vmin = vmin; A.thr = tol * vset2; A.tan_phi = tan_phi;
    A.volt = volt_out; A.volt_lin = volt_lin_out; A.flow = flow_out; A.loss = loss_out; A.qflow = qflow_out;
    A.sU = base; A.sVL = base + cells; A.sP = base + 2 * cells; A.sQ = base + 3 * cells; A.sLP = base + 4 * cells;
    A.sLQ = base + 5 * cells;
    revs_pf_slot_t *slot_scr = (revs_pf_slot_t *)(base + 6 * cells);
    A.slot = slot_out; A.slot_scr = day_out ? slot_scr : nullptr;
    rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        if (xw)
            return launch_lds(net_pf_kernel<nt(), ipt(), true>, dim3(T, S), dim3(nt()), pf_lds_bytes(tr.n), (hipStream_t)stream,
                              who, A);
        return launch_lds(net_pf_kernel<nt(), ipt(), false>, dim3(T, S), dim3(nt()), pf_lds_bytes(tr.n), (hipStream_t)stream,
                          who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out) {
        PfSumArgs P;
        P.stage = A.sU; P.mask = node_mask; P.nop = node_of_pos; P.out = summary_out;
        P.T = T; P.n = tr.n; P.n_out = n_out; P.vmin = vmin;
        hipLaunchKernelGGL(pf_summary_kernel, dim3(T, S), dim3(kPfSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (node_day_out) {
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(pf_node_day_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double *)A.sU, (const double *)A.sVL, node_of_pos, node_day_out, (int)S, (int)T, (int)tr.n,
                           (int)n_out, vmin);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        hipLaunchKernelGGL(pf_day_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                           (const revs_pf_slot_t *)slot_scr, cost, day_out, (int)S, (int)T, slot_hours);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
