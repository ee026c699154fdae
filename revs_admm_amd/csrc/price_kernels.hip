// The price report (include/revs_admm_ops.h, "price report"): what the multipliers y of the voltage
// rows say -- per node and slot the price a residence faces (energy, marginal loss, congestion), per line the multiplier
// Y of the flow through it and the congestion rent it collects, per slot and per day who pays what.  With
// R = sum_e w_e 1_sub(e) 1_sub(e)^T the congestion term d = R y is the network report's two scans on y, and
// g^T R y = sum_e w_e P_e Y_e splits the congestion payment into a rent per line.
//
//   revs_net_prices   net_prices_kernel<NT, IPT>, the four shapes of tree_shape(), on revs_net_study's T x S grid; then
//                     price_summary_kernel (one workgroup per (slot, scenario): box_select64 of boxplot.h over the staged
//                     prices), price_days_kernel (one thread per (scenario, position): the node's and the line's day) and
//                     price_day_kernel (one workgroup per scenario: the slot loops and the top 8 by repeated arg-max)
//
// One workgroup per (slot, scenario), four scans from net_scans.h's pieces (five with the marginal loss), one after the
// other on the same LDS:
//   1. the injections: net_gather of node_g, this thread's subtree of `delivered`, the flow and the drop scans of the
//      network report (the same bits); the flows are kept (PARK: in the scratch; else in registers);
//   2. with_loss: den = vset2 - drop and its test, c = (w flow) / den, mlf = net_path_scan(c) -- the loss report's bits --
//      and lossp = cost[t] mlf, kept likewise (else +0.0);
//   3. the multipliers: net_gather of node_y with its test, then the slot's one flag (__syncthreads_or; its barrier also
//      puts the last reads of step 2's scan in front of the next scan's writes); Y = the flow scan; rent = ((w Y) flow) s + 0.0
//      stored and staged at once, so the flows die here; d = the drop scan;
//   4. a chunk at a time cong = s d, price = (cost[t] + lossp) + cong, the injections gathered again (a chunk's: they were
//      not carried through four scans), the products inj lossp, inj cong, inj price, the stores and the staged values, this
//      thread's subtrees of the payments and its candidates for the largest and smallest price and the largest cong;
//   5. the fixed tree above the threads (losses_kernels.hip's), the three arg-max, the counts by LDS atomics, the record.
// Between a path scan and the flow scan behind it no barrier is added (risk_kernels.hip says why).
//
// LDS: the scans' buffer and wave totals (tree_lds_bytes) and, behind them, kPriceRedDoubles doubles for the reductions.
// The caller's scratch holds, by position, the staged price, rent, inj price and inj cong [S][T][n] each, the slot records
// [S][T] and the lines' day rents [S][n].
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"       // pair_tree, arg_better, wave_argmax
#include "net_scans.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

struct PriceArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const double *y;              // row multipliers double[S][m][T]
    const double *scale;          // [S], or NULL (1.0)
    const double *cost;           // [T]
    const uint8_t *line_mask;     // per position, or NULL (every line)
    const uint8_t *node_mask;     // per position, or NULL (every node)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t m, T, n_out, with_loss;
    int32_t P;                    // threads that hold leaves of the fixed tree: next_pow2(n) / IPT (at least 1)
    double vset2;
    double *price, *cong, *lossp, *line_y, *rent, *drop, *flow;      // [S][n_out][T], or NULL
    revs_price_slot_t *slot;      // [S][T], or NULL
    revs_price_slot_t *slot_scr;  // [S][T] in the scratch, or NULL
    double *stage_price, *stage_rent, *stage_pp, *stage_pc;          // [S][T][n] by position, or NULL (all or none)
};

constexpr int kPriceSums = 4;      // delivered, loss_pay, cong_pay, rent_total
constexpr int kPriceArgs = 3;      // price_max, -price_min, cong_max
// the sums' wave roots, the arg-max's values and indices, the two counts
constexpr int kPriceRedDoubles = kPriceSums * 16 + kPriceArgs * 16 + kPriceArgs * 8 + 2;

inline size_t price_lds_bytes(int n) { return (tree_lds_doubles_even(n) + kPriceRedDoubles) * sizeof(double); }

// (net_scans.h above is compiled as every tree report compiles it: flow, drop, Y and d keep the network report's bits.)
// Everything below rounds each operation on its own (the contract's IEEE operations): no product is fused into a sum.
#pragma clang fp contract(off)

// PARK: the caller gave the scratch, and the flows and lossp wait in stage_rent's and stage_pp's cells of this (slot,
// scenario) -- each thread's own positions, written behind the scan that made them and read back by the same thread in
// front of the rent and the product that overwrite them -- instead of in 2 IPT registers through the scans behind them.
// Without the scratch (arrays and slot records only) they are carried, and the 1024-thread shapes spill.
template <int NT, int IPT, bool PARK>
__global__ __launch_bounds__(NT) void net_prices_kernel(PriceArgs A0) {
    extern __shared__ double price_lds[];
    double *lds = price_lds;
    PriceArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y, lane = tid & 63, wave = tid >> 6;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T, cell = ((int64_t)sc * T + t) * n, rows = (int64_t)sc * A.m * T;
        A.g += rows; A.y += rows;
        if (A.price) A.price += arr;
        if (A.cong) A.cong += arr;
        if (A.lossp) A.lossp += arr;
        if (A.line_y) A.line_y += arr;
        if (A.rent) A.rent += arr;
        if (A.drop) A.drop += arr;
        if (A.flow) A.flow += arr;
        if (A.stage_price) { A.stage_price += cell; A.stage_rent += cell; A.stage_pp += cell; A.stage_pc += cell; }
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *sred = lds + net_lds_doubles<NT, IPT>();               // [kPriceSums][16]
    double *mred = sred + kPriceSums * 16;                          // [kPriceArgs][16]
    int *ired = reinterpret_cast<int *>(mred + kPriceArgs * 16);    // [kPriceArgs][16]
    int *cnt = ired + kPriceArgs * 16;                              // n_priced, n_rows
    const double nan = __builtin_nan("");
    const double s = A.scale ? A.scale[sc] : 1.0;
    const double ct = A.cost[t];
    if (tid == 0) {
        lds[1] = 0.0;                                               // base[-1]
        cnt[0] = cnt[1] = 0;
    }

    double a[IPT], f[PARK ? 2 : IPT], lp[PARK ? 2 : IPT];           // (!PARK) f: the flows, then the rents; lp: lossp
    double root[kPriceSums] = {0.0, 0.0, 0.0, 0.0};                 // this thread's subtree of each sum
    bool bad = !(s - s == 0.0 && s >= 0.0);
    // ---- 1. the injections: delivered, flow, drop
    {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, &bad);     // (A's fields, not locals: net_scans.h)
        root[0] = pair_tree<IPT>(a);
        net_flow_scan<NT, IPT>(act, lds, se, a);
    }
    NET_CHUNK_FENCE();
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        if (A.flow) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.flow[(int64_t)nd[i] * T + t] = a[c + i];
        }
        if constexpr (PARK) {
            if (act) {
#pragma unroll
                for (int i = 0; i < kNetChunk; i += 2)
                    *reinterpret_cast<TreeD2 *>(A.stage_rent + j0 + c + i) = TreeD2{{a[c + i], a[c + i + 1]}};
            }
        } else {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) f[c + i] = a[c + i];
        }
        NET_CHUNK_FENCE();
    }
    net_times_w<IPT>(tr, act, jl, a);
    net_path_scan<NT, IPT>(tr, act, jl, lds, a);
    // ---- 2. den and its test, c = (w flow) / den, lossp = cost mlf
    if (A.drop || A.with_loss) {                                    // (uniform)
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; i += 2) {
                const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + jl + c + i);
                TreeD2 fl = TreeD2{{0.0, 0.0}};
                if constexpr (PARK) {
                    if (act) fl = *reinterpret_cast<const TreeD2 *>(A.stage_rent + j0 + c + i);
                } else {
                    fl = TreeD2{{f[PARK ? 0 : c + i], f[PARK ? 1 : c + i + 1]}};
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (A.drop && nd[i + e] >= 0) A.drop[(int64_t)nd[i + e] * T + t] = a[c + i + e];
                    const double den = A.vset2 - a[c + i + e];
                    bad |= A.with_loss && nd[i + e] >= 0 && !(den > 0.0);
                    const double wf = wv.v[e] * fl.v[e];
                    a[c + i + e] = act ? wf / den : 0.0;
                }
            }
            NET_CHUNK_FENCE();
        }
    }
    if (A.with_loss) {                                              // (uniform)
        __syncthreads();                                            // (every read of the drop scan's F is done)
        net_path_scan<NT, IPT>(tr, act, jl, lds, a);
#pragma unroll
        for (int i = 0; i < IPT; ++i) a[i] = ct * a[i];
    } else {
#pragma unroll
        for (int i = 0; i < IPT; ++i) a[i] = 0.0;
    }
    if constexpr (PARK) {
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeD2 *>(A.stage_pp + j0 + i) = TreeD2{{a[i], a[i + 1]}};
        }
    } else {
#pragma unroll
        for (int i = 0; i < IPT; ++i) lp[i] = a[i];
    }
    NET_CHUNK_FENCE();
    // ---- 3. the multipliers: the slot's flag, Y, the rents, d
    int n_rows = 0;
    bool badslot;
    {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.y, A.m, A.T, t, act, se, a, &bad);
#pragma unroll
        for (int i = 0; i < IPT; ++i) n_rows += a[i] != 0.0 ? 1 : 0;
        badslot = __syncthreads_or(bad ? 1 : 0) != 0;               // (its barrier: every read of the last scan's F is done)
        net_flow_scan<NT, IPT>(act, lds, se, a);
    }
    NET_CHUNK_FENCE();
    double half[IPT / kNetChunk];
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long lm = net_load_bytes(A.line_mask, jl + c);
        if (A.line_y) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.line_y[(int64_t)nd[i] * T + t] = a[c + i];
        }
        net_times_w_chunk<IPT>(tr, act, jl, c, a);                  // w Y: the drop scan's terms
        double leaf[kNetChunk];
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 2) {
            TreeD2 fl = TreeD2{{0.0, 0.0}};
            if constexpr (PARK) {
                if (act) fl = *reinterpret_cast<const TreeD2 *>(A.stage_rent + j0 + c + i);
            } else {
                fl = TreeD2{{f[PARK ? 0 : c + i], f[PARK ? 1 : c + i + 1]}};
            }
            double x[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int k = i + e;
                const double wyf = a[c + k] * fl.v[e];
                const double r = wyf * s + 0.0;                     // (a zero rent is +0.0 whatever the flow's sign)
                x[e] = badslot ? nan : r;
                const bool summed = nd[k] >= 0 && ((lm >> (8 * k)) & 0xFFull) != 0ull;
                leaf[k] = summed ? r : 0.0;
                if (A.rent && nd[k] >= 0) A.rent[(int64_t)nd[k] * T + t] = x[e];
            }
            if (A.stage_rent && act) *reinterpret_cast<TreeD2 *>(A.stage_rent + j0 + c + i) = TreeD2{{x[0], x[1]}};
        }
        half[c / kNetChunk] = pair_tree<kNetChunk>(leaf);
        NET_CHUNK_FENCE();
    }
    if constexpr (IPT == kNetChunk) root[3] = half[0];
    else root[3] = half[0] + half[IPT / kNetChunk - 1];
    net_path_scan<NT, IPT>(tr, act, jl, lds, a);
    // ---- 4. cong, price, the payments; the stores; the candidates
    double bv[kPriceArgs] = {0.0, 0.0, 0.0};
    int bi[kPriceArgs] = {-1, -1, -1};
    int n_priced = 0;
    double hl[IPT / kNetChunk], hc[IPT / kNetChunk];
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long nm = net_load_bytes(A.node_mask, jl + c);
        unsigned se[kNetChunk];
        double inj[kNetChunk], ll[kNetChunk], lc[kNetChunk];
        net_load_se<kNetChunk>(tr, jl + c, se);
        net_gather<kNetChunk>(A.g, A.m, A.T, t, act, se, inj, nullptr);
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 2) {
            double xp[2], xpp[2], xpc[2];
            TreeD2 parked = TreeD2{{0.0, 0.0}};
            if constexpr (PARK) {
                if (act) parked = *reinterpret_cast<const TreeD2 *>(A.stage_pp + j0 + c + i);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int k = i + e;
                const double lpk = PARK ? parked.v[e] : lp[PARK ? 0 : c + k];
                const double cg = s * a[c + k];
                const double en = ct + lpk;
                const double pr = en + cg;
                const double pl = inj[k] * lpk;
                const double pc = inj[k] * cg;
                const double pp = inj[k] * pr;
                const bool masked = nd[k] >= 0 && ((nm >> (8 * k)) & 0xFFull) != 0ull;
                ll[k] = masked ? pl : 0.0;
                lc[k] = masked ? pc : 0.0;
                xp[e] = badslot ? nan : pr; xpp[e] = badslot ? nan : pp; xpc[e] = badslot ? nan : pc;
                if (masked && !badslot) {
                    n_priced += cg != 0.0 ? 1 : 0;
                    if (pr == pr) { arg_better(bv[0], bi[0], pr, nd[k]); arg_better(bv[1], bi[1], -pr, nd[k]); }
                    if (cg == cg) arg_better(bv[2], bi[2], cg, nd[k]);
                }
                if (nd[k] >= 0) {
                    const int64_t at = (int64_t)nd[k] * T + t;
                    if (A.price) A.price[at] = xp[e];
                    if (A.cong) A.cong[at] = badslot ? nan : cg;
                    if (A.lossp) A.lossp[at] = badslot ? nan : lpk;
                }
            }
            if (A.stage_price && act) {
                *reinterpret_cast<TreeD2 *>(A.stage_price + j0 + c + i) = TreeD2{{xp[0], xp[1]}};
                *reinterpret_cast<TreeD2 *>(A.stage_pp + j0 + c + i) = TreeD2{{xpp[0], xpp[1]}};
                *reinterpret_cast<TreeD2 *>(A.stage_pc + j0 + c + i) = TreeD2{{xpc[0], xpc[1]}};
            }
        }
        hl[c / kNetChunk] = pair_tree<kNetChunk>(ll);
        hc[c / kNetChunk] = pair_tree<kNetChunk>(lc);
        NET_CHUNK_FENCE();
    }
    if (!A.slot && !A.slot_scr) return;                             // (uniform)
    if constexpr (IPT == kNetChunk) { root[1] = hl[0]; root[2] = hc[0]; }
    else { root[1] = hl[0] + hl[IPT / kNetChunk - 1]; root[2] = hc[0] + hc[IPT / kNetChunk - 1]; }
    // ---- 5. the fixed tree above the threads: lanes by an xor butterfly, then the wavefronts' roots level by level
    const int P = A.P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if (o < P) {                                                // (uniform)
#pragma unroll
            for (int q = 0; q < kPriceSums; ++q) root[q] += __shfl_xor(root[q], o);
        }
        n_priced += __shfl_xor(n_priced, o); n_rows += __shfl_xor(n_rows, o);
    }
#pragma unroll
    for (int q = 0; q < kPriceArgs; ++q) wave_argmax(bv[q], bi[q]);
    const int W = P > 64 ? P / 64 : 1;
    if (lane == 0) {
        if (wave < W) {
#pragma unroll
            for (int q = 0; q < kPriceSums; ++q) sred[q * 16 + wave] = root[q];
        }
#pragma unroll
        for (int q = 0; q < kPriceArgs; ++q) { mred[q * 16 + wave] = bv[q]; ired[q * 16 + wave] = bi[q]; }
        if (n_priced) atomicAdd(cnt + 0, n_priced);
        if (n_rows) atomicAdd(cnt + 1, n_rows);
    }
    __syncthreads();
    if (tid < kPriceSums) {
        double *r = sred + tid * 16;
        for (int w = W; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    } else if (tid >= 64 && tid < 64 + kPriceArgs) {
        const int q = tid - 64;
        double v = mred[q * 16];
        int ix = ired[q * 16];
        for (int w = 1; w < NT / 64; ++w) arg_better(v, ix, mred[q * 16 + w], ired[q * 16 + w]);
        mred[q * 16] = v; ired[q * 16] = ix;
    }
    __syncthreads();
    if (tid == 0) {
        revs_price_slot_t r;
        const double dl = sred[0];
        const double ep = ct * dl;
        r.delivered = badslot ? nan : dl;
        r.energy_pay = badslot ? nan : ep;
        r.loss_pay = badslot ? nan : sred[16];
        r.cong_pay = badslot ? nan : sred[32];
        r.rent_total = badslot ? nan : sred[48];
        r.price_max_index = ired[0]; r.price_min_index = ired[16]; r.cong_max_index = ired[32];
        r.price_max = ired[0] >= 0 ? mred[0] : nan;
        r.price_min = ired[16] >= 0 ? -mred[16] : nan;
        r.cong_max = ired[32] >= 0 ? mred[32] : nan;
        r.n_priced = badslot ? 0 : cnt[0];
        r.n_rows = badslot ? 0 : cnt[1];
        r.n_bad = badslot ? 1 : 0;
        r.reserved[0] = r.reserved[1] = 0;
        if (A.slot) A.slot[(size_t)sc * T + t] = r;
        if (A.slot_scr) A.slot_scr[(size_t)sc * T + t] = r;
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged prices over the nodes with node_mask
constexpr int kPriceSumNT = 256;
struct PriceSumArgs {
    const double *stage;          // [S][T][n]
    const uint8_t *mask;          // node_mask per position, or NULL
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T]
    int32_t T, n, n_out;
    double price_cap;
};

__global__ __launch_bounds__(kPriceSumNT) void price_summary_kernel(PriceSumArgs A) {
    __shared__ BoxSelect<kPriceSumNT> sh;
    constexpr int NT = kPriceSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf();
    // box_select64's walk: an element is part of the sample when it is summarised and no NaN
    auto walk = [&](auto f) {
        net_for_each<NT>(row, A.n, A.nop, A.n_out, A.mask, [&](double v, int nd, int) { f(box_key(v), nd >= 0 && v == v, v, 0, nd); });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, above price_cap
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        if (ok) {
            s[2] += v > A.price_cap ? 1.0 : 0.0;
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
    // ---- the selection; in its neighbour walk the worst node: the lowest caller-side index with the largest price
    double wi[1] = {ninf};
    const BoxFigures b = box_select64(sh, kcnt, walk, [&](unsigned long long, bool ok, double v, int, int nd) {
        if (ok && v == x[1]) wi[0] = fmax(wi[0], -(double)nd);
    });
    block_reduce_multi<NT, 1, false>(wi, sh.red);
    if (tid == 0) {
        r.min = -x[0]; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo; r.whisker_hi = b.whi;
        r.n_fliers = b.n_fliers;
        r.worst_value = x[1]; r.worst_index = (int)-wi[0];
        *out = r;
    }
}

// ---- the day of one (scenario, position): the node's payments and peak price, the line's rent (the loss report's line
// rule on the rents), and the day rent by position into the scratch for the day kernel's top 8
struct PriceDaysArgs {
    const double *stage_price, *stage_rent, *stage_pp, *stage_pc;   // [S][T][n]
    const int32_t *nop;
    revs_price_node_day_t *node_out;  // [S][n_out], or NULL
    revs_loss_line_day_t *line_out;   // [S][n_out], or NULL
    double *rent_scr;                 // [S][n]
    int32_t S, T, n, n_out;
    double slot_hours;
};

__global__ void price_days_kernel(PriceDaysArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.S * A.n) return;
    const int sc = idx / A.n, j = idx - sc * A.n;
    double paid = 0.0, cpaid = 0.0, rsum = 0.0, ppeak = 0.0, rpeak = 0.0;
    int pat = -1, rat = -1;
    bool pnan = false, rnan = false;
    for (int t = 0; t < A.T; ++t) {
        const int64_t at = ((int64_t)sc * A.T + t) * A.n + j;
        const double pr = A.stage_price[at], rn = A.stage_rent[at];
        paid = paid + A.stage_pp[at];
        cpaid = cpaid + A.stage_pc[at];
        rsum = rsum + rn;
        pnan |= pr != pr; rnan |= rn != rn;
        if (pat < 0 || pr > ppeak) { ppeak = pr; pat = t; }
        if (rat < 0 || rn > rpeak) { rpeak = rn; rat = t; }
    }
    const double nan = __builtin_nan("");
    revs_price_node_day_t nr;
    nr.paid = paid * A.slot_hours;
    nr.cong_paid = cpaid * A.slot_hours;
    nr.peak_price = pnan ? nan : ppeak;
    nr.peak_slot = pnan ? -1 : pat;
    nr.reserved = 0;
    revs_loss_line_day_t lr;
    lr.energy = rsum * A.slot_hours;
    lr.peak = rnan ? nan : rpeak;
    lr.peak_slot = rnan ? -1 : rat;
    lr.reserved = 0;
    A.rent_scr[(int64_t)sc * A.n + j] = lr.energy;
    const int nd = A.nop ? A.nop[j] : j;
    if (nd >= 0 && nd < A.n_out) {
        if (A.node_out) A.node_out[(int64_t)sc * A.n_out + nd] = nr;
        if (A.line_out) A.line_out[(int64_t)sc * A.n_out + nd] = lr;
    }
}

// ---- the day of one scenario: the slot records summed in slot order by one thread, then the eight summarised lines of
// largest day rent by eight arg-max rounds, each over the lines after the last pick in (rent down, index up) order
constexpr int kPriceDayNT = 256;
struct PriceDayArgs {
    const revs_price_slot_t *slot;  // [S][T]
    const double *rent;             // [S][n] by position
    const uint8_t *mask;            // line_mask per position, or NULL
    const int32_t *nop;
    revs_price_day_t *out;          // [S]
    int32_t T, n, n_out;
    double slot_hours;
};

__global__ __launch_bounds__(kPriceDayNT) void price_day_kernel(PriceDayArgs A) {
    __shared__ double mv[kPriceDayNT / 64];
    __shared__ int mi[kPriceDayNT / 64];
    __shared__ revs_price_day_t rec;
    const int tid = threadIdx.x, sc = (int)blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nan = __builtin_nan("");
    if (tid == 0) {
        const revs_price_slot_t *s = A.slot + (size_t)sc * A.T;
        double e = 0.0, l = 0.0, c = 0.0, r = 0.0, peak = 0.0;
        int at = -1, ix = -1, nbad = 0, ncong = 0;
        for (int t = 0; t < A.T; ++t) {
            e = e + s[t].energy_pay; l = l + s[t].loss_pay; c = c + s[t].cong_pay; r = r + s[t].rent_total;
            if (s[t].price_max_index >= 0 && (at < 0 || s[t].price_max > peak)) {
                peak = s[t].price_max; at = t; ix = s[t].price_max_index;
            }
            nbad += s[t].n_bad;
            ncong += s[t].n_rows > 0 ? 1 : 0;
        }
        rec.energy_pay = e * A.slot_hours; rec.loss_pay = l * A.slot_hours;
        rec.cong_pay = c * A.slot_hours; rec.rent_total = r * A.slot_hours;
        const bool none = nbad != 0 || at < 0;
        rec.peak_price = none ? nan : peak; rec.peak_slot = none ? -1 : at; rec.peak_index = none ? -1 : ix;
        rec.n_bad_slots = nbad; rec.n_cong_slots = ncong;
        rec.reserved[0] = rec.reserved[1] = 0;
    }
    const double *en = A.rent + (size_t)sc * A.n;
    double pv = __builtin_inf();
    int pi = -1;                                   // the last pick: everything is after (+inf, -1)
    for (int k = 0; k < 8; ++k) {
        double bv = 0.0;
        int bi = -1;
        for (int j = tid; j < A.n; j += kPriceDayNT) {
            int nd = A.nop ? A.nop[j] : j;
            nd = (nd >= 0 && nd < A.n_out && (!A.mask || A.mask[j] != 0)) ? nd : -1;
            const double v = en[j];
            if (nd >= 0 && v == v && (v < pv || (v == pv && nd > pi))) arg_better(bv, bi, v, nd);
        }
        wave_argmax(bv, bi);
        if (lane == 0) { mv[wave] = bv; mi[wave] = bi; }
        __syncthreads();
        bv = mv[0]; bi = mi[0];
        for (int w = 1; w < kPriceDayNT / 64; ++w) arg_better(bv, bi, mv[w], mi[w]);
        __syncthreads();                           // (every read of mv / mi is done)
        if (tid == 0) { rec.top_index[k] = bi; rec.top_rent[k] = bi >= 0 ? bv : nan; }
        if (bi >= 0) { pv = bv; pi = bi; }
        else { pv = -__builtin_inf(); pi = 0x7FFFFFFF; }       // (uniform) nothing is left
    }
    if (tid == 0) A.out[sc] = rec;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_prices_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (!net_scratch_sizes_ok(S, T, tree_n)) return 0;
    return (int64_t)S * T * tree_n * 4 * (int64_t)sizeof(double) + (int64_t)S * T * (int64_t)sizeof(revs_price_slot_t) +
           (int64_t)S * tree_n * (int64_t)sizeof(double);
}

extern "C" int revs_net_prices(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                               const double *node_y, const double *scale, const double *cost, const uint8_t *line_mask,
                               const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out, double vset2,
                               int32_t with_loss, double slot_hours, double price_cap, double *price_out, double *cong_out,
                               double *lossp_out, double *line_y_out, double *rent_out, double *drop_out, double *flow_out,
                               revs_net_summary_t *summary_out, revs_price_slot_t *slot_out,
                               revs_price_node_day_t *node_day_out, revs_loss_line_day_t *line_day_out,
                               revs_price_day_t *day_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_price_slot_t) == 96 && sizeof(revs_price_node_day_t) == 32 && sizeof(revs_price_day_t) == 160, "");
    const char *who = "revs_net_prices";
    TreeArgs tr;
    int rc = net_tree_checks(who, S, m, T, tree, node_g, " node_g", n_out, &tr);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(node_y, "%s: null pointer argument node_y", who);
    REVS_REQUIRE(cost, "%s: null pointer argument cost", who);
    REVS_REQUIRE(!with_loss || (vset2 - vset2 == 0.0 && vset2 > 0.0), "%s: vset2 must be finite and > 0 with with_loss", who);
    REVS_REQUIRE(slot_hours - slot_hours == 0.0 && slot_hours > 0.0, "%s: slot_hours must be finite and > 0", who);
    REVS_REQUIRE(price_cap == price_cap, "%s: price_cap is a NaN", who);
    REVS_REQUIRE(price_out || cong_out || lossp_out || line_y_out || rent_out || drop_out || flow_out || summary_out ||
                 slot_out || node_day_out || line_day_out || day_out, "%s: every output is NULL", who);
    const bool staged = summary_out || node_day_out || line_day_out || day_out;
    rc = net_scratch_checks(who, staged, scratch, "summary_out / node_day_out / line_day_out / day_out need",
                            "revs_net_prices_scratch");
    if (rc != REVS_OK) return rc;
    const size_t cells = (size_t)S * T * tr.n;
    double *stage = staged ? (double *)scratch : nullptr;
    revs_price_slot_t *slot_scr = staged ? (revs_price_slot_t *)(stage + 4 * cells) : nullptr;
    double *rent_scr = staged ? (double *)(slot_scr + (size_t)S * T) : nullptr;
    PriceArgs A;
    A.tr = tr;
    A.g = node_g; A.y = node_y; A.scale = scale; A.cost = cost;
    A.line_mask = line_mask; A.node_mask = node_mask; A.nop = node_of_pos;
    A.m = m; A.T = T; A.n_out = n_out; A.with_loss = with_loss ? 1 : 0; A.P = net_leaf_threads(tr.n);
    A.vset2 = vset2;
    A.price = price_out; A.cong = cong_out; A.lossp = lossp_out; A.line_y = line_y_out; A.rent = rent_out;
    A.drop = drop_out; A.flow = flow_out;
    A.slot = slot_out; A.slot_scr = day_out ? slot_scr : nullptr;
    A.stage_price = stage;
    A.stage_rent = staged ? stage + cells : nullptr;
    A.stage_pp = staged ? stage + 2 * cells : nullptr;
    A.stage_pc = staged ? stage + 3 * cells : nullptr;
    rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        if (staged)
            return launch_lds(net_prices_kernel<nt(), ipt(), true>, dim3(T, S), dim3(nt()), price_lds_bytes(tr.n),
                              (hipStream_t)stream, who, A);
        return launch_lds(net_prices_kernel<nt(), ipt(), false>, dim3(T, S), dim3(nt()), price_lds_bytes(tr.n),
                          (hipStream_t)stream, who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out) {
        PriceSumArgs P;
        P.stage = A.stage_price; P.mask = node_mask; P.nop = node_of_pos; P.out = summary_out;
        P.T = T; P.n = tr.n; P.n_out = n_out; P.price_cap = price_cap;
        hipLaunchKernelGGL(price_summary_kernel, dim3(T, S), dim3(kPriceSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (node_day_out || line_day_out || day_out) {
        PriceDaysArgs D;
        D.stage_price = A.stage_price; D.stage_rent = A.stage_rent; D.stage_pp = A.stage_pp; D.stage_pc = A.stage_pc;
        D.nop = node_of_pos; D.node_out = node_day_out; D.line_out = line_day_out; D.rent_scr = rent_scr;
        D.S = S; D.T = T; D.n = tr.n; D.n_out = n_out; D.slot_hours = slot_hours;
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(price_days_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, D);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        PriceDayArgs D;
        D.slot = slot_scr; D.rent = rent_scr; D.mask = line_mask; D.nop = node_of_pos; D.out = day_out;
        D.T = T; D.n = tr.n; D.n_out = n_out; D.slot_hours = slot_hours;
        hipLaunchKernelGGL(price_day_kernel, dim3(S), dim3(kPriceDayNT), 0, (hipStream_t)stream, D);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
