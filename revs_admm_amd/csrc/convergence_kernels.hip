// The convergence report (include/revs_admm_ops.h, "convergence report"): the statistics of the
// residual history diff[k][i][s] -- what the reference's solve_ADMM returns besides the schedules and plot_convergence
// draws -- computed where the streaming launches leave it.
//
//   conv_iter_kernel   one workgroup per (row k, block of up to kConvSets scenarios): the box-plot record of every
//                      scenario's kept residuals of that row.  The workgroup reads the columns i S + s0 .. + ns - 1 of
//                      every residence i with adjacent threads on adjacent addresses (the whole row when S <= 8, 32-byte
//                      pieces beyond) and keeps everything per scenario in LDS: class counters, the digit histograms of
//                      a radix select over the floats' ordered keys (four 8-bit digits, three ranks), the keys of the
//                      extremes, neighbours and whiskers.  Integers all: LDS atomics, no order to depend on.  `total` is
//                      the one floating sum: every thread owns one column, adds its values in row order and the partial
//                      sums meet in a fixed tree.
//   conv_pool_kernel   the same selection over all columns of a row for up to kConvPoolSets groups per workgroup (a
//                      column's group from a table in LDS); total and the worst entry come from the members' records,
//                      in scenario order, so a pool of one scenario repeats that scenario's record byte for byte.
//   conv_res_kernel    one thread per column walks the K rows (adjacent threads, adjacent addresses): the per-residence
//                      record, and for kept residences an integer histogram of `settle` per scenario.
//   conv_final_kernel  one workgroup per scenario: the record over `settle` from that histogram (exact: the values are
//                      small integers), and the run's record from the maxima of the scenario's iteration records.
//
// The tie case.  The rows of a settled run are exact zeros for the most part.  Pass 0 counts negatives and zeros per set; a rank that falls
// among the zeros is settled there and takes no part in the digit passes, and a set none of whose ranks is open skips
// them altogether (a workgroup all of whose sets are settled runs pass 0, the neighbour / whisker / flier passes and
// nothing else).  Counts go to LDS once per distinct address of a wavefront, not once per lane.
#include "common.h"
#include "boxplot.h"

#include <math.h>

// Every product and sum of this file is rounded on its own, as numpy's: no contraction to fused multiply-adds.
#pragma clang fp contract(off)

namespace revs {

constexpr int kConvNT = 1024;                     // threads of a selection workgroup
constexpr int kConvSets = 8;                      // scenarios (or groups) one selection workgroup holds
constexpr int kConvMaskWords = REVS_STUDY_MAX_S / 64;

// classes of a kept value: the counters of a set
enum { kClsBad = 0, kClsNeg = 1, kClsZero = 2, kClsLow = 3, kClsAbove = 4, kClsN = 8 };

struct ConvShared {
    alignas(16) unsigned hist[kConvSets * 3 * 256];
    unsigned cls[kConvSets * kClsN];
    unsigned ans[kConvSets][3], left[kConvSets][3], eq[kConvSets][3], rank[kConvSets][3], rem4[kConvSets][3];
    unsigned open[kConvSets][3], slot[kConvSets][3], need[kConvSets][3];
    unsigned nb[kConvSets][3];                    // the smallest key above ans
    unsigned wk[kConvSets][2];                    // keys of the whiskers' candidates
    unsigned ext[kConvSets][2];                   // keys of min, max
    unsigned count[kConvSets], fl[kConvSets];
    int worst[kConvSets];
    double q[kConvSets][3], lim[kConvSets][2], w[kConvSets][2];
    double part[kConvNT];
    unsigned any_open, any_fl;
};

// The walk over the columns c0 .. c0 + nc - 1 of every residence of one row: thread t of the first NA = (NT / nc) nc
// takes element t, t + NA, ..: adjacent threads, adjacent addresses, and (nc <= NT) one column per thread throughout.
struct ConvWalk {
    const float *row;                             // hist + k ld
    const uint8_t *keep;                          // [S][n] or NULL
    const signed char *set_of;                    // LDS: the set of column c, -1: none; NULL: c - c0
    uint32_t n, S, c0, nc;
    double eps;

    // f(key, value, cls, set, i): cls -1: not part of any sample; kClsBad: kept and not finite; else finite
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        const uint32_t tid = threadIdx.x, total = n * nc;
        const uint32_t na = nc <= (uint32_t)kConvNT ? ((uint32_t)kConvNT / nc) * nc : (uint32_t)kConvNT;
        for (uint32_t jb = 0; jb < total; jb += na) {
            const uint32_t t = jb + tid;
            int cls = -1, set = 0;
            uint32_t i = 0;
            unsigned key = 0u;
            double v = 0.0;
            if (tid < na && t < total) {
                i = t / nc;
                const uint32_t c = c0 + (t - i * nc);
                const int sc = set_of ? (int)set_of[c] : (int)(c - c0);
                if (sc >= 0 && (!keep || keep[(size_t)c * n + i] != 0)) {
                    set = sc;
                    const unsigned u = __float_as_uint(row[(size_t)i * S + c]);
                    if ((u & 0x7F800000u) == 0x7F800000u) cls = kClsBad;
                    else {
                        key = box_key_f(u);
                        v = box_val_f(key);
                        cls = key < kBoxKey0F ? kClsNeg : key == kBoxKey0F ? kClsZero : v > eps ? kClsAbove : kClsLow;
                    }
                }
            }
            f(key, v, cls, set, i);
        }
    }
};

// The selection of `nsets` sets over the walk: on return thread ls < nsets finds in `sh` the counters (cls, count), the
// keys of min and max (ext), the quartiles (q), the whiskers (w) and the fliers (fl) of set ls.  hook0(value, cls, set,
// i) runs on every element of pass 0, hook1(key, cls, set, i) on every element of the neighbour pass (after ext is
// final).  Every thread of the workgroup calls it.
template <class H0, class H1>
__device__ __forceinline__ void conv_select(ConvShared &sh, const ConvWalk &W, int nsets, H0 hook0, H1 hook1) {
    constexpr int NT = kConvNT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kConvSets * 3 * 256; i += NT) sh.hist[i] = 0u;
    if (tid < kConvSets * kClsN) sh.cls[tid] = 0u;
    if (tid < kConvSets) {
        sh.ext[tid][0] = 0xFFFFFFFFu; sh.ext[tid][1] = 0u;
        sh.wk[tid][0] = 0xFFFFFFFFu; sh.wk[tid][1] = 0u;
        sh.fl[tid] = 0u; sh.worst[tid] = 0x7FFFFFFF;
        for (int e = 0; e < 3; ++e) sh.nb[tid][e] = 0xFFFFFFFFu;
    }
    if (tid == 0) { sh.any_open = 0u; sh.any_fl = 0u; }
    __syncthreads();
    // ---- pass 0: the classes' counts, the extremes, the top digit's histogram
    W.each([&](unsigned key, double v, int cls, int set, uint32_t i) {
        const bool ok = cls > kClsBad;
        conv_add(sh.cls, cls >= 0, (unsigned)(set * kClsN + (cls < 0 ? 0 : cls)));
        conv_add(sh.hist, ok, (unsigned)(set * 3 * 256) + (key >> 24));
        if (ok) {
            if (key < sh.ext[set][0]) atomicMin(&sh.ext[set][0], key);
            if (key > sh.ext[set][1]) atomicMax(&sh.ext[set][1], key);
        }
        hook0(v, cls, set, i);
    });
    __syncthreads();
    if (tid < nsets) {
        const unsigned *c = sh.cls + tid * kClsN;
        const unsigned nneg = c[kClsNeg], nzero = c[kClsZero], cnt = nneg + nzero + c[kClsLow] + c[kClsAbove];
        sh.count[tid] = cnt;
        for (int e = 0; e < 3; ++e) {
            unsigned r;
            box_rank(cnt, e + 1, r, sh.rem4[tid][e]);
            sh.rank[tid][e] = r; sh.left[tid][e] = r; sh.eq[tid][e] = 0u; sh.ans[tid][e] = 0u; sh.slot[tid][e] = 0u;
            const bool open = cnt && !box_settled_at_zero(r, nneg, nzero, sh.ans[tid][e], sh.left[tid][e], sh.eq[tid][e]);
            sh.open[tid][e] = open ? 1u : 0u;
            if (open) sh.any_open = 1u;
        }
    }
    __syncthreads();
    if (sh.any_open) {                            // (uniform)
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (pass > 0) {
                W.each([&](unsigned key, double, int cls, int set, uint32_t) {
                    const bool ok = cls > kClsBad;
                    const unsigned pk = key >> (shift + 8), d = (key >> shift) & 0xFFu;
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const bool on = ok && sh.open[set][e] && sh.slot[set][e] == (unsigned)e
                                        && pk == (sh.ans[set][e] >> (shift + 8));
                        conv_add(sh.hist, on, (unsigned)((set * 3 + e) * 256) + d);
                    }
                });
            }
            __syncthreads();
            // the bin that holds each open rank: a wavefront per (set, rank), four bins per lane, a prefix sum across lanes
            for (int task = wave; task < nsets * 3; task += NT / 64) {
                const int set = task / 3, e = task - 3 * set;
                if (!sh.open[set][e]) continue;   // (uniform in the wavefront)
                const unsigned *h = sh.hist + (set * 3 + (int)sh.slot[set][e]) * 256;
                unsigned bin, left, eq;
                pick_bin(*reinterpret_cast<const uint4 *>(h + 4 * lane), sh.left[set][e], bin, left, eq);
                if (lane == 0) { sh.ans[set][e] |= bin << shift; sh.left[set][e] = left; sh.eq[set][e] = eq; }
            }
            __syncthreads();
            if (pass < 3) {
                // open ranks whose prefixes agree share a histogram (the prefixes ascend with the ranks)
                if (tid < nsets) {
                    const unsigned *a = sh.ans[tid], *o = sh.open[tid];
                    const unsigned s1 = (o[0] && o[1] && a[1] == a[0]) ? 0u : 1u;
                    const unsigned s2 = (o[1] && o[2] && a[2] == a[1]) ? s1 : (o[0] && o[2] && a[2] == a[0]) ? 0u : 2u;
                    sh.slot[tid][0] = 0u; sh.slot[tid][1] = s1; sh.slot[tid][2] = s2;
                }
                for (int i = tid; i < kConvSets * 3 * 256; i += NT) sh.hist[i] = 0u;
                __syncthreads();
            }
        }
    }
    // ---- the upper neighbours: the smallest key above each rank's, where the next order statistic is another value
    if (tid < nsets) {
        const unsigned cnt = sh.count[tid];
        for (int e = 0; e < 3; ++e) {
            const unsigned r = sh.rank[tid][e], cle = r - sh.left[tid][e] + sh.eq[tid][e];      // values <= the statistic
            sh.need[tid][e] = (sh.rem4[tid][e] != 0u && box_next_differs(r, cnt, cle)) ? 1u : 0u;
        }
    }
    __syncthreads();
    W.each([&](unsigned key, double, int cls, int set, uint32_t i) {
        if (cls > kClsBad) {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (sh.need[set][e] && key > sh.ans[set][e] && key < sh.nb[set][e]) atomicMin(&sh.nb[set][e], key);
        }
        hook1(key, cls, set, i);
    });
    __syncthreads();
    if (tid < nsets && sh.count[tid]) {
        for (int e = 0; e < 3; ++e) {
            const double lo = box_val_f(sh.ans[tid][e]);
            const double hi = sh.need[tid][e] ? box_val_f(sh.nb[tid][e]) : lo;
            sh.q[tid][e] = box_quartile(lo, hi, sh.rem4[tid][e]);
        }
        box_limits(sh.q[tid][0], sh.q[tid][2], sh.lim[tid][0], sh.lim[tid][1]);
    }
    __syncthreads();
    // ---- whiskers and fliers
    W.each([&](unsigned key, double v, int cls, int set, uint32_t) {
        if (cls > kClsBad) {
            if (v >= sh.lim[set][0] && key < sh.wk[set][0]) atomicMin(&sh.wk[set][0], key);
            if (v <= sh.lim[set][1] && key > sh.wk[set][1]) atomicMax(&sh.wk[set][1], key);
        }
    });
    __syncthreads();
    if (tid < nsets && sh.count[tid]) {
        const double q1 = sh.q[tid][0], q3 = sh.q[tid][2];
        const unsigned k0 = sh.wk[tid][0], k1 = sh.wk[tid][1];
        const double wlo = box_whisker_lo(q1, k0 != 0xFFFFFFFFu, box_val_f(k0));
        const double whi = box_whisker_hi(q3, k1 != 0u, box_val_f(k1));
        sh.w[tid][0] = wlo; sh.w[tid][1] = whi;
        if (box_val_f(sh.ext[tid][0]) < wlo || box_val_f(sh.ext[tid][1]) > whi) sh.any_fl = 1u;
    }
    __syncthreads();
    if (sh.any_fl) {                              // (uniform)
        W.each([&](unsigned, double v, int cls, int set, uint32_t) {
            conv_add(sh.fl, cls > kClsBad && box_is_flier(v, sh.w[set][0], sh.w[set][1]), (unsigned)set);
        });
        __syncthreads();
    }
}

// the record of set ls from the selection's state, but for total and the worst entry
__device__ __forceinline__ revs_bill_summary_t conv_record(const ConvShared &sh, int ls) {
    const double nan = __builtin_nan("");
    revs_bill_summary_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.total = nan;
    r.reserved0 = 0.0;
    const unsigned *c = sh.cls + ls * kClsN;
    r.count = (int)sh.count[ls]; r.n_nan = (int)c[kClsBad]; r.n_fliers = 0; r.n_above = (int)c[kClsAbove];
    r.worst_index = r.worst_scenario = -1;
    if (r.count) {
        r.min = box_val_f(sh.ext[ls][0]); r.max = box_val_f(sh.ext[ls][1]);
        r.q1 = sh.q[ls][0]; r.median = sh.q[ls][1]; r.q3 = sh.q[ls][2];
        r.whisker_lo = sh.w[ls][0]; r.whisker_hi = sh.w[ls][1];
        r.n_fliers = (int)sh.fl[ls];
    }
    return r;
}

struct ConvIterArgs {
    const float *hist;
    const uint8_t *keep;
    const int32_t *index;
    revs_bill_summary_t *out;                     // [S][K]
    int64_t ld;
    double eps;
    uint32_t n, S, K;
};

__global__ __launch_bounds__(kConvNT) void conv_iter_kernel(ConvIterArgs A) {
    __shared__ ConvShared sh;
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x, s0 = blockIdx.y * kConvSets;
    const uint32_t nc = A.S - s0 < (uint32_t)kConvSets ? A.S - s0 : (uint32_t)kConvSets;
    ConvWalk W;
    W.row = A.hist + (int64_t)k * A.ld; W.keep = A.keep; W.set_of = nullptr;
    W.n = A.n; W.S = A.S; W.c0 = s0; W.nc = nc; W.eps = A.eps;
    double acc = 0.0;                             // this thread's column, rows ascending
    conv_select(sh, W, (int)nc,
        [&](double v, int cls, int, uint32_t) { if (cls > kClsBad) acc = acc + v; },
        [&](unsigned key, int cls, int set, uint32_t i) {
            if (cls > kClsBad && key == sh.ext[set][1]) {
                const int idx = A.index ? A.index[i] : (int)i;
                if (idx < sh.worst[set]) atomicMin(&sh.worst[set], idx);
            }
        });
    // total: the threads' partial sums of a column meet in a fixed tree
    const int per = kConvNT / (int)nc, na = per * (int)nc, jt = tid / (int)nc;
    sh.part[tid] = acc;
    __syncthreads();
    for (int h = kConvNT / 2; h >= 1; h >>= 1) {
        if (tid < na && jt < h && jt + h < per) sh.part[tid] = sh.part[tid] + sh.part[tid + h * (int)nc];
        __syncthreads();
    }
    if (tid < (int)nc) {
        revs_bill_summary_t r = conv_record(sh, tid);
        if (r.count) {
            r.total = sh.part[tid];
            r.worst_index = sh.worst[tid]; r.worst_scenario = (int)(s0 + tid);
        }
        A.out[(size_t)(s0 + tid) * A.K + k] = r;
    }
}

constexpr int kConvPoolSets = 4;                  // groups of one pool workgroup (their masks: 2 KB of arguments)
struct ConvPoolArgs {
    const float *hist;
    const uint8_t *keep;
    const revs_bill_summary_t *iter;              // [S][K]
    revs_bill_summary_t *out;                     // [G][K]
    int64_t ld;
    double eps;
    uint32_t n, S, K;
    int32_t g0, ng, words;
    unsigned long long member[kConvPoolSets][kConvMaskWords];     // bit s of a group's mask: scenario s
};

__global__ __launch_bounds__(kConvNT) void conv_pool_kernel(ConvPoolArgs A) {
    __shared__ ConvShared sh;
    __shared__ signed char set_of[REVS_STUDY_MAX_S];
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x;
    for (uint32_t s = tid; s < A.S; s += kConvNT) {
        int g = -1;
        for (int j = 0; j < A.ng; ++j)
            if ((A.member[j][s >> 6] >> (s & 63)) & 1ull) g = j;
        set_of[s] = (signed char)g;
    }
    __syncthreads();
    ConvWalk W;
    W.row = A.hist + (int64_t)k * A.ld; W.keep = A.keep; W.set_of = set_of;
    W.n = A.n; W.S = A.S; W.c0 = 0; W.nc = A.S; W.eps = A.eps;
    conv_select(sh, W, A.ng, [](double, int, int, uint32_t) {}, [](unsigned, int, int, uint32_t) {});
    if (tid < A.ng) {
        revs_bill_summary_t r = conv_record(sh, tid);
        if (r.count) {
            // total and the worst entry from the members' records, scenarios ascending: the largest value, then the
            // lowest scenario, then (the record's rule) the lowest index
            bool first = true;
            double best = 0.0;
            for (int w = 0; w < A.words; ++w) {
                unsigned long long mk = A.member[tid][w];
                while (mk) {
                    const int s = 64 * w + (int)__builtin_ctzll(mk);
                    mk &= mk - 1;
                    const revs_bill_summary_t m = A.iter[(size_t)s * A.K + k];
                    if (!m.count) continue;
                    r.total = first ? m.total : r.total + m.total;
                    if (first || m.max > best) { best = m.max; r.worst_index = m.worst_index; r.worst_scenario = s; }
                    first = false;
                }
            }
        }
        A.out[(size_t)(A.g0 + tid) * A.K + k] = r;
    }
}

struct ConvResArgs {
    const float *hist;
    const uint8_t *keep;
    const int32_t *index;
    revs_conv_res_t *out;                         // [S][n] or NULL
    int32_t *cnt;                                 // [S][K + 1]: kept residences by settle
    unsigned long long *code;                     // [S]: max of settle 2^32 + (2^31 - 1 - caller-side index)
    int64_t ld;
    double eps;
    uint32_t n, S, K;
};

__global__ __launch_bounds__(256) void conv_res_kernel(ConvResArgs A) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= A.n * A.S) return;
    const uint32_t i = c / A.S, s = c - i * A.S;
    const float *col = A.hist + c;
    float mx = 0.f, x = 0.f;
    int wi = -1, above = 0, lasta = -1;
    for (uint32_t k = 0; k < A.K; ++k) {
        x = col[(int64_t)k * A.ld];
        if (!((double)x <= A.eps)) { ++above; lasta = (int)k; }
        if (x == x && (wi < 0 || x > mx)) { mx = x; wi = (int)k; }
    }
    const int settle = lasta + 1;
    if (A.out) {
        revs_conv_res_t r;
        r.max = wi < 0 ? __builtin_nanf("") : mx + 0.f; r.last = x;
        r.settle = settle; r.n_above = above; r.worst_iteration = wi; r.reserved = 0;
        A.out[(size_t)s * A.n + i] = r;
    }
    if (A.cnt && (!A.keep || A.keep[(size_t)s * A.n + i] != 0)) {
        atomicAdd(A.cnt + (size_t)s * (A.K + 1) + settle, 1);
        const int idx = A.index ? A.index[i] : (int)i;
        atomicMax(A.code + s, (unsigned long long)settle << 32 | (unsigned)(0x7FFFFFFF - idx));
    }
}

struct ConvFinalArgs {
    const revs_bill_summary_t *iter;              // [S][K]
    const int32_t *cnt;                           // [S][K + 1] or NULL
    const unsigned long long *code;
    revs_conv_run_t *run;                         // [S] or NULL
    revs_bill_summary_t *settle;                  // [S] or NULL
    double eps;
    uint32_t K;
    int32_t patience, counts;                     // counts: run's n_unsettled / n_never come from cnt (else -1)
};

__global__ __launch_bounds__(256) void conv_final_kernel(ConvFinalArgs A) {
    constexpr int NT = 256;
    __shared__ int first_a[NT], last_a[NT], inner[NT];
    __shared__ unsigned csum[NT], coff[NT + 1];
    __shared__ unsigned long long tot;
    __shared__ int ex[2], wk[2], os[6], nfl;
    __shared__ double lim[2], wh[2], qv[3];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int K = (int)A.K;
    if (A.run) {
        // the rows above eps of this thread's stretch of rows: the first, the last, and the first start of `patience`
        // rows within eps between two of them
        const int chunk = (K + NT - 1) / NT, k0 = tid * chunk, k1 = min(k0 + chunk, K);
        int fa = -1, la = -1, in = -1;
        for (int k = k0; k < k1; ++k) {
            const double m = A.iter[(size_t)s * A.K + k].max;
            if (!(m <= A.eps)) {
                if (fa < 0) fa = k;
                else if (in < 0 && k - (la + 1) >= A.patience) in = la + 1;
                la = k;
            }
        }
        first_a[tid] = fa; last_a[tid] = la; inner[tid] = in;
        __syncthreads();
        if (tid == 0) {
            int prev = -1, conv = -1;
            bool done = false;
            for (int t = 0; t < NT && !done; ++t) {
                if (first_a[t] < 0) continue;
                if (first_a[t] - (prev + 1) >= A.patience) { conv = prev + 1; done = true; }
                else if (inner[t] >= 0) { conv = inner[t]; done = true; }
                prev = last_a[t];
            }
            if (!done) {
                if (K - (prev + 1) >= A.patience) conv = prev + 1;
            } else {
                for (int t = 0; t < NT; ++t) if (last_a[t] >= 0) prev = last_a[t];
            }
            revs_conv_run_t r;
            r.converged_at = conv; r.last_above = prev; r.n_unsettled = r.n_never = -1;
            if (A.counts) {
                r.n_unsettled = A.cnt[(size_t)s * (A.K + 1) + A.K]; r.n_never = A.cnt[(size_t)s * (A.K + 1)];
            }
            A.run[s] = r;
        }
    }
    if (!A.settle) return;                        // (uniform)
    // ---- the record over settle from its histogram: bins 0 .. K, a contiguous stretch per thread
    const int32_t *cnt = A.cnt + (size_t)s * (A.K + 1);
    const int nb = K + 1, chunk = (nb + NT - 1) / NT, b0 = min(tid * chunk, nb), b1 = min(b0 + chunk, nb);
    if (tid == 0) { tot = 0ull; ex[0] = 0x7FFFFFFF; ex[1] = -1; wk[0] = 0x7FFFFFFF; wk[1] = -1; nfl = 0; }
    __syncthreads();
    unsigned sum = 0u;
    unsigned long long vs = 0ull;
    int lo = 0x7FFFFFFF, hi = -1;
    for (int b = b0; b < b1; ++b) {
        const unsigned c = (unsigned)cnt[b];
        if (c) { sum += c; vs += (unsigned long long)c * (unsigned)b; lo = min(lo, b); hi = b; }
    }
    csum[tid] = sum;
    if (sum) { atomicAdd(&tot, vs); atomicMin(&ex[0], lo); atomicMax(&ex[1], hi); }
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0u;
        for (int t = 0; t < NT; ++t) { coff[t] = run; run += csum[t]; }
        coff[NT] = run;
    }
    __syncthreads();
    const unsigned N = coff[NT];
    const double nan = __builtin_nan("");
    revs_bill_summary_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.total = nan;
    r.reserved0 = 0.0;
    r.count = (int)N; r.n_nan = 0; r.n_fliers = 0; r.n_above = 0;
    r.worst_index = r.worst_scenario = -1;
    if (N == 0u) {                                // (uniform)
        if (tid == 0) A.settle[s] = r;
        return;
    }
    // the order statistics at the quartiles' lower ranks and the ranks above them
    unsigned rem4[3];
    for (int e = 0; e < 3; ++e) {
        unsigned rk[2];
        box_rank(N, e + 1, rk[0], rem4[e]);
        rk[1] = min(rk[0] + 1u, N - 1u);
        for (int j = 0; j < 2; ++j) {
            if (sum && rk[j] >= coff[tid] && rk[j] < coff[tid] + sum) {
                unsigned below = coff[tid];
                for (int b = b0; b < b1; ++b) {
                    below += (unsigned)cnt[b];
                    if (rk[j] < below) { os[2 * e + j] = b; break; }
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int e = 0; e < 3; ++e) qv[e] = box_quartile((double)os[2 * e], (double)os[2 * e + 1], rem4[e]);
        box_limits(qv[0], qv[2], lim[0], lim[1]);
    }
    __syncthreads();
    for (int b = b0; b < b1; ++b) {
        if (!cnt[b]) continue;
        if ((double)b >= lim[0]) atomicMin(&wk[0], b);
        if ((double)b <= lim[1]) atomicMax(&wk[1], b);
    }
    __syncthreads();
    if (tid == 0) {
        wh[0] = box_whisker_lo(qv[0], wk[0] != 0x7FFFFFFF, (double)wk[0]);
        wh[1] = box_whisker_hi(qv[2], wk[1] >= 0, (double)wk[1]);
    }
    __syncthreads();
    int f = 0;
    for (int b = b0; b < b1; ++b)
        if (box_is_flier((double)b, wh[0], wh[1])) f += cnt[b];
    if (f) atomicAdd(&nfl, f);
    __syncthreads();
    if (tid == 0) {
        r.min = (double)ex[0]; r.max = (double)ex[1];
        r.q1 = qv[0]; r.median = qv[1]; r.q3 = qv[2];
        r.whisker_lo = wh[0]; r.whisker_hi = wh[1];
        r.total = (double)tot;
        r.n_fliers = nfl; r.n_above = (int)N - cnt[0];
        r.worst_scenario = s;
        r.worst_index = 0x7FFFFFFF - (int)(unsigned)(A.code[s] & 0xFFFFFFFFull);
        A.settle[s] = r;
    }
}

}  // namespace revs

using namespace revs;

static bool conv_sizes_ok(int32_t S, int64_t n, int32_t K, int32_t G) {
    return study_sizes_ok(S, n) && K >= 1 && K < 0x7FFFFFFF && G >= 0 && G <= REVS_STUDY_MAX_S;
}

// the scratch: int32 cnt[S][K + 1], then uint64 code[S] (16-byte aligned)
static int64_t conv_cnt_bytes(int32_t S, int32_t K) { return (((int64_t)S * ((int64_t)K + 1) * 4 + 15) / 16) * 16; }

extern "C" int64_t revs_conv_report_scratch(int32_t S, int64_t n, int32_t K, int32_t G) {
    if (!conv_sizes_ok(S, n, K, G)) return 0;
    return conv_cnt_bytes(S, K) + (((int64_t)S * 8 + 15) / 16) * 16;
}

extern "C" int revs_conv_report(int32_t S, int64_t n, int32_t K, const float *hist, int64_t ld, const uint8_t *keep,
                                const int32_t *index, const int32_t *groups, int32_t G, double eps, int32_t patience,
                                revs_bill_summary_t *iter_rec, revs_bill_summary_t *pool_rec, revs_conv_res_t *res_rec,
                                revs_conv_run_t *run_rec, revs_bill_summary_t *settle_rec, void *scratch, void *stream) {
    static_assert(sizeof(revs_bill_summary_t) == 96 && sizeof(revs_conv_res_t) == 24 && sizeof(revs_conv_run_t) == 16, "");
    static_assert(sizeof(ConvPoolArgs) <= 4096, "kernel arguments");
    static_assert(sizeof(ConvShared) + REVS_STUDY_MAX_S <= 64 * 1024, "LDS");
    static_assert(kConvPoolSets <= kConvSets && kConvMaskWords * 64 == REVS_STUDY_MAX_S, "");
    const char *who = "revs_conv_report";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(K >= 1 && K < 0x7FFFFFFF, "%s: K=%d outside 1..2^31-2", who, (int)K);
    REVS_REQUIRE(study_sizes_ok(S, n), "%s: S*n columns, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(ld >= n * S, "%s: ld=%lld < n*S=%lld", who, (long long)ld, (long long)(n * S));
    REVS_REQUIRE(patience >= 1, "%s: patience=%d < 1", who, (int)patience);
    REVS_REQUIRE(eps >= 0.0, "%s: eps=%g is negative or a NaN", who, eps);
    REVS_REQUIRE(hist, "%s: null pointer argument hist", who);
    REVS_REQUIRE(iter_rec, "%s: null pointer argument iter_rec", who);
    REVS_REQUIRE(scratch, "%s: null pointer argument scratch (revs_conv_report_scratch bytes)", who);
    REVS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    REVS_REQUIRE(G >= 0 && G <= REVS_STUDY_MAX_S, "%s: G=%d outside 0..%d", who, (int)G, REVS_STUDY_MAX_S);
    REVS_REQUIRE(G == 0 || groups, "%s: groups is NULL with G > 0", who);
    REVS_REQUIRE(G == 0 || pool_rec, "%s: pool_rec is NULL with G > 0", who);
    for (int s = 0; s < S && G > 0; ++s)
        REVS_REQUIRE(groups[s] >= -1 && groups[s] < G, "%s: groups[%d]=%d outside -1..G-1", who, s, (int)groups[s]);

    hipStream_t st = (hipStream_t)stream;
    ConvIterArgs I;
    I.hist = hist; I.keep = keep; I.index = index; I.out = iter_rec; I.ld = ld; I.eps = eps;
    I.n = (uint32_t)n; I.S = (uint32_t)S; I.K = (uint32_t)K;
    // (rows along x: K < 2^31; scenario blocks along y: at most REVS_STUDY_MAX_S / 8)
    hipLaunchKernelGGL(conv_iter_kernel, dim3((unsigned)K, (unsigned)((S + kConvSets - 1) / kConvSets)), dim3(kConvNT), 0,
                       st, I);
    REVS_CHECK_LAUNCH(who);
    if (G > 0) {
        ConvPoolArgs P;
        P.hist = hist; P.keep = keep; P.iter = iter_rec; P.out = pool_rec; P.ld = ld; P.eps = eps;
        P.n = (uint32_t)n; P.S = (uint32_t)S; P.K = (uint32_t)K; P.words = (S + 63) / 64;
        for (int g0 = 0; g0 < G; g0 += kConvPoolSets) {
            const int ng = G - g0 < kConvPoolSets ? G - g0 : kConvPoolSets;
            for (int j = 0; j < kConvPoolSets; ++j)
                for (int w = 0; w < kConvMaskWords; ++w) P.member[j][w] = 0ull;
            for (int s = 0; s < S; ++s)
                if (groups[s] >= g0 && groups[s] < g0 + ng) P.member[groups[s] - g0][s / 64] |= 1ull << (s % 64);
            P.g0 = g0; P.ng = ng;
            hipLaunchKernelGGL(conv_pool_kernel, dim3((unsigned)K), dim3(kConvNT), 0, st, P);
            REVS_CHECK_LAUNCH(who);
        }
    }
    const bool walk = res_rec || settle_rec;
    int32_t *cnt = (int32_t *)scratch;
    unsigned long long *code = (unsigned long long *)((char *)scratch + conv_cnt_bytes(S, K));
    if (walk) {
        const bool hist_settle = settle_rec || run_rec;
        if (hist_settle) {
            if (hipMemsetAsync(scratch, 0, (size_t)revs_conv_report_scratch(S, n, K, G), st) != hipSuccess) {
                revs::set_error("%s: hipMemsetAsync failed", who);
                return REVS_ELAUNCH;
            }
        }
        ConvResArgs R;
        R.hist = hist; R.keep = keep; R.index = index; R.out = res_rec; R.cnt = hist_settle ? cnt : nullptr; R.code = code;
        R.ld = ld; R.eps = eps; R.n = (uint32_t)n; R.S = (uint32_t)S; R.K = (uint32_t)K;
        const int64_t cols = (int64_t)S * n;
        hipLaunchKernelGGL(conv_res_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, R);
        REVS_CHECK_LAUNCH(who);
    }
    if (run_rec || settle_rec) {
        ConvFinalArgs F;
        F.iter = iter_rec; F.cnt = walk ? cnt : nullptr; F.code = code; F.run = run_rec; F.settle = settle_rec;
        F.eps = eps; F.K = (uint32_t)K; F.patience = patience; F.counts = (run_rec && res_rec) ? 1 : 0;
        hipLaunchKernelGGL(conv_final_kernel, dim3((unsigned)S), dim3(256), 0, st, F);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
