// The bill report (include/revs_admm_ops.h, "bill report"): what a schedule costs each
// residence under the tariff, its deviation from a baseline schedule, and the box-plot records of both per scenario
// and pooled over the scenarios of a group.
//
//   bill_rows_kernel<TG>   bill[s][i] = sum_t tariff[t] (double) g[s][i][t].  A workgroup owns 256 rows and walks the
//                          slots in chunks: the chunk of every row is staged in LDS by loads that run along the rows
//                          (a wavefront reads whole 128-byte pieces of two or four rows), then thread r adds row r's
//                          chunk to its ONE accumulator in slot order.  The LDS row stride is the chunk plus one
//                          element: thread r reads word 33 r + t (float) or doubles at 17 r + t, which spreads the 32
//                          lanes of a half wavefront over all banks.  Which thread holds a row changes nothing in its
//                          arithmetic: the bits are those of the sequential loop.
//   bill_dev_kernel        dev[s][i] = (100 (bill[s][i] - bill[b][i])) / bill[b][i]; the scenarios' baselines travel
//                          in the kernel arguments, kBillBaseMax scenarios per launch
//   bill_select_kernel     one workgroup per (member set, quantity): net_pool_kernel's digit-wise radix select
//                          (network_kernels.hip) over signed doubles under across_kernels.hip's ordered keys, reading
//                          the values themselves (bill / dev, double[S][n]) under the keep mask.  A member set is one
//                          scenario (the summaries) or a group's bit mask from the kernel arguments (the pools); both
//                          walk a scenario's row with the same thread for the same element, so a pool of one scenario
//                          repeats that scenario's record bit for bit, `total` included.
#include "common.h"

#include <math.h>

// Every product and sum below is rounded on its own, as numpy's: no contraction to fused multiply-adds anywhere in this
// file.  (The rounding intrinsics of the HIP headers, _rn, are plain operators compiled under the headers' own contraction
// setting: a product and a sum from them still fuse after inlining.  The operators of this file, under this pragma, do not.)
#pragma clang fp contract(off)

namespace revs {

__device__ __forceinline__ double bill_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double bill_add(double a, double b) { return a + b; }
__device__ __forceinline__ double bill_sub(double a, double b) { return a - b; }

constexpr int kBillNT = 256;                      // rows of a tile: one thread each
template <typename TG> struct BillChunk { static constexpr int value = sizeof(TG) == 4 ? 32 : 16; };   // 128 bytes of a row

struct BillRowsArgs {
    const void *g;
    const double *tariff;
    double *bill;
    int64_t stride_s, stride_i;
    uint32_t n, S, rows;                          // rows = S n < 2^31
    int32_t T, inner_i;                           // inner_i: rows are taken in the order s n + i (else i S + s)
};

// the row a thread owns: its offset in g and in bill (-1: past the end)
__device__ __forceinline__ void bill_row_of(const BillRowsArgs &A, uint32_t mr, int64_t &off, int64_t &out) {
    off = out = -1;
    if (mr >= A.rows) return;
    uint32_t s, i;
    if (A.inner_i) { s = mr / A.n; i = mr - s * A.n; }
    else           { i = mr / A.S; s = mr - i * A.S; }
    off = (int64_t)s * A.stride_s + (int64_t)i * A.stride_i;
    out = (int64_t)s * A.n + i;
}

#ifndef REVS_BILL_ROWS_DIRECT
template <typename TG>
__global__ __launch_bounds__(kBillNT) void bill_rows_kernel(BillRowsArgs A) {
    constexpr int TC = BillChunk<TG>::value, LD = TC + 1;
    __shared__ TG tile[kBillNT * LD];
    __shared__ int64_t rowoff[kBillNT];
    const int tid = threadIdx.x;
    int64_t off, out;
    bill_row_of(A, (uint32_t)blockIdx.x * kBillNT + (uint32_t)tid, off, out);
    rowoff[tid] = off;
    const TG *g = (const TG *)A.g;
    double acc = 0.0;
    for (int c0 = 0; c0 < A.T; c0 += TC) {
        __syncthreads();                          // (rowoff is visible; the chunk before is read)
#pragma unroll
        for (int k = 0; k < TC; ++k) {            // element e of the tile's chunk: row e / TC, slot c0 + e % TC
            const int e = k * kBillNT + tid, r = e / TC, t = e % TC;
            const int64_t ro = rowoff[r];
            TG x = (TG)0;
            if (ro >= 0 && c0 + t < A.T) x = g[ro + c0 + t];
            tile[r * LD + t] = x;
        }
        __syncthreads();
        const int tc = A.T - c0 < TC ? A.T - c0 : TC;
        const TG *row = tile + tid * LD;
        for (int t = 0; t < tc; ++t) acc = bill_add(acc, bill_mul(A.tariff[c0 + t], (double)row[t]));
    }
    if (out >= 0) A.bill[out] = acc;
}
#else
// the other mapping (a tuning build: tools/bill_times.py): every thread reads its own row, the caches do the rest
template <typename TG>
__global__ __launch_bounds__(kBillNT) void bill_rows_kernel(BillRowsArgs A) {
    int64_t off, out;
    bill_row_of(A, (uint32_t)blockIdx.x * kBillNT + (uint32_t)threadIdx.x, off, out);
    if (out < 0) return;
    const TG *row = (const TG *)A.g + off;
    double acc = 0.0;
    for (int t = 0; t < A.T; ++t) acc = bill_add(acc, bill_mul(A.tariff[t], (double)row[t]));
    A.bill[out] = acc;
}
#endif

constexpr int kBillBaseMax = 256;                 // scenarios of one deviation launch (1 KB of arguments)
struct BillDevArgs {
    const double *bill;
    double *dev;
    int64_t n;
    int32_t s0;
    int32_t base[kBillBaseMax];                   // of scenarios s0 .. s0 + gridDim.y - 1
};

__global__ __launch_bounds__(256) void bill_dev_kernel(BillDevArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const int s = A.s0 + (int)blockIdx.y, b = A.base[blockIdx.y];
    double d = __builtin_nan("");
    if (b >= 0) {
        const double c1 = A.bill[(int64_t)b * A.n + i], c2 = A.bill[(int64_t)s * A.n + i];
        d = bill_mul(100.0, bill_sub(c2, c1)) / c1;
    }
    A.dev[(int64_t)s * A.n + i] = d;
}

// ---- the selection ---------------------------------------------------------------------------------------------------
constexpr int kBillSelNT = 1024;
constexpr int kBillMaskWords = 448;               // member bit masks of the groups of one launch (3.5 KB of arguments)
constexpr int kBillRed = 8;                       // values one block reduction carries
struct BillSelArgs {
    const double *val[2];                         // bill, dev: [S][n]
    const uint8_t *keep;                          // [S][n], or NULL
    const int32_t *ior;                           // index_of_row[n], or NULL
    revs_bill_summary_t *out;                     // [sets][2]
    int64_t n;
    int32_t words, g0, single;                    // single: the set of workgroup y is scenario y alone (no masks)
    unsigned long long member[kBillMaskWords];    // [groups of this launch][words]: bit s of a group's mask: scenario s
};

// a < b  <=>  bill_key(a) < bill_key(b) for two doubles that are no NaNs (across_kernels.hip's across_key)
__device__ __forceinline__ unsigned long long bill_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : u | (1ull << 63);
}
__device__ __forceinline__ double bill_val(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ (1ull << 63) : ~k));
}
// numpy.percentile's _lerp without contraction: across_lerp's roundings
__device__ __forceinline__ double bill_lerp(double a, double b, double t) {
    const double d = bill_sub(b, a);
    return t >= 0.5 ? bill_sub(b, bill_mul(d, bill_sub(1.0, t))) : bill_add(a, bill_mul(d, t));
}
__device__ __forceinline__ unsigned long long bill_uniform_u64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ double bill_uniform_d(double v) {
    return __longlong_as_double((long long)bill_uniform_u64((unsigned long long)__double_as_longlong(v)));
}

// max / sum of N values over the workgroup in a fixed tree (lanes, then the 16 wavefronts across one row of lanes):
// every thread gets them, the same bits from call to call.  `red`: 16 * kBillRed doubles.
template <int N, bool SUM>
__device__ __forceinline__ void bill_block_reduce(double (&v)[N], double *red) {
    static_assert(N <= kBillRed && kBillSelNT == 1024, "");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = SUM ? wave_sum_d(v[e]) : wave_max_d(v[e]);
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) red[wave * kBillRed + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) {
        double r = red[(lane & 15) * kBillRed + e];
        r = SUM ? r + dpp_rot_d<0x128>(r) : fmax(r, dpp_rot_d<0x128>(r));
        r = SUM ? r + dpp_rot_d<0x124>(r) : fmax(r, dpp_rot_d<0x124>(r));
        r = SUM ? r + dpp_rot_d<0x122>(r) : fmax(r, dpp_rot_d<0x122>(r));
        r = SUM ? r + dpp_rot_d<0x121>(r) : fmax(r, dpp_rot_d<0x121>(r));
        v[e] = bill_uniform_d(r);
    }
    __syncthreads();
}

// one count into h[d] per matching lane: by the first matching lane alone when the wavefront's digits agree
__device__ __forceinline__ void bill_hist_add(unsigned *h, bool match, unsigned d) {
    const unsigned long long m = __ballot(match);
    if (m == 0ull) return;
    const int first = (int)__builtin_ctzll(m);
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, first);
    if (__ballot(match && d == d0) == m) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(h + d0, (unsigned)__popcll(m));
    } else if (match) {
        atomicAdd(h + d, 1u);
    }
}

// f(v, ok, kept, scenario, row) over every row of the set's scenarios, ascending, every thread the same number of
// times (threads past a row's end see a value that is not kept): lane masks and reductions stay whole.  v is the
// value with -0.0 as +0.0; ok: kept and finite.
template <class F>
__device__ __forceinline__ void bill_for_each(const BillSelArgs &A, const double *val, int set, F f) {
    const int tid = threadIdx.x;
    for (int w = 0; w < A.words; ++w) {
        unsigned long long mk = A.single ? ((set >> 6) == w ? 1ull << (set & 63) : 0ull) : A.member[(size_t)set * A.words + w];
        while (mk) {
            const int s = 64 * w + (int)__builtin_ctzll(mk);
            mk &= mk - 1;
            const double *row = val + (int64_t)s * A.n;
            const uint8_t *kp = A.keep ? A.keep + (int64_t)s * A.n : nullptr;
            for (int64_t jb = 0; jb < A.n; jb += kBillSelNT) {
                const int64_t j = jb + tid;
                double v = __builtin_nan("");
                bool kept = false;
                if (j < A.n) {
                    kept = !kp || kp[j] != 0;
                    v = row[j] + 0.0;
                }
                f(v, kept && (v - v == 0.0), kept, s, (int)j);
            }
        }
    }
}

__global__ __launch_bounds__(kBillSelNT) void bill_select_kernel(BillSelArgs A) {
    __shared__ alignas(16) unsigned hist[3 * 256];
    __shared__ double red[16 * kBillRed];
    __shared__ unsigned found[3][4];              // per rank: digit, rank left inside the bin, the bin's count
    constexpr int NT = kBillSelNT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x, set = (int)blockIdx.y;
    const double *val = A.val[q];
    const double ninf = -__builtin_inf(), nan = __builtin_nan("");

    for (int i = tid; i < 3 * 256; i += NT) hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts, extremes, the total, and the top digit's histogram
    double c[4] = {0.0, 0.0, 0.0, 0.0};           // finite, kept and not finite, above zero; the values' sum
    double x[2] = {ninf, ninf};                   // -min, max
    bill_for_each(A, val, set, [&](double v, bool ok, bool kept, int, int) {
        c[0] += ok ? 1.0 : 0.0;
        c[1] += (kept && !ok) ? 1.0 : 0.0;
        if (ok) {
            c[2] += v > 0.0 ? 1.0 : 0.0;
            c[3] += v;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v);
        }
        bill_hist_add(hist, ok, (unsigned)(bill_key(v) >> 56));
    });
    bill_block_reduce<4, true>(c, red);
    bill_block_reduce<2, false>(x, red);
    const int kcnt = (int)c[0];
    revs_bill_summary_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.total = nan;
    r.reserved0 = 0.0;
    r.count = kcnt; r.n_nan = (int)c[1]; r.n_fliers = 0; r.n_above = (int)c[2];
    r.worst_index = r.worst_scenario = -1;
    revs_bill_summary_t *out = A.out + ((size_t)(A.g0 + set) * 2 + q);
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    // ---- the quartiles' lower order statistics: rank (k - 1) e / 4, e = 1, 2, 3
    int rank[3], rem4[3];
    unsigned left[3], eq[3] = {0u, 0u, 0u};       // rank left among the keys that share the prefix; keys equal to ans
    unsigned long long ans[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const long long rr = (long long)(kcnt - 1) * (e + 1);
        rank[e] = (int)(rr >> 2); rem4[e] = (int)(rr & 3);
        left[e] = (unsigned)rank[e];
    }
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        // ranks whose prefixes agree share a histogram (the prefixes ascend with the ranks: equal ones are adjacent)
        int slot[3] = {0, 0, 0};
        if (pass > 0) {
            slot[1] = ans[1] == ans[0] ? 0 : 1;
            slot[2] = ans[2] == ans[1] ? slot[1] : 2;
            const bool own1 = slot[1] == 1, own2 = slot[2] == 2;
            const unsigned long long p0 = ans[0] >> (shift + 8), p1 = ans[1] >> (shift + 8), p2 = ans[2] >> (shift + 8);
            bill_for_each(A, val, set, [&](double v, bool ok, bool, int, int) {
                const unsigned long long k = bill_key(v), pk = k >> (shift + 8);
                const unsigned d = (unsigned)(k >> shift) & 0xFFu;
                bill_hist_add(hist, ok && pk == p0, d);
                if (own1) bill_hist_add(hist + 256, ok && pk == p1, d);
                if (own2) bill_hist_add(hist + 512, ok && pk == p2, d);
            });
        }
        __syncthreads();
        // the bin that holds each rank: wavefront e for rank e, four bins per lane, a prefix sum across the lanes
        if (wave < 3) {
            const unsigned *h = hist + 256 * slot[wave];
            const uint4 cc = *reinterpret_cast<const uint4 *>(h + 4 * lane);
            const unsigned own = cc.x + cc.y + cc.z + cc.w;
            unsigned incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = (unsigned)__shfl_up((int)incl, o);
                if (lane >= o) incl += up;
            }
            const unsigned want = left[wave], excl = incl - own;
            if (want >= excl && want < incl) {    // (one lane: the bins' counts sum to more than the rank left)
                unsigned b = 0, below = excl, cnt = cc.x;
                if (want >= below + cnt) { below += cnt; b = 1; cnt = cc.y; }
                if (b == 1 && want >= below + cnt) { below += cnt; b = 2; cnt = cc.z; }
                if (b == 2 && want >= below + cnt) { below += cnt; b = 3; cnt = cc.w; }
                found[wave][0] = 4u * lane + b; found[wave][1] = want - below; found[wave][2] = cnt;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            ans[e] = bill_uniform_u64(ans[e] | (unsigned long long)found[e][0] << shift);      // (every lane holds the same)
            left[e] = __builtin_amdgcn_readfirstlane(found[e][1]); eq[e] = __builtin_amdgcn_readfirstlane(found[e][2]);
        }
        __syncthreads();                          // (every read of hist and found is done)
        for (int i = tid; i < 3 * 256; i += NT) hist[i] = 0u;
        __syncthreads();
    }
    // ---- the upper neighbours (the smallest value above each), and the worst entry: the largest value, lowest scenario,
    // then lowest caller-side index.  scenario 2^31 + index < 2^43 is exact in a double.
    double nw[4] = {ninf, ninf, ninf, ninf};      // -next above rank e; -(code of the worst entry)
    bill_for_each(A, val, set, [&](double v, bool ok, bool, int sidx, int j) {
        if (!ok) return;
        const unsigned long long k = bill_key(v);
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (k > ans[e]) nw[e] = fmax(nw[e], -v);
        if (v == x[1]) {
            const int idx = A.ior ? A.ior[j] : j;
            nw[3] = fmax(nw[3], -((double)sidx * 2147483648.0 + (double)idx));
        }
    });
    bill_block_reduce<4, false>(nw, red);
    double qv[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double lo = bill_val(ans[e]);
        const int cle = rank[e] - (int)left[e] + (int)eq[e];        // values <= the order statistic
        const bool last = rank[e] + 1 >= kcnt;
        const double hi = (last || cle > rank[e] + 1) ? lo : -nw[e];
        qv[e] = bill_lerp(lo, hi, 0.25 * (double)rem4[e]);
    }
    // ---- whiskers and fliers, as net_report_kernel's
    const double iqr = bill_sub(qv[2], qv[0]);
    const double lim0 = bill_sub(qv[0], bill_mul(1.5, iqr)), lim1 = bill_add(qv[2], bill_mul(1.5, iqr));
    double wk[2] = {ninf, ninf};
    bill_for_each(A, val, set, [&](double v, bool ok, bool, int, int) {
        if (ok && v >= lim0) wk[0] = fmax(wk[0], -v);
        if (ok && v <= lim1) wk[1] = fmax(wk[1], v);
    });
    bill_block_reduce<2, false>(wk, red);
    const double wlo = (wk[0] == ninf || -wk[0] > qv[0]) ? qv[0] : -wk[0];
    const double whi = (wk[1] == ninf || wk[1] < qv[2]) ? qv[2] : wk[1];
    double fl[1] = {0.0};
    bill_for_each(A, val, set, [&](double v, bool ok, bool, int, int) {
        fl[0] += (ok && (v < wlo || v > whi)) ? 1.0 : 0.0;
    });
    bill_block_reduce<1, true>(fl, red);
    if (tid == 0) {
        const long long code = (long long)-nw[3];
        r.min = -x[0] + 0.0; r.q1 = qv[0]; r.median = qv[1]; r.q3 = qv[2]; r.max = x[1];
        r.whisker_lo = wlo + 0.0; r.whisker_hi = whi;
        r.total = c[3];
        r.n_fliers = (int)fl[0];
        r.worst_scenario = (int)(code >> 31); r.worst_index = (int)(code & 0x7FFFFFFFll);
        *out = r;
    }
}

}  // namespace revs

using namespace revs;

static bool bill_sizes_ok(int32_t S, int64_t n) {
    return S >= 1 && S <= REVS_STUDY_MAX_S && n >= 1 && n < ((int64_t)1 << 31) && (int64_t)S * n < ((int64_t)1 << 31);
}

extern "C" int revs_bill_rows(int32_t S, int64_t n, int32_t T, const void *g, int32_t g_f64, int64_t stride_s,
                              int64_t stride_i, const double *tariff, double *bill, void *stream) {
    const char *who = "revs_bill_rows";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(bill_sizes_ok(S, n), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(g, "%s: null pointer argument g", who);
    REVS_REQUIRE(tariff, "%s: null pointer argument tariff", who);
    REVS_REQUIRE(bill, "%s: null pointer argument bill", who);
    REVS_REQUIRE(g_f64 == 0 || g_f64 == 1, "%s: g_f64=%d is neither 0 nor 1", who, (int)g_f64);
    // a >= k b for positive integers is a / b >= k: no product that could overflow
    const bool inner_i = stride_i >= T && stride_s / stride_i >= n;
    const bool inner_s = stride_s >= T && stride_i / stride_s >= S;
    REVS_REQUIRE(inner_i || inner_s, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    BillRowsArgs A;
    A.g = g; A.tariff = tariff; A.bill = bill; A.stride_s = stride_s; A.stride_i = stride_i;
    A.n = (uint32_t)n; A.S = (uint32_t)S; A.rows = (uint32_t)((int64_t)S * n); A.T = T; A.inner_i = inner_i ? 1 : 0;
    const dim3 grid((A.rows + kBillNT - 1) / kBillNT);
    if (g_f64) hipLaunchKernelGGL(bill_rows_kernel<double>, grid, dim3(kBillNT), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(bill_rows_kernel<float>, grid, dim3(kBillNT), 0, (hipStream_t)stream, A);
    REVS_CHECK_LAUNCH(who);
    return REVS_OK;
}

extern "C" int64_t revs_bill_study_scratch(int32_t S, int64_t n) {
    if (!bill_sizes_ok(S, n)) return 0;
    return (int64_t)S * n * (int64_t)sizeof(double);
}

extern "C" int revs_bill_study(int32_t S, int64_t n, const double *bill, const int32_t *base, const uint8_t *keep,
                               const int32_t *index_of_row, const int32_t *group, int32_t G, double *dev_out,
                               revs_bill_summary_t *summary_out, revs_bill_summary_t *pooled_out, void *scratch,
                               void *stream) {
    static_assert(sizeof(revs_bill_summary_t) == 96, "");
    static_assert(sizeof(BillSelArgs) <= 4096 && sizeof(BillDevArgs) <= 4096, "kernel arguments");
    const char *who = "revs_bill_study";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(bill_sizes_ok(S, n), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(bill, "%s: null pointer argument bill", who);
    REVS_REQUIRE(base, "%s: base is NULL", who);
    for (int s = 0; s < S; ++s)
        REVS_REQUIRE(base[s] >= -1 && base[s] < S, "%s: base[%d]=%d outside -1..S-1", who, s, (int)base[s]);
    REVS_REQUIRE(G >= 0 && G <= S, "%s: G=%d outside 0..S", who, (int)G);
    REVS_REQUIRE(G == 0 || group, "%s: group is NULL with G > 0", who);
    for (int s = 0; s < S && G > 0; ++s)
        REVS_REQUIRE(group[s] >= -1 && group[s] < G, "%s: group[%d]=%d outside -1..G-1", who, s, (int)group[s]);
    const bool select = summary_out || pooled_out;
    REVS_REQUIRE(dev_out || select, "%s: every output is NULL", who);
    REVS_REQUIRE(!pooled_out || G > 0, "%s: pooled_out with G == 0", who);
    REVS_REQUIRE(!select || scratch, "%s: summary_out / pooled_out need scratch (revs_bill_study_scratch bytes)", who);
    REVS_REQUIRE(!select || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);

    hipStream_t st = (hipStream_t)stream;
    double *dev = dev_out ? dev_out : (double *)scratch;
    BillDevArgs D;
    D.bill = bill; D.dev = dev; D.n = n;
    for (int s0 = 0; s0 < S; s0 += kBillBaseMax) {
        const int ns = S - s0 < kBillBaseMax ? S - s0 : kBillBaseMax;
        for (int i = 0; i < kBillBaseMax; ++i) D.base[i] = i < ns ? base[s0 + i] : -1;
        D.s0 = s0;
        hipLaunchKernelGGL(bill_dev_kernel, dim3((unsigned)((n + 255) / 256), ns), dim3(256), 0, st, D);
        REVS_CHECK_LAUNCH(who);
    }
    if (!select) return REVS_OK;
    BillSelArgs A;
    A.val[0] = bill; A.val[1] = dev; A.keep = keep; A.ior = index_of_row; A.n = n; A.words = (S + 63) / 64;
    for (int i = 0; i < kBillMaskWords; ++i) A.member[i] = 0ull;
    if (summary_out) {
        A.out = summary_out; A.g0 = 0; A.single = 1;
        hipLaunchKernelGGL(bill_select_kernel, dim3(2, S), dim3(kBillSelNT), 0, st, A);
        REVS_CHECK_LAUNCH(who);
    }
    if (pooled_out) {
        // the groups' member masks travel as kernel arguments: as many groups per launch as kBillMaskWords holds
        A.out = pooled_out; A.single = 0;
        const int per = kBillMaskWords / A.words;
        for (int g0 = 0; g0 < G; g0 += per) {
            const int ng = G - g0 < per ? G - g0 : per;
            for (int i = 0; i < kBillMaskWords; ++i) A.member[i] = 0ull;
            for (int s = 0; s < S; ++s)
                if (group[s] >= g0 && group[s] < g0 + ng)
                    A.member[(size_t)(group[s] - g0) * A.words + s / 64] |= 1ull << (s % 64);
            A.g0 = g0;
            hipLaunchKernelGGL(bill_select_kernel, dim3(2, ng), dim3(kBillSelNT), 0, st, A);
            REVS_CHECK_LAUNCH(who);
        }
    }
    return REVS_OK;
}
