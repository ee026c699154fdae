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
//   bill_select_kernel     one workgroup per (member set, quantity): pass 0, then the radix selection of boxplot.h
//                          (box_select64) over signed doubles under their ordered keys, reading
//                          the values themselves (bill / dev, double[S][n]) under the keep mask.  A member set is one
//                          scenario (the summaries) or a group's bit mask from the kernel arguments (the pools); both
//                          walk a scenario's row with the same thread for the same element, so a pool of one scenario
//                          repeats that scenario's record bit for bit, `total` included.
#include "common.h"
#include "boxplot.h"

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
struct BillSelArgs {
    const double *val[2];                         // bill, dev: [S][n]
    const uint8_t *keep;                          // [S][n], or NULL
    const int32_t *ior;                           // index_of_row[n], or NULL
    revs_bill_summary_t *out;                     // [sets][2]
    int64_t n;
    int32_t words, g0, single;                    // single: the set of workgroup y is scenario y alone (no masks)
    unsigned long long member[kGroupMaskWords];   // [groups of this launch][words]: bit s of a group's mask: scenario s
};

// f(key, ok, v, scenario, row, kept) over every row of the set's scenarios, ascending, every thread the same number of
// times (threads past a row's end see a value that is not kept): lane masks and reductions stay whole.  v is the
// value with -0.0 as +0.0, key its ordered key; ok: kept and finite.
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
                double raw = __builtin_nan("");
                bool kept = false;
                if (j < A.n) {
                    kept = !kp || kp[j] != 0;
                    raw = row[j];
                }
                const double v = raw + 0.0;
                f(box_key(raw), kept && (v - v == 0.0), v, s, (int)j, kept);
            }
        }
    }
}

__global__ __launch_bounds__(kBillSelNT) void bill_select_kernel(BillSelArgs A) {
    __shared__ BoxSelect<kBillSelNT> sh;
    constexpr int NT = kBillSelNT;
    const int tid = threadIdx.x;
    const int q = (int)blockIdx.x, set = (int)blockIdx.y;
    const double *val = A.val[q];
    const double ninf = -__builtin_inf(), nan = __builtin_nan("");

    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts, extremes, the total, and the top digit's histogram
    double c[4] = {0.0, 0.0, 0.0, 0.0};           // finite, kept and not finite, above zero; the values' sum
    double x[2] = {ninf, ninf};                   // -min, max
    bill_for_each(A, val, set, [&](unsigned long long k, bool ok, double v, int, int, bool kept) {
        c[0] += ok ? 1.0 : 0.0;
        c[1] += (kept && !ok) ? 1.0 : 0.0;
        if (ok) {
            c[2] += v > 0.0 ? 1.0 : 0.0;
            c[3] += v;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v);
        }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 4, true>(c, sh.red);
    block_reduce_multi<NT, 2, false>(x, sh.red);
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
    // ---- the selection; in its neighbour walk the worst entry: the largest value, lowest scenario, then lowest
    // caller-side index.  scenario 2^31 + index < 2^43 is exact in a double.
    double wc[1] = {ninf};                        // -(code of the worst entry)
    const BoxFigures b = box_select64(sh, kcnt,
        [&](auto f) {
            bill_for_each(A, val, set, [&](unsigned long long k, bool ok, double v, int s, int j, bool) { f(k, ok, v, s, j); });
        },
        [&](unsigned long long, bool ok, double v, int sidx, int j) {
            if (ok && v == x[1]) {
                const int idx = A.ior ? A.ior[j] : j;
                wc[0] = fmax(wc[0], -((double)sidx * 2147483648.0 + (double)idx));
            }
        });
    block_reduce_multi<NT, 1, false>(wc, sh.red);
    if (tid == 0) {
        const long long code = (long long)-wc[0];
        r.min = -x[0] + 0.0; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo + 0.0; r.whisker_hi = b.whi;
        r.total = c[3];
        r.n_fliers = b.n_fliers;
        r.worst_scenario = (int)(code >> 31); r.worst_index = (int)(code & 0x7FFFFFFFll);
        *out = r;
    }
}

}  // namespace revs

using namespace revs;

extern "C" int revs_bill_rows(int32_t S, int64_t n, int32_t T, const void *g, int32_t g_f64, int64_t stride_s,
                              int64_t stride_i, const double *tariff, double *bill, void *stream) {
    const char *who = "revs_bill_rows";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(study_sizes_ok(S, n), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(g, "%s: null pointer argument g", who);
    REVS_REQUIRE(tariff, "%s: null pointer argument tariff", who);
    REVS_REQUIRE(bill, "%s: null pointer argument bill", who);
    REVS_REQUIRE(g_f64 == 0 || g_f64 == 1, "%s: g_f64=%d is neither 0 nor 1", who, (int)g_f64);
    const int inner_i = rows_inner_i(S, n, T, stride_s, stride_i);
    REVS_REQUIRE(inner_i >= 0, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    BillRowsArgs A;
    A.g = g; A.tariff = tariff; A.bill = bill; A.stride_s = stride_s; A.stride_i = stride_i;
    A.n = (uint32_t)n; A.S = (uint32_t)S; A.rows = (uint32_t)((int64_t)S * n); A.T = T; A.inner_i = inner_i;
    const dim3 grid((A.rows + kBillNT - 1) / kBillNT);
    if (g_f64) hipLaunchKernelGGL(bill_rows_kernel<double>, grid, dim3(kBillNT), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(bill_rows_kernel<float>, grid, dim3(kBillNT), 0, (hipStream_t)stream, A);
    REVS_CHECK_LAUNCH(who);
    return REVS_OK;
}

extern "C" int64_t revs_bill_study_scratch(int32_t S, int64_t n) {
    if (!study_sizes_ok(S, n)) return 0;
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
    REVS_REQUIRE(study_sizes_ok(S, n), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
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
    BillSelArgs A = {};
    A.val[0] = bill; A.val[1] = dev; A.keep = keep; A.ior = index_of_row; A.n = n; A.words = (S + 63) / 64;
    if (summary_out) {
        A.out = summary_out; A.g0 = 0; A.single = 1;
        hipLaunchKernelGGL(bill_select_kernel, dim3(2, S), dim3(kBillSelNT), 0, st, A);
        REVS_CHECK_LAUNCH(who);
    }
    if (pooled_out) {
        A.out = pooled_out; A.single = 0;
        for (int g0 = 0, ng; g0 < G; g0 += ng) {
            ng = pack_group_masks(group, S, G, g0, A.member);
            A.g0 = g0;
            hipLaunchKernelGGL(bill_select_kernel, dim3(2, ng), dim3(kBillSelNT), 0, st, A);
            REVS_CHECK_LAUNCH(who);
        }
    }
    return REVS_OK;
}
