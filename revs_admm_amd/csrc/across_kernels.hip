// Statistics per node and per line ACROSS the scenarios of a study (include/revs_admm_ops.h, "study report, per node
// and per line"): for every cell (node or line n, slot t) of revs_net_study's volt_out or
// loading_out, the box-plot numbers, the mean, the violations, the band counts and the worst scenario over the
// scenarios of a group.
//
//   net_across_kernel        one thread per cell c = n T + t and group: values[s] is contiguous over c, so the walk over
//                            the group's members at stride n_out T reads coalesced rows; the member loop is the same for
//                            every thread of a workgroup.  Nothing crosses lanes.
//   net_across_daily_kernel  a scenario's daily extreme per node into the scratch, double[S][n_out]: net_across_kernel
//                            then runs on it as its T = 1 case
//   net_across_exposure_kernel   the (member, slot) pairs in violation per node
//
// Members travel as bit masks in the kernel arguments (pack_group_masks, common.h), as many groups per
// launch as fit; a workgroup expands its group's mask once into a list of scenario indices in LDS (8 KB), so that the
// member loops are counted loops the compiler unrolls with their loads in flight together.
//
// The order statistics are exact and need no sort: a double's ordered key (boxplot.h) orders like the value (any
// double: negatives, infinities; -0.0 as +0.0), and the k-th smallest key is built bit by bit from the top for the
// three quartile ranks at once, one pass over the members per bit -- starting below the bits the cell's smallest and
// largest key share, which no pass needs to find.  The passes re-read the members' values: a study's arrays stay in L2.
#include "common.h"
#include "boxplot.h"

#include <math.h>

namespace revs {

constexpr int kAcrossNT = 256;
struct AcrossArgs {
    const double *values;                         // [S][cells]
    const uint8_t *keep;                          // [n_out], or NULL
    revs_net_across_t *out;                       // [G][cells]
    int32_t cells, T, g0, words, le;              // cells = n_out T; le: bands count v <= band (else v >= band)
    double lo, hi;
    double band[REVS_ACROSS_MAX_BANDS];           // (a NaN: unused, never counted)
    unsigned long long member[kGroupMaskWords];  // [groups of this launch][words]: bit s of a group's mask: scenario s
};

__global__ __launch_bounds__(kAcrossNT) void net_across_kernel(AcrossArgs A) {
    __shared__ unsigned short mem[REVS_STUDY_MAX_S];
    __shared__ int mem_count;
    const int tid = threadIdx.x, gl = (int)blockIdx.y;
    if (tid < 64) {                               // the group's members, ascending
        const unsigned long long *member = A.member + (size_t)gl * A.words;
        int base = 0;
        for (int w = 0; w < A.words; ++w) {
            const unsigned long long mk = member[w];
            if ((mk >> tid) & 1ull) mem[base + __popcll(mk & ((1ull << tid) - 1ull))] = (unsigned short)(64 * w + tid);
            base += __popcll(mk);
        }
        if (tid == 0) mem_count = base;
    }
    __syncthreads();
    const int c = (int)blockIdx.x * kAcrossNT + tid;
    if (c >= A.cells) return;
    const bool kept = !A.keep || A.keep[c / A.T] != 0;
    const int nm = kept ? mem_count : 0;
    const int64_t stride = A.cells;
    const double *col = A.values + c;
    const double lo = A.lo, hi = A.hi, inf = __builtin_inf(), nan = __builtin_nan("");
    const bool le = A.le != 0;

    // ---- pass 1: counts, extremes, the ordered sum, violations, bands, the worst scenario
    int cnt = 0, nnan = 0, viol = 0, worst = -1;
    int bc[REVS_ACROSS_MAX_BANDS];
#pragma unroll
    for (int b = 0; b < REVS_ACROSS_MAX_BANDS; ++b) bc[b] = 0;
    double mn = inf, mx = -inf, sum = 0.0, wexc = -inf;
#pragma unroll 4
    for (int k = 0; k < nm; ++k) {
        const int s = mem[k];
        const double v = col[s * stride] + 0.0;
        if (v != v) { ++nnan; continue; }
        const double exc = fmax(lo - v, v - hi);
        if (cnt == 0 || exc > wexc) { wexc = exc; worst = s; }
        ++cnt;
        sum += v;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
        viol += (v < lo || v > hi) ? 1 : 0;
#pragma unroll
        for (int b = 0; b < REVS_ACROSS_MAX_BANDS; ++b) bc[b] += (le ? v <= A.band[b] : v >= A.band[b]) ? 1 : 0;
    }

    revs_net_across_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.mean = nan;
    r.count = cnt; r.n_nan = nnan; r.n_violations = viol; r.worst_scenario = worst;
#pragma unroll
    for (int b = 0; b < REVS_ACROSS_MAX_BANDS; ++b) r.band_count[b] = bc[b];
    revs_net_across_t *out = A.out + ((int64_t)(A.g0 + gl) * A.cells + c);
    if (cnt == 0) { *out = r; return; }

    // ---- pass 2: the quartiles' lower order statistics, rank (cnt - 1) e / 4, e = 1, 2, 3, bit by bit below the
    // prefix the smallest and the largest key share
    unsigned rank[3];
    unsigned long long ans[3];
    const unsigned long long kmin = box_key(mn), kmax = box_key(mx);
    const int top = kmin == kmax ? -1 : 63 - (int)__builtin_clzll(kmin ^ kmax);
    const unsigned long long prefix = top < 0 ? kmin : kmin & ~((2ull << top) - 1ull);     // (top == 63: no shared bit)
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        unsigned rem4;
        box_rank((unsigned)cnt, e + 1, rank[e], rem4);
        ans[e] = prefix;
    }
#pragma unroll 1
    for (int bit = top; bit >= 0; --bit) {
        unsigned long long trial[3];
        int below[3] = {0, 0, 0};
#pragma unroll
        for (int e = 0; e < 3; ++e) trial[e] = ans[e] | (1ull << bit);
#pragma unroll 4
        for (int k = 0; k < nm; ++k) {
            const double v = col[mem[k] * stride];
            const unsigned long long key = box_key(v);
            const bool ok = v == v;
#pragma unroll
            for (int e = 0; e < 3; ++e) below[e] += (ok && key < trial[e]) ? 1 : 0;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if ((unsigned)below[e] <= rank[e]) ans[e] = trial[e];
    }
    // ---- the upper neighbours of the five order statistics (min, the quartiles, max): the same value when it repeats
    // past the rank, else the smallest value above it
    const unsigned long long stat[5] = {kmin, ans[0], ans[1], ans[2], kmax};
    int cle[5] = {0, 0, 0, 0, 0};
    unsigned long long nxt[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll 4
    for (int k = 0; k < nm; ++k) {
        const double v = col[mem[k] * stride];
        const unsigned long long key = box_key(v);
        if (v != v) continue;
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            if (key <= stat[e]) ++cle[e];
            else nxt[e] = key < nxt[e] ? key : nxt[e];
        }
    }
    // numpy's rule for all five, min and max too: a + (b - a) 0 is a for finite values and a NaN where b - a is not
    double qv[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        unsigned rk, rem4;
        box_rank((unsigned)cnt, e, rk, rem4);
        const double a = box_val(stat[e]);
        qv[e] = box_quartile(a, box_next_differs(rk, (unsigned)cnt, (unsigned)cle[e]) ? box_val(nxt[e]) : a, rem4);
    }
    r.min = qv[0]; r.q1 = qv[1]; r.median = qv[2]; r.q3 = qv[3]; r.max = qv[4];
    r.mean = sum / (double)cnt;
    *out = r;
}

// daily[s][n] = min (le) / max over t of values[s][n][t]; a NaN if any slot is one
__global__ void net_across_daily_kernel(int total, int T, int le, const double *values, double *daily) {
    const int idx = (int)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const double *p = values + (int64_t)idx * T;
    double d = p[0];
    bool bad = d != d;
    for (int t = 1; t < T; ++t) {
        const double v = p[t];
        bad |= v != v;
        d = le ? (v < d ? v : d) : (v > d ? v : d);
    }
    daily[idx] = bad ? __builtin_nan("") : d;
}

struct ExposureArgs {
    const double *values;
    const uint8_t *keep;
    int32_t *out;                                 // [G][n_out]
    int32_t n_out, T, g0, words;
    double lo, hi;
    unsigned long long member[kGroupMaskWords];
};

__global__ __launch_bounds__(kAcrossNT) void net_across_exposure_kernel(ExposureArgs A) {
    const int n = (int)blockIdx.x * kAcrossNT + (int)threadIdx.x, gl = (int)blockIdx.y;
    if (n >= A.n_out) return;
    const unsigned long long *member = A.member + (size_t)gl * A.words;
    int viol = 0;
    if (!A.keep || A.keep[n] != 0) {
        for (int w = 0; w < A.words; ++w) {
            unsigned long long mk = member[w];
            while (mk) {
                const int s = 64 * w + (int)__builtin_ctzll(mk);
                mk &= mk - 1;
                const double *p = A.values + ((int64_t)s * A.n_out + n) * A.T;
                for (int t = 0; t < A.T; ++t) viol += (p[t] < A.lo || p[t] > A.hi) ? 1 : 0;
            }
        }
    }
    A.out[(int64_t)(A.g0 + gl) * A.n_out + n] = viol;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_across_scratch(int32_t S, int32_t n_out) {
    if (S < 1 || S > REVS_STUDY_MAX_S || n_out < 1 || n_out > 0xFFFF) return 0;
    return (int64_t)S * n_out * (int64_t)sizeof(double);
}

extern "C" int revs_net_across(int32_t S, int32_t n_out, int32_t T, const double *values, const uint8_t *keep,
                               const int32_t *group, int32_t G, double lo, double hi, int32_t sense, const double *band,
                               int32_t B, revs_net_across_t *slot_out, revs_net_across_t *daily_out, int32_t *exposure_out,
                               void *scratch, void *stream) {
    static_assert(sizeof(revs_net_across_t) == 96, "");
    static_assert(sizeof(AcrossArgs) <= 4096 && sizeof(ExposureArgs) <= 4096, "kernel arguments");
    const char *who = "revs_net_across";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n_out > 0 && n_out <= 0xFFFF, "%s: n_out=%d outside 1..65535", who, (int)n_out);
    const int64_t total = (int64_t)S * n_out * T;
    REVS_REQUIRE(total < ((int64_t)1 << 31), "%s: S*n_out*T=%lld values, 2^31 or more", who, (long long)total);
    REVS_REQUIRE(G >= 1 && G <= S, "%s: G=%d outside 1..S", who, (int)G);
    REVS_REQUIRE(group, "%s: group is NULL", who);
    for (int s = 0; s < S; ++s)
        REVS_REQUIRE(group[s] >= -1 && group[s] < G, "%s: group[%d]=%d outside -1..G-1", who, s, (int)group[s]);
    REVS_REQUIRE(B >= 0 && B <= REVS_ACROSS_MAX_BANDS, "%s: B=%d outside 0..%d", who, (int)B, REVS_ACROSS_MAX_BANDS);
    REVS_REQUIRE(B == 0 || band, "%s: band is NULL with B > 0", who);
    for (int b = 0; b < B; ++b)
        REVS_REQUIRE(band[b] - band[b] == 0.0, "%s: band[%d] is not finite", who, b);
    REVS_REQUIRE(sense == -1 || sense == 1, "%s: sense=%d is neither -1 nor +1", who, (int)sense);
    REVS_REQUIRE(lo <= hi, "%s: lo > hi, or a NaN in either", who);     // (also rejects NaN)
    REVS_REQUIRE(values, "%s: null pointer argument values", who);
    REVS_REQUIRE(slot_out || daily_out || exposure_out, "%s: every output is NULL", who);
    // (exposure_out alone never touches the scratch -- only the daily extremes are staged there -- but the contract
    //  asks for it with either output, so that a caller's buffer does not depend on which of the two it wants)
    const bool day = daily_out || exposure_out;
    REVS_REQUIRE(!day || scratch, "%s: daily_out / exposure_out need scratch (revs_net_across_scratch bytes)", who);
    REVS_REQUIRE(!day || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);

    hipStream_t st = (hipStream_t)stream;
    const int le = sense < 0 ? 1 : 0;
    if (daily_out) {
        const int tot = S * n_out;
        hipLaunchKernelGGL(net_across_daily_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tot, (int)T, le,
                           values, (double *)scratch);
        REVS_CHECK_LAUNCH(who);
    }
    AcrossArgs A;
    A.keep = keep; A.lo = lo; A.hi = hi; A.le = le; A.words = (S + 63) / 64;
    for (int b = 0; b < REVS_ACROSS_MAX_BANDS; ++b) A.band[b] = b < B ? band[b] : NAN;
    ExposureArgs E;
    E.values = values; E.keep = keep; E.out = exposure_out; E.n_out = n_out; E.T = T; E.words = A.words; E.lo = lo; E.hi = hi;
    for (int g0 = 0, ng; g0 < G; g0 += ng) {
        ng = pack_group_masks(group, S, G, g0, A.member);
        A.g0 = g0;
        if (slot_out) {
            A.values = values; A.out = slot_out; A.cells = n_out * T; A.T = T;
            hipLaunchKernelGGL(net_across_kernel, dim3((unsigned)((A.cells + kAcrossNT - 1) / kAcrossNT), ng), dim3(kAcrossNT),
                               0, st, A);
            REVS_CHECK_LAUNCH(who);
        }
        if (daily_out) {                          // the same kernel on the daily extremes: T = 1
            A.values = (const double *)scratch; A.out = daily_out; A.cells = n_out; A.T = 1;
            hipLaunchKernelGGL(net_across_kernel, dim3((unsigned)((A.cells + kAcrossNT - 1) / kAcrossNT), ng), dim3(kAcrossNT),
                               0, st, A);
            REVS_CHECK_LAUNCH(who);
        }
        if (exposure_out) {
            for (int i = 0; i < kGroupMaskWords; ++i) E.member[i] = A.member[i];
            E.g0 = g0;
            hipLaunchKernelGGL(net_across_exposure_kernel, dim3((unsigned)((n_out + kAcrossNT - 1) / kAcrossNT), ng),
                               dim3(kAcrossNT), 0, st, E);
            REVS_CHECK_LAUNCH(who);
        }
    }
    return REVS_OK;
}
