// Rule-based charging baselines (include/revs_admm_ops.h, "rule schedules"): what the charger
// does when nobody schedules it -- from the first window slot on (uncontrolled), as late as the window allows
// (last-minute) or at one constant power over the window (trickle) -- with the state of charge and the net load that
// follow, for every (residence, scenario) record at once.
//
// Every output element is a function of its row's record and its slot index alone: no LDS, no cross-lane traffic, no
// atomics, and nothing of the sweep's lane-group shapes.  One launch per kind of output that is wanted:
//   rule_pg_kernel<VEC, P, G>   p and / or g, float[rows][T] taken as ONE run of rows T elements.  A thread owns VEC
//                               consecutive elements; VEC = 4 where T % 4 == 0 (the four never leave their row) and the
//                               arrays are 16-byte aligned: a wavefront then writes 1 KiB of consecutive addresses per
//                               store instruction (and reads load the same way), otherwise 256 bytes.
//   rule_soc_kernel             soc, float[rows][T + 1] as one run of rows (T + 1) elements, dword stores (T + 1 and T
//                               are never both multiples of four).
//   rule_status_kernel          status, one thread per row.
// A thread finds its row from the workgroup's first element (one 64-bit division of uniform values) and a 32-bit
// division of its offset from there.  It loads the row's 32-byte record itself: the lanes of a wavefront that share a
// row carry the same address in the same load instruction, so the record reaches the wavefront by that one
// instruction and is fetched from memory once; the row's plan (window, number of full slots, partial slot) is then
// formed once per thread, not once per element.
#include "common.h"

#include <math.h>

// Every double operation is rounded on its own, as numpy's (tests/rules_ref.py): no contraction anywhere in this file.
#pragma clang fp contract(off)

namespace revs {

constexpr int kRuleNT = 256;

struct RuleArgs {
    const revs_home_t *homes;
    const float *load;
    float *p, *soc, *g;
    int32_t *status;
    int64_t rows;
    int32_t T, policy, fill, integral;
    int32_t rec16;                                // homes is 16-byte aligned: a record is two 16-byte loads
};

enum : int { kRuleNoEv = 0, kRuleEmpty = 1, kRuleBlock = 2, kRuleEven = 3 };

// What the elements of a row are functions of.  Window positions j = t - ws in 0 .. W - 1; the slots at `rating` are
// positions first .. first + nfull - 1, the partial slot (power rem) is position part (-1: none).
struct RulePlan {
    double rating, cap, ini, rem, even;
    float rating_f, ini_f, rem_f, even_f;
    int ws, W, first, nfull, part, kind, status;
};

__device__ __forceinline__ revs_home_t rule_record(const RuleArgs &A, int64_t row) {
    revs_home_t h;
    if (A.rec16) {
        const uint4 *q = reinterpret_cast<const uint4 *>(A.homes + row);
        const uint4 a = q[0], b = q[1];
        h.ev = (int32_t)a.x; h.start = (int32_t)a.y; h.end = (int32_t)a.z; h.nmin = (int32_t)a.w;
        h.nmax = (int32_t)b.x; h.rating = __uint_as_float(b.y); h.capacity = __uint_as_float(b.z);
        h.initial = __uint_as_float(b.w);
    } else {
        h = A.homes[row];
    }
    return h;
}

__device__ __forceinline__ RulePlan rule_plan(const revs_home_t &h, const RuleArgs &A) {
    RulePlan P;
    const int T = A.T;
    const int ws = min(max(h.start, 0), T), we = min(max(h.end, 0), T);
    const int W = max(we - ws, 0);
    P.rating = (double)h.rating; P.cap = (double)h.capacity; P.ini = (double)h.initial;
    P.rating_f = h.rating; P.ini_f = h.initial;
    P.rem = 0.0; P.even = 0.0; P.rem_f = 0.f; P.even_f = 0.f;
    P.ws = ws; P.W = 0; P.first = 0; P.nfull = 0; P.part = -1; P.status = 0;
    if (h.ev == 0) { P.kind = kRuleNoEv; return P; }
    if (h.nmax < 0 || (A.integral && h.nmin > h.nmax)) { P.kind = kRuleEmpty; P.status = 1; return P; }
    P.W = W;
    P.kind = kRuleBlock;
    int kf;
    if (A.integral) {
        const int k = A.fill == REVS_FILL_FULL ? h.nmax : h.nmin;
        const int on = min(k, W);
        P.status = on < h.nmin ? 1 : 0;
        kf = max(on, 0);
    } else {
        const double top = P.ini > 0.9 ? P.ini : 0.9;
        const double elo = (top - P.ini) * P.cap, ehi = (1.0 - P.ini) * P.cap;
        const double E = A.fill == REVS_FILL_FULL ? ehi : elo;
        const double rw = P.rating * (double)W;
        const double D = rw < E ? rw : E;
        P.status = D < elo ? 1 : 0;
        if (A.policy == REVS_RULE_EVEN) {
            P.kind = kRuleEven;
            P.even = W > 0 ? D / (double)W : 0.0;
            P.even_f = (float)P.even;
            return P;
        }
        const double q = floor(D / P.rating);
        kf = P.rating > 0.0 ? (q >= (double)W ? W : (q > 0.0 ? (int)q : 0)) : 0;
        if (kf < W) {
            // (D / rating may round UP to an integer: the remainder is then a rounding error below zero, never a power)
            const double r = D - (double)kf * P.rating;
            P.rem = r > 0.0 ? r : 0.0;
            P.rem_f = (float)P.rem;
        }
    }
    P.nfull = kf;
    if (A.policy == REVS_RULE_ALAP) {
        P.first = W - kf;
        P.part = (!A.integral && kf < W) ? W - kf - 1 : -1;
    } else {
        P.part = (!A.integral && kf < W) ? kf : -1;
    }
    return P;
}

__device__ __forceinline__ float rule_p(const RulePlan &P, int t) {
    const int j = t - P.ws;
    if (j < 0 || j >= P.W) return 0.f;            // (no EV, empty rows: W = 0)
    if (P.kind == kRuleEven) return P.even_f;
    if (j >= P.first && j < P.first + P.nfull) return P.rating_f;
    if (j == P.part) return P.rem_f;
    return 0.f;
}

// soc[t], t in 0 .. T: initial + (energy of the slots before t) / capacity, the energy in closed form
__device__ __forceinline__ float rule_soc(const RulePlan &P, int t) {
    if (P.kind == kRuleNoEv) return 0.f;
    if (t == 0 || P.kind == kRuleEmpty) return P.ini_f;
    const int jt = min(max(t - P.ws, 0), P.W);    // window slots before t
    double E;
    if (P.kind == kRuleEven) {
        E = (double)jt * P.even;
    } else {
        const int nf = min(max(jt - P.first, 0), P.nfull);
        E = (double)nf * P.rating;
        if (P.part >= 0 && jt > P.part) E = E + P.rem;
    }
    return (float)(P.ini + E / P.cap);
}

// the row and the slot of element tid * VEC of the workgroup's run of kRuleNT * VEC elements, rows of `width` elements
__device__ __forceinline__ void rule_locate(int width, int vec, int64_t &row, int &t, int64_t &e) {
    const int64_t e0 = (int64_t)blockIdx.x * (int64_t)(kRuleNT * vec);          // (uniform)
    const int64_t r0 = e0 / width;
    const uint32_t off = (uint32_t)(e0 - r0 * width) + (uint32_t)threadIdx.x * (uint32_t)vec;   // < width + 1024
    const uint32_t dr = off / (uint32_t)width;
    row = r0 + (int64_t)dr;
    t = (int)(off - dr * (uint32_t)width);
    e = e0 + (int64_t)threadIdx.x * vec;
}

template <int VEC, bool HAS_P, bool HAS_G>
__global__ __launch_bounds__(kRuleNT) void rule_pg_kernel(RuleArgs A) {
    int64_t row, e;
    int t;
    rule_locate(A.T, VEC, row, t, e);
    if (row >= A.rows) return;                    // (e < rows T exactly when row < rows; VEC divides T)
    const revs_home_t h = rule_record(A, row);
    const RulePlan P = rule_plan(h, A);
    if constexpr (VEC == 4) {
        float4 pv;
        pv.x = rule_p(P, t); pv.y = rule_p(P, t + 1); pv.z = rule_p(P, t + 2); pv.w = rule_p(P, t + 3);
        if constexpr (HAS_P) *reinterpret_cast<float4 *>(A.p + e) = pv;
        if constexpr (HAS_G) {
            const float4 l = *reinterpret_cast<const float4 *>(A.load + e);
            float4 gv;
            gv.x = l.x + pv.x; gv.y = l.y + pv.y; gv.z = l.z + pv.z; gv.w = l.w + pv.w;
            *reinterpret_cast<float4 *>(A.g + e) = gv;
        }
    } else {
        const float pv = rule_p(P, t);
        if constexpr (HAS_P) A.p[e] = pv;
        if constexpr (HAS_G) A.g[e] = A.load[e] + pv;
    }
}

__global__ __launch_bounds__(kRuleNT) void rule_soc_kernel(RuleArgs A) {
    int64_t row, e;
    int t;
    rule_locate(A.T + 1, 1, row, t, e);
    if (row >= A.rows) return;
    const revs_home_t h = rule_record(A, row);
    const RulePlan P = rule_plan(h, A);
    A.soc[e] = rule_soc(P, t);
}

__global__ __launch_bounds__(kRuleNT) void rule_status_kernel(RuleArgs A) {
    const int64_t row = (int64_t)blockIdx.x * kRuleNT + threadIdx.x;
    if (row >= A.rows) return;
    const revs_home_t h = rule_record(A, row);
    A.status[row] = rule_plan(h, A).status;
}

}  // namespace revs

using namespace revs;

extern "C" int revs_rule_schedule(int64_t rows, int32_t T, const revs_home_t *homes, const float *load, int32_t policy,
                                  int32_t fill, int32_t integral, float *p_out, float *soc_out, float *g_out,
                                  int32_t *status_out, void *stream) {
    static_assert(sizeof(revs_home_t) == 32, "");
    const char *who = "revs_rule_schedule";
    REVS_REQUIRE(rows >= 1, "%s: rows=%lld < 1", who, (long long)rows);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    // one workgroup per 256 elements at the least: the grid of the widest array stays below 2^31 workgroups
    REVS_REQUIRE(rows <= (((int64_t)1 << 31) - 1) * (kRuleNT / 2) / (T + 1), "%s: rows=%lld times T=%d is beyond one launch",
                 who, (long long)rows, (int)T);
    REVS_REQUIRE(homes, "%s: null pointer argument homes", who);
    REVS_REQUIRE(policy == REVS_RULE_ASAP || policy == REVS_RULE_ALAP || policy == REVS_RULE_EVEN,
                 "%s: policy=%d is none of REVS_RULE_ASAP / _ALAP / _EVEN", who, (int)policy);
    REVS_REQUIRE(fill == REVS_FILL_TARGET || fill == REVS_FILL_FULL, "%s: fill=%d is neither REVS_FILL_TARGET nor _FULL",
                 who, (int)fill);
    REVS_REQUIRE(policy != REVS_RULE_EVEN || integral == 0,
                 "%s: policy REVS_RULE_EVEN with integral=%d (an on/off charger has no constant trickle power)", who,
                 (int)integral);
    REVS_REQUIRE(p_out || soc_out || g_out || status_out, "%s: every output is NULL (p_out, soc_out, g_out, status_out)", who);
    REVS_REQUIRE(!g_out || load, "%s: g_out without load", who);

    RuleArgs A;
    A.homes = homes; A.load = load; A.p = p_out; A.soc = soc_out; A.g = g_out; A.status = status_out;
    A.rows = rows; A.T = T; A.policy = policy; A.fill = fill; A.integral = integral ? 1 : 0;
    A.rec16 = ((uintptr_t)homes & 15) == 0 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(kRuleNT);
    if (p_out || g_out) {
        const uintptr_t bits = (uintptr_t)p_out | (uintptr_t)g_out | (g_out ? (uintptr_t)load : 0);
        const bool vec = T % 4 == 0 && (bits & 15) == 0;
        const int64_t per = vec ? 4 * kRuleNT : kRuleNT;
        const dim3 grid((unsigned)((rows * T + per - 1) / per));
#define REVS_RULE_PG(VEC)                                                                                      \
        do {                                                                                                   \
            if (p_out && g_out) hipLaunchKernelGGL((rule_pg_kernel<VEC, true, true>), grid, block, 0, st, A);  \
            else if (p_out) hipLaunchKernelGGL((rule_pg_kernel<VEC, true, false>), grid, block, 0, st, A);     \
            else hipLaunchKernelGGL((rule_pg_kernel<VEC, false, true>), grid, block, 0, st, A);                \
        } while (0)
        if (vec) REVS_RULE_PG(4);
        else REVS_RULE_PG(1);
#undef REVS_RULE_PG
        REVS_CHECK_LAUNCH(who);
    }
    if (soc_out) {
        const dim3 grid((unsigned)((rows * (T + 1) + kRuleNT - 1) / kRuleNT));
        hipLaunchKernelGGL(rule_soc_kernel, grid, block, 0, st, A);
        REVS_CHECK_LAUNCH(who);
    }
    if (status_out) {
        const dim3 grid((unsigned)((rows + kRuleNT - 1) / kRuleNT));
        hipLaunchKernelGGL(rule_status_kernel, grid, block, 0, st, A);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
