// The box-plot record's rules, each written once: the ordered keys of floats and doubles,
// numpy.percentile's interpolation, the quartiles' ranks, matplotlib.cbook.boxplot_stats' whiskers and fliers -- and what
// the reports' exact selections share on the device: counting into a histogram, the bin that holds a rank, and the
// radix selection of a workgroup over 64-bit keys (net_pool_kernel, bill_select_kernel).
//
// The scalar rules are __host__ __device__ and hold no lane or LDS operation: a host program can call them
// (tests/boxplot_rules_main.cpp).  Each of them rounds every operation on its own, as numpy does: contraction to fused
// multiply-adds is off INSIDE their bodies and nowhere else -- including this header changes nothing for the file that
// includes it.  (The _rn intrinsics of the HIP headers would not do: they are plain operators compiled under the
// headers' own contraction setting, and a product and a sum from them still fuse after inlining.)
#pragma once
#include "common.h"

namespace revs {

// ---- ordered keys: a < b  <=>  key(a) < key(b) for values that are no NaNs; -0.0 has +0.0's key
constexpr unsigned kBoxKey0F = 0x80000000u;       // box_key_f(+0.0f)
__host__ __device__ inline unsigned box_key_f(unsigned u) {       // u: a float's bits
    if (u == 0x80000000u) u = 0u;
    return (u >> 31) ? ~u : u | 0x80000000u;
}
__host__ __device__ inline double box_val_f(unsigned k) {
    return (double)__builtin_bit_cast(float, (k >> 31) ? k ^ 0x80000000u : ~k);
}
__host__ __device__ inline unsigned long long box_key(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v + 0.0);
    return (u >> 63) ? ~u : u | (1ull << 63);
}
__host__ __device__ inline double box_val(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) ? k ^ (1ull << 63) : ~k);
}

// ---- numpy.percentile's linear interpolation between the order statistics a <= b at fraction t (_lerp)
__host__ __device__ inline double box_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}
// quartile e = 1, 2, 3 (0 and 4: the extremes) of cnt values lies between the order statistics rank and rank + 1, rem4
// quarters of the way: (cnt - 1) e / 4 and its remainder
__host__ __device__ inline void box_rank(unsigned cnt, int e, unsigned &rank, unsigned &rem4) {
    const unsigned long long rr = cnt ? (unsigned long long)(cnt - 1) * (unsigned)e : 0ull;
    rank = (unsigned)(rr >> 2); rem4 = (unsigned)(rr & 3ull);
}
// The 32-bit selections count negatives and zeros first (the rows of a settled run are zeros for the most part): a rank
// that falls among the zeros is settled there -- its key, the rank left among the zeros, their number -- without a digit pass
__host__ __device__ inline bool box_settled_at_zero(unsigned rank, unsigned nneg, unsigned nzero, unsigned &ans,
                                                    unsigned &left, unsigned &eq) {
    if (rank < nneg || rank >= nneg + nzero) return false;
    ans = kBoxKey0F; left = rank - nneg; eq = nzero;
    return true;
}
// the order statistic above `rank` is another value than the one at `rank`, of which and below which there are cle:
// else it repeats, or (numpy clips the upper index to cnt - 1) there is none above
__host__ __device__ inline bool box_next_differs(unsigned rank, unsigned cnt, unsigned cle) {
    return rank + 1 < cnt && cle <= rank + 1;
}
__host__ __device__ inline double box_quartile(double lo, double hi, unsigned rem4) {
    return box_lerp(lo, hi, 0.25 * (double)rem4);
}
// ---- matplotlib.cbook.boxplot_stats at whis = 1.5: the product rounded, then the difference / the sum
__host__ __device__ inline void box_limits(double q1, double q3, double &lim_lo, double &lim_hi) {
#pragma clang fp contract(off)
    const double reach = 1.5 * (q3 - q1);
    lim_lo = q1 - reach; lim_hi = q3 + reach;
}
// a whisker is the farthest datum within the limit (cand; any: there is one) -- the box's edge when no datum lies inside
__host__ __device__ inline double box_whisker_lo(double q1, bool any, double cand) { return (!any || cand > q1) ? q1 : cand; }
__host__ __device__ inline double box_whisker_hi(double q3, bool any, double cand) { return (!any || cand < q3) ? q3 : cand; }
__host__ __device__ inline bool box_is_flier(double v, double wlo, double whi) { return v < wlo || v > whi; }

// ---- counting into LDS histograms, by whole wavefronts ----------------------------------------------------------------
// one count into h[d] per matching lane: by the first matching lane alone when the wavefront's digits agree (the common
// case in the top passes, where 64 atomics on one address would queue)
__device__ __forceinline__ void hist_add(unsigned *h, bool match, unsigned d) {
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
// the other policy: tab[idx] += 1 for every lane with `on`, one atomic per distinct idx of the wavefront for the first
// four, then per lane
__device__ __forceinline__ void conv_add(unsigned *tab, bool on, unsigned idx) {
    unsigned long long m = __ballot(on);
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll 1
    for (int it = 0; m != 0ull && it < 4; ++it) {
        const int first = (int)__builtin_ctzll(m);
        const unsigned i0 = (unsigned)__builtin_amdgcn_readlane((int)idx, first);
        const unsigned long long same = __ballot(on && idx == i0);
        if (lane == first) atomicAdd(tab + i0, (unsigned)__popcll(same));
        m &= ~same;
    }
    if ((m >> lane) & 1ull) atomicAdd(tab + idx, 1u);
}

// The bin of a 256-bin histogram (four counts per lane) that holds rank `want`, by one wavefront: every lane gets the
// bin, the rank inside the bin and the bin's count.
__device__ __forceinline__ void pick_bin(const uint4 cc, unsigned want, unsigned &bin, unsigned &left, unsigned &eq) {
    const int lane = threadIdx.x & 63;
    const unsigned own = cc.x + cc.y + cc.z + cc.w;
    unsigned incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
    }
    const unsigned excl = incl - own;
    const bool hit = want >= excl && want < incl;                 // (one lane: want < the histogram's total)
    unsigned b = 0, below = excl, cnt = cc.x;
    if (want >= below + cnt) { below += cnt; b = 1; cnt = cc.y; }
    if (b == 1 && want >= below + cnt) { below += cnt; b = 2; cnt = cc.z; }
    if (b == 2 && want >= below + cnt) { below += cnt; b = 3; cnt = cc.w; }
    const unsigned long long m = __ballot(hit);
    const int src = m ? (int)__builtin_ctzll(m) : 0;
    bin = (unsigned)__shfl((int)(4u * lane + b), src);
    left = (unsigned)__shfl((int)(want - below), src);
    eq = (unsigned)__shfl((int)cnt, src);
}

// ---- the selection of one workgroup of NT threads over 64-bit ordered keys --------------------------------------------
// The k-th smallest key by digits of 8 bits from the top: a pass counts, among the keys that share the prefix found so
// far, the next digit's 256 values in LDS; the three quartile ranks keep a prefix each and share a histogram while
// their prefixes agree.  The counts are integers: LDS atomics in any order give the same bits.  The last pass leaves,
// for free, the number of keys below and equal to each order statistic.
template <int NT>
struct BoxSelect {
    alignas(16) unsigned hist[3 * 256];
    double red[(NT / 64) * kBlockRed];            // block_reduce_multi's
    unsigned found[3][4];                         // per rank: digit, rank left inside the bin, the bin's count
};
struct BoxFigures { double q[3], wlo, whi; int n_fliers; };

// What follows the caller's pass 0, which has counted the kcnt > 0 sample values and left the top digit's histogram
// (key >> 56) in sh.hist[0 .. 255], the rest zero.  walk(f) calls f(key, ok, value, scenario, index) for every element,
// in every thread the same number of times (ok: part of the sample; key = box_key(value)); hook(key, ok, value,
// scenario, index) runs on every element of the neighbour walk: the caller's search for its worst entry.  Every thread
// of the workgroup calls it and gets the figures.  (An element that is not ok takes no part.  A walk whose keys and
// values keep such elements out by themselves -- a key with no prefix of an order statistic's, a NaN for the value --
// may call them ok.)
template <int NT, class Walk, class Hook>
__device__ __forceinline__ BoxFigures box_select64(BoxSelect<NT> &sh, int kcnt, Walk walk, Hook hook) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double ninf = -__builtin_inf();
    unsigned rank[3], rem4[3], left[3], eq[3] = {0u, 0u, 0u};     // left: among the keys that share the prefix; eq: keys equal to ans
    unsigned long long ans[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        box_rank((unsigned)kcnt, e + 1, rank[e], rem4[e]);
        left[e] = rank[e];
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
            walk([&](unsigned long long k, bool ok, double, int, int) {
                const unsigned long long pk = k >> (shift + 8);
                const unsigned d = (unsigned)(k >> shift) & 0xFFu;
                hist_add(sh.hist, ok && pk == p0, d);
                if (own1) hist_add(sh.hist + 256, ok && pk == p1, d);
                if (own2) hist_add(sh.hist + 512, ok && pk == p2, d);
            });
        }
        __syncthreads();
        if (wave < 3) {                           // wavefront e for rank e
            const uint4 c = *reinterpret_cast<const uint4 *>(sh.hist + 256 * slot[wave] + 4 * lane);
            unsigned bin, lf, cnt;
            pick_bin(c, left[wave], bin, lf, cnt);
            if (lane == 0) { sh.found[wave][0] = bin; sh.found[wave][1] = lf; sh.found[wave][2] = cnt; }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            ans[e] = uniform_u64(ans[e] | (unsigned long long)sh.found[e][0] << shift);     // (every lane holds the same)
            left[e] = __builtin_amdgcn_readfirstlane(sh.found[e][1]); eq[e] = __builtin_amdgcn_readfirstlane(sh.found[e][2]);
        }
        __syncthreads();                          // (every read of hist and found is done)
        for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
        __syncthreads();
    }
    // ---- the upper neighbours: the smallest value above each order statistic
    double nxt[3] = {ninf, ninf, ninf};
    walk([&](unsigned long long k, bool ok, double v, int s, int j) {
        if (ok) {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (k > ans[e]) nxt[e] = fmax(nxt[e], -v);
        }
        hook(k, ok, v, s, j);
    });
    block_reduce_multi<NT, 3, false>(nxt, sh.red);
    BoxFigures r;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double lo = box_val(ans[e]);
        const unsigned cle = rank[e] - left[e] + eq[e];             // keys <= the order statistic
        r.q[e] = box_quartile(lo, box_next_differs(rank[e], (unsigned)kcnt, cle) ? -nxt[e] : lo, rem4[e]);
    }
    // ---- whiskers: the farthest datum within 1.5 IQR of the box, then the fliers
    double lim0, lim1, wk[2] = {ninf, ninf};
    box_limits(r.q[0], r.q[2], lim0, lim1);
    walk([&](unsigned long long, bool ok, double v, int, int) {
        if (ok && v >= lim0) wk[0] = fmax(wk[0], -v);
        if (ok && v <= lim1) wk[1] = fmax(wk[1], v);
    });
    block_reduce_multi<NT, 2, false>(wk, sh.red);
    r.wlo = box_whisker_lo(r.q[0], wk[0] != ninf, -wk[0]);
    r.whi = box_whisker_hi(r.q[2], wk[1] != ninf, wk[1]);
    double fl[1] = {0.0};
    walk([&](unsigned long long, bool ok, double v, int, int) { fl[0] += (ok && box_is_flier(v, r.wlo, r.whi)) ? 1.0 : 0.0; });
    block_reduce_multi<NT, 1, true>(fl, sh.red);
    r.n_fliers = (int)fl[0];
    return r;
}

}  // namespace revs
