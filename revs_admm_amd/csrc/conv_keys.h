// The ordered keys of floats, numpy.percentile's interpolation and the per-address counting of a wavefront: what the
// exact selections of the convergence report (convergence_kernels.hip) and the load-profile report
// (load_profile_kernels.hip) share.
#pragma once
#include "common.h"

// Quartiles interpolate as numpy.percentile does, every operation rounded on its own: no fused multiply-adds.
#pragma clang fp contract(off)

namespace revs {

constexpr unsigned kConvKey0 = 0x80000000u;       // conv_key(+0.0f)

// a < b  <=>  conv_key(a) < conv_key(b) for floats that are no NaNs; -0.0 has +0.0's key
__device__ __forceinline__ unsigned conv_key(unsigned u) {
    if (u == 0x80000000u) u = 0u;
    return (u >> 31) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ double conv_val(unsigned k) {
    return (double)__uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k);
}
__device__ __forceinline__ double conv_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double conv_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double conv_addd(double a, double b) { return a + b; }
// numpy.percentile's _lerp
__device__ __forceinline__ double conv_lerp(double a, double b, double t) {
    const double d = conv_sub(b, a);
    return t >= 0.5 ? conv_sub(b, conv_mul(d, conv_sub(1.0, t))) : conv_addd(a, conv_mul(d, t));
}

// tab[idx] += 1 for every lane with `on`: one atomic per distinct idx of the wavefront for the first four, then per lane.
// Called by whole wavefronts.
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

}  // namespace revs
