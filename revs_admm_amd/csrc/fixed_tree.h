// What the reports' fixed-order reductions share (DESIGN.md sections 3.16, 3.17): the root of a fixed binary tree over
// consecutive values, and the arg-max in (value down, index up) order over lanes.  Only additions and comparisons: their
// bits depend on no contraction setting, so including this header changes nothing for the file that includes it.
#pragma once
#include "common.h"

namespace revs {

// the root of the fixed binary tree over N consecutive values: x[i] = x[2i] + x[2i + 1], level by level
template <int N>
__device__ __forceinline__ double pair_tree(const double (&x)[N]) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = x[i];
#pragma unroll
    for (int w = N; w > 1; w >>= 1) {
#pragma unroll
        for (int i = 0; i < w / 2; ++i) y[i] = y[2 * i] + y[2 * i + 1];
    }
    return y[0];
}

// (value, index) pairs ordered for the arg-max: the larger value, then the lower index; index -1: no candidate
__device__ __forceinline__ void arg_better(double &bv, int &bi, double ov, int oi) {
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
}
__device__ __forceinline__ void wave_argmax(double &bv, int &bi) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        arg_better(bv, bi, ov, oi);
    }
}

}  // namespace revs
