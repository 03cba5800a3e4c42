// ep24 - scans over the 64 lanes of a wave by shuffles, shared by the radix sort's scan (evaluate.hip), the accumulate kernel
// (accumulate.h) and the RLE scans (rle.hip).  The step across waves differs per site and stays there.
#pragma once
#include "common.h"

// v of this lane and of every lane below it (int or long long: exact)
template <typename T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T x = __shfl_up(v, o, 64);
        if (lane >= o) v += x;
    }
    return v;
}

// the largest v of this lane and of every lane above it (fmax is exact)
__device__ __forceinline__ double wave_suffix_max(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double x = __shfl_down(v, o, 64);
        if (lane + o < 64) v = fmax(v, x);
    }
    return v;
}
