// ep24 - the candidate list of NMS, shared by nms_kernel (infer.hip) and the polygon NMS (polynms.hip).
#pragma once
#include "common.h"

// One workgroup of NT threads per image: compact the rows with sc >= 0 (post_prepare writes -1 below conf_thre; a NaN score is
// no candidate) into key / idx and bitonic-sort them by (score desc, index asc) in global scratch.  The order is total, so the
// result does not depend on the order the atomics compacted the rows in.  Returns the number of candidates; key / idx hold them
// in [0, n) and padding up to the next power of two.  n_sh: one int of LDS.
template <int NT>
__device__ __forceinline__ int nms_compact_sort(const float* sc, int A, float* key, int* idx, int* n_sh) {
    const int tid = threadIdx.x;
    if (tid == 0) *n_sh = 0;
    __syncthreads();
    for (int a = tid; a < A; a += NT)
        if (sc[a] >= 0.f) { const int j = atomicAdd(n_sh, 1); key[j] = sc[a]; idx[j] = a; }
    __syncthreads();
    const int n = *n_sh;
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    for (int j = n + tid; j < P2; j += NT) { key[j] = -2.0f; idx[j] = 0x7FFFFFFF; }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;          // "up" blocks hold the better (earlier) elements first
                    const float ki = key[i], kl = key[l];
                    const int ii = idx[i], il = idx[l];
                    const bool i_first = ki > kl || (ki == kl && ii < il);
                    if (up != i_first) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
                }
            }
            __syncthreads();
        }
    return n;
}
