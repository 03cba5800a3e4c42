// ep24 - pycocotools accumulate over the records ep24_eval_sort ordered: the one kernel behind ep24_eval_accumulate
// (evaluate.hip) and ep24_segm_accumulate (segmeval.hip), compiled once in each.
#pragma once
#include "wave_scan.h"

namespace {

constexpr int ACC_T = 10;            // IoU thresholds
constexpr int ACC_R = 101;           // recall thresholds

// grid (K, NA * NM): class k for area range a and max_dets[m].  A record beyond max_dets[m], or ignored at the threshold (bit
// 16 + t of its rec_m word), stays in the list with neither a TP nor an FP: it repeats its predecessor's (recall, precision)
// point, which neither the envelope nor the left search sees.  rec_key == null: no position filter, every record is inside every
// max_dets (max_dets may then be null too).  The 24-point evaluator is NA = NM = 1 with rec_m = its TP masks (no bit above 9)
// and no key: every record counts, the scanned TP + FP count at j is the integer j + 1.
// The records are ordered by class, so the workgroup finds its class's [first, last) itself: two searches over
// rec_cls[order[.]], in waves 0 and 1.

// The first j in [0, n) with rec_cls[order[j]] >= c, n if there is none; one wave, 64 probes a round (the probes of a round are
// loaded side by side: 3 rounds for 8 192 records where a binary search makes 13 dependent steps).  Below lo every class is < c,
// at hi it is >= c (or hi == n); lo and hi are the same in every lane.
__device__ __forceinline__ long long class_lower_bound(const int32_t* order, const int32_t* rec_cls, long long n, int c, int lane) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long step = (hi - lo + 63) >> 6, p = lo + lane * step;
        const unsigned long long ge = __ballot(p >= hi || rec_cls[order[p]] >= c);
        const int f = ge ? __ffsll((long long)ge) - 1 : 64;  // the first probe at or past the answer; probe f - 1 lies before it
        const long long top = lo + f * step;
        if (top < hi) hi = top;
        if (f) lo += (f - 1) * step + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void accumulate_kernel(const int32_t* order, const long long* rec_key, const int32_t* rec_cls,
                                                         const int32_t* rec_m, const int32_t* npig, int K, int NA, int NM,
                                                         const int32_t* max_dets, const double* rthr, long long n_all,
                                                         int32_t* ctp_all, double* env_all, double* precision, double* recall) {
    __shared__ long long range_sh[2];
    __shared__ int wsi[4];
    __shared__ double wsd[4];
    __shared__ int carry_tp, carry_n;
    __shared__ double carry_d;
    const int k = blockIdx.x, am = blockIdx.y, a = am / NM, m = am - a * NM;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long stride = (long long)K * NA * NM, col = ((long long)k * NA + a) * NM + m;
    const int np = npig[k * NA + a];
    if (np == 0) {                                            // no GT to find in this class and range: excluded (-1)
        for (int i = tid; i < ACC_T * ACC_R; i += 256) precision[(long long)i * stride + col] = -1.0;
        if (tid < ACC_T) recall[(long long)tid * stride + col] = -1.0;
        return;
    }
    if (w < 2) {                                              // the first record of class k (wave 0) and of the classes after it (wave 1)
        const long long j = class_lower_bound(order, rec_cls, n_all, k + w, lane);
        if (lane == 0) range_sh[w] = j;
    }
    __syncthreads();
    const long long s = range_sh[0], n = range_sh[1] - s;
    int32_t* ctp = ctp_all + (long long)am * n_all;
    double* env = env_all + (long long)am * n_all;
    const int md = rec_key ? max_dets[m] : 1;                 // without a key every position reads as 0
    const double dnp = (double)np;
    for (int t = 0; t < ACC_T; ++t) {
        // inclusive counts of TPs and of TPs + FPs; pr_j = tp / (tp + fp + eps).  Within a chunk of 1 024 records both fit 16 bits:
        // one int scan, TPs in the low half and TPs + FPs in the high half; the counts up to the chunk are two ints in LDS
        if (tid == 0) carry_tp = carry_n = 0;
        __syncthreads();
        for (long long b0 = 0; b0 < n; b0 += 1024) {
            // this thread's four records.  A position past the end reads the last record and counts nothing, so no load stands
            // under a branch and the four of a step are in flight together: three round trips a chunk, not three a record
            const long long j0 = b0 + tid * 4;
            int rec[4], mm[4], pos[4] = {0, 0, 0, 0}, v[4], sum = 0;
            for (int q = 0; q < 4; ++q) rec[q] = order[s + min(j0 + q, n - 1)];
            for (int q = 0; q < 4; ++q) mm[q] = rec_m[(long long)rec[q] * NA + a];
            if (rec_key)
                for (int q = 0; q < 4; ++q) pos[q] = (int)(rec_key[rec[q]] & 127);
            for (int q = 0; q < 4; ++q) {
                const bool in = j0 + q < n && pos[q] < md && !((mm[q] >> (16 + t)) & 1);
                v[q] = in ? (1 << 16) | ((mm[q] >> t) & 1) : 0;
                sum += v[q];
            }
            const int incl = wave_incl_sum(sum, lane);
            if (lane == 63) wsi[w] = incl;
            __syncthreads();
            int pre = incl - sum;
            for (int q = 0; q < w; ++q) pre += wsi[q];
            int tp = carry_tp + (pre & 0xFFFF), cnt = carry_n + (pre >> 16);
            for (int q = 0; q < 4; ++q) {
                const long long jj = j0 + q;
                tp += v[q] & 1;
                cnt += v[q] >> 16;
                if (jj < n) {
                    ctp[s + jj] = tp;
                    env[s + jj] = (double)tp / ((double)cnt + 2.220446049250313e-16);
                }
            }
            __syncthreads();
            if (tid == 0) {
                const int all = wsi[0] + wsi[1] + wsi[2] + wsi[3];
                carry_tp += all & 0xFFFF;
                carry_n += all >> 16;
            }
            __syncthreads();
        }
        // envelope: pr_j = max over i >= j (chunks from the right)
        if (tid == 0) carry_d = 0.0;
        __syncthreads();
        const long long nch = (n + 1023) / 1024;
        for (long long ch = nch - 1; ch >= 0; --ch) {
            const long long b0 = ch * 1024;
            double v[4];
            double mx = 0.0;
            for (int q = 3; q >= 0; --q) {
                const long long jj = b0 + tid * 4 + q;
                v[q] = jj < n ? env[s + jj] : 0.0;
                mx = fmax(mx, v[q]);
            }
            const double incl = wave_suffix_max(mx, lane);    // over this lane and the lanes above it
            if (lane == 0) wsd[w] = incl;
            __syncthreads();
            double run = carry_d;
            for (int q = w + 1; q < 4; ++q) run = fmax(run, wsd[q]);
            const double above = __shfl_down(incl, 1, 64);
            if (lane < 63) run = fmax(run, above);
            for (int q = 3; q >= 0; --q) {
                const long long jj = b0 + tid * 4 + q;
                run = fmax(run, v[q]);
                if (jj < n) env[s + jj] = run;
            }
            __syncthreads();
            if (tid == 0) carry_d = fmax(fmax(fmax(carry_d, wsd[0]), fmax(wsd[1], wsd[2])), wsd[3]);
            __syncthreads();
        }
        // the 101 recall thresholds: precision at the first j with rc_j >= r (searchsorted 'left'), 0 past the end
        if (tid < ACC_R) {
            const double rt = rthr[tid];
            long long lo = 0, hi = n;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if ((double)ctp[s + mid] / dnp >= rt) hi = mid; else lo = mid + 1;
            }
            precision[((long long)t * ACC_R + tid) * stride + col] = lo < n ? env[s + lo] : 0.0;
        }
        if (tid == 0) recall[(long long)t * stride + col] = n ? (double)ctp[s + n - 1] / dnp : 0.0;
        __syncthreads();
    }
}

// ctp_scratch [NA * NM][n] int32, env_scratch [NA * NM][n] double; the entry points check the arguments
void launch_accumulate(const int32_t* order, const int64_t* rec_key, const int32_t* rec_cls, const int32_t* rec_m, int64_t n,
                       const int32_t* npig, int K, int NA, const int32_t* max_dets, int NM, const double* rec_thr,
                       int32_t* ctp_scratch, double* env_scratch, double* precision, double* recall, hipStream_t stream) {
    hipLaunchKernelGGL(accumulate_kernel, dim3(K, NA * NM), dim3(256), 0, stream, order, (const long long*)rec_key, rec_cls, rec_m, npig,
                       K, NA, NM, max_dets, rec_thr, (long long)n, ctp_scratch, env_scratch, precision, recall);
}

}  // namespace
