// ep24 - evaluation of 24-point detections: COCO-style AP (the evaluateImg + accumulate semantics of pycocotools for one
// area range "all", no crowd / ignore regions, one maxDets) with matching and accumulation on the GPU.
//
//   eval_iou      pairwise IoU matrix [G][D] (double) of GT rows against detections, for tests and for the host API
//                 (circle24 and rect in 26 floats of geometry per object; poly24, the exact area IoU of poly24.h, in 48)
//   eval_match    the STRATA = false instance of eval_match_kernel (evalgeom.h): one workgroup per image: GT count / geometry into
//                 LDS, the image's detections sorted by (class, score desc, p asc) in global scratch, then one wave per class
//                 segment greedily matches the first max_dets detections against the class's GTs for all 10 IoU thresholds and
//                 appends one record per detection
//   eval_sort     stable LSD radix sort of the records by (class, score desc, image seq, rank)
//   eval_accumulate  the accumulate kernel of accumulate.h (shared with segmeval.hip) for one area range and one maxDets: one
//                 workgroup per class finds its records in the sorted order, then cumulative TP / FP counts, precision envelope
//                 and the 101 recall look-ups in double
//
// Determinism: the only atomics are integer ones whose order does not matter - the GT count per class (a sum) and the
// append offset of a class segment's records (the sort key fixes the final order; (class, seq, rank) is unique).
// No floating-point atomics anywhere.
//
// The geometry, the pair IoUs, the match kernel and its host-side check live in evalgeom.h, shared with the evaluation by strata
// (evalstrata.hip).
#include "accumulate.h"
#include "evalgeom.h"

namespace {

// GW = floats of geometry per object: 26 for circle24 / rect, 48 for poly24
template <int GW>
__global__ __launch_bounds__(256) void eval_iou_kernel(const float* gt50, const float* det26, int G, int D, int iou_type,
                                                       const float* cs, double* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)G * D) return;
    const int g = (int)(i / D), d = (int)(i - (long)g * D);
    float gg[GW], qq[GW];
    gt_geometry<GW>(gt50 + (long)g * 50, iou_type, gg);
    det_geometry<GW>(det26 + (long)d * 26, iou_type, cs, qq);
    out[i] = pair_iou<GW>(gg, qq, iou_type);
}

// ---------------------------------------------------------------------------------------------- radix sort of the records
// Stable LSD passes of 8 bits over the 96-bit value (class << 64 | key); tile of EV_TILE records per workgroup.
constexpr int EV_TILE = 4096;

__device__ __forceinline__ int digit_of(int64_t k, int32_t c, int shift) {
    return shift < 64 ? (int)(((uint64_t)k >> shift) & 255u) : (int)(((uint32_t)c >> (shift - 64)) & 255u);
}

__global__ __launch_bounds__(256) void radix_hist_kernel(const int64_t* key, const int32_t* cls, int64_t n, int shift, int nblk,
                                                         int32_t* hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * EV_TILE;
    for (int r = 0; r < EV_TILE / 256; ++r) {
        const int64_t i = base + r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[digit_of(key[i], cls[i], shift)], 1);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// exclusive prefix sum of m int32 counts, one workgroup of 1024 (each thread 4 consecutive entries per chunk of 4096)
__global__ __launch_bounds__(1024) void scan_excl_kernel(int32_t* a, int64_t m) {
    __shared__ int ws[16];
    __shared__ int carry_sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry_sh = 0;
    __syncthreads();
    for (int64_t base = 0; base < m; base += 4096) {
        int v[4], s = 0;
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + tid * 4 + q;
            v[q] = i < m ? a[i] : 0;
            s += v[q];
        }
        const int incl = wave_incl_sum(s, lane);
        if (lane == 63) ws[w] = incl;
        __syncthreads();
        int pre = carry_sh;
        for (int q = 0; q < w; ++q) pre += ws[q];
        int run = pre + incl - s;
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + tid * 4 + q;
            if (i < m) a[i] = run;
            run += v[q];
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int q = 0; q < 16; ++q) t += ws[q];
            carry_sh += t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void radix_scatter_kernel(const int64_t* key, const int32_t* cls, const int32_t* idx, int64_t n,
                                                            int shift, int nblk, const int32_t* hist, int64_t* key_o, int32_t* cls_o,
                                                            int32_t* idx_o) {
    __shared__ int off[256];
    __shared__ int wc[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    off[tid] = hist[(int64_t)tid * nblk + blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * EV_TILE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < EV_TILE / 256; ++r) {
        for (int q = 0; q < 4; ++q) wc[q][tid] = 0;
        __syncthreads();
        const int64_t i = base + r * 256 + tid;
        const bool valid = i < n;
        int64_t k = 0;
        int32_t c = 0, x = 0;
        int d = 0;
        if (valid) {
            k = key[i];
            c = cls[i];
            x = idx ? idx[i] : (int32_t)i;
            d = digit_of(k, c, shift);
        }
        unsigned long long mm = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bb = __ballot((d >> bit) & 1);
            mm &= ((d >> bit) & 1) ? bb : ~bb;
        }
        const int rank = __popcll(mm & lt);
        if (valid && rank == 0) wc[w][d] = __popcll(mm);
        __syncthreads();
        if (valid) {
            int pos = off[d] + rank;
            for (int q = 0; q < w; ++q) pos += wc[q][d];
            key_o[pos] = k;
            cls_o[pos] = c;
            idx_o[pos] = x;
        }
        __syncthreads();
        off[tid] += wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
        __syncthreads();
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_eval_iou(const float* gt50, const float* det26, int G, int D, int iou_type, const float* ray_cs, double* out,
                             void* stream) {
    if ((long)G * D == 0) return EP24_OK;
    EP24_REQUIRE(gt50 && det26 && ray_cs && out && G > 0 && D > 0, EP24_E_ARG, "eval_iou: bad arguments");
    EP24_REQUIRE(iou_type >= 0 && iou_type <= 2, EP24_E_UNSUPPORTED, "eval_iou: iou_type %d (0 circle24, 1 rect, 2 poly24)", iou_type);
    const dim3 grid((unsigned)(((long)G * D + 255) / 256));
    if (iou_type == 2)
        hipLaunchKernelGGL(eval_iou_kernel<48>, grid, dim3(256), 0, S_, gt50, det26, G, D, iou_type, ray_cs, out);
    else
        hipLaunchKernelGGL(eval_iou_kernel<26>, grid, dim3(256), 0, S_, gt50, det26, G, D, iou_type, ray_cs, out);
    EP24_LAUNCH_CHECK("ep24_eval_iou");
    return EP24_OK;
}

extern "C" int ep24_eval_match(const float* labels, int L, int B, const float* rows, int ncols, const int64_t* row_off,
                               const int32_t* keep, int64_t keep_stride, const int32_t* count, const float* conf, const int32_t* cls,
                               int num_classes, int iou_type, const float* ray_cs, const double* iou_thr, int max_dets,
                               int64_t seq_base, int64_t* sort_scratch, int P, int64_t* rec_key, int32_t* rec_cls, int32_t* rec_p,
                               int32_t* rec_tp, int32_t* rec_count, int32_t* npig, int32_t* err, void* stream) {
    return eval_match_launch("eval_match", labels, L, B, rows, ncols, row_off, keep, keep_stride, count, conf, cls, num_classes, iou_type,
                             ray_cs, iou_thr, max_dets, seq_base, sort_scratch, P, StrataArgs<false>{}, rec_key, rec_cls, rec_p, rec_tp,
                             rec_count, npig, err, S_);
}

extern "C" int ep24_eval_sort(const int64_t* key, const int32_t* cls, int64_t n, int key_low_bits, int cls_bits, int64_t* key_tmp,
                              int32_t* cls_tmp, int32_t* idx_tmp, int32_t* hist, int32_t* order, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(key && cls && key_tmp && cls_tmp && idx_tmp && hist && order && n > 0, EP24_E_ARG, "eval_sort: bad arguments");
    EP24_REQUIRE(n <= 0x7FFFFFFFLL, EP24_E_UNSUPPORTED, "eval_sort: %lld records (at most 2^31 - 1)", (long long)n);
    EP24_REQUIRE(key_low_bits >= 0 && key_low_bits <= 32 && cls_bits >= 0 && cls_bits <= 32, EP24_E_ARG, "eval_sort: bit counts");
    const int nblk = (int)((n + EV_TILE - 1) / EV_TILE);
    int shifts[16], np = 0;
    for (int sft = 0; sft < key_low_bits; sft += 8) shifts[np++] = sft;
    for (int sft = 32; sft < 64; sft += 8) shifts[np++] = sft;
    for (int sft = 0; sft < cls_bits; sft += 8) shifts[np++] = 64 + sft;
    const int64_t* kin = key;
    const int32_t* cin = cls;
    const int32_t* iin = nullptr;
    for (int p = 0; p < np; ++p) {
        int64_t* ko = key_tmp + (p & 1) * n;
        int32_t* co = cls_tmp + (p & 1) * n;
        int32_t* io = (p == np - 1) ? order : idx_tmp + (p & 1) * n;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(256), 0, S_, kin, cin, n, shifts[p], nblk, hist);
        hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, S_, hist, (int64_t)256 * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(256), 0, S_, kin, cin, iin, n, shifts[p], nblk, hist, ko, co, io);
        kin = ko;
        cin = co;
        iin = io;
    }
    EP24_LAUNCH_CHECK("ep24_eval_sort");
    return EP24_OK;
}

extern "C" int ep24_eval_accumulate(const int32_t* order, const int32_t* rec_cls, const int32_t* rec_tp, int64_t n, const int32_t* npig,
                                    int num_classes, const double* rec_thr, int64_t* cls_range, int32_t* ctp_scratch,
                                    double* env_scratch, double* precision, double* recall, void* stream) {
    EP24_REQUIRE(npig && rec_thr && precision && recall && num_classes > 0, EP24_E_ARG, "eval_accumulate: bad arguments");
    EP24_REQUIRE(n == 0 || (order && rec_cls && rec_tp && ctp_scratch && env_scratch), EP24_E_ARG, "eval_accumulate: null record buffer");
    // one area range, one maxDets, no ignore bits, no position filter: rec_tp is the rec_m of accumulate.h
    launch_accumulate(order, nullptr, rec_cls, rec_tp, n, npig, num_classes, 1, nullptr, 1, rec_thr, ctp_scratch, env_scratch, precision,
                      recall, S_);
    EP24_LAUNCH_CHECK("ep24_eval_accumulate");
    return EP24_OK;
}
