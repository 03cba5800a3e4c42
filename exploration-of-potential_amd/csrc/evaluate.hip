// ep24 - evaluation of 24-point detections: COCO-style AP (the evaluateImg + accumulate semantics of pycocotools for one
// area range "all", no crowd / ignore regions, one maxDets) with matching and accumulation on the GPU.
//
//   eval_iou      pairwise IoU matrix [G][D] (double) of GT rows against detections, for tests and for the host API
//                 (circle24 and rect in 26 floats of geometry per object; poly24, the exact area IoU of poly24.h, in 48)
//   eval_match    one workgroup per image: GT count / geometry into LDS, the image's detections sorted by (class, score desc,
//                 p asc) in global scratch, then one wave per class segment greedily matches the first max_dets detections
//                 against the class's GTs for all 10 IoU thresholds and appends one record per detection
//   eval_sort     stable LSD radix sort of the records by (class, score desc, image seq, rank)
//   eval_accumulate  the accumulate kernel of accumulate.h (shared with segmeval.hip) for one area range and one maxDets: one
//                 workgroup per class finds its records in the sorted order, then cumulative TP / FP counts, precision envelope
//                 and the 101 recall look-ups in double
//
// Determinism: the only atomics are integer ones whose order does not matter - the GT count per class (a sum) and the
// append offset of a class segment's records (the sort key fixes the final order; (class, seq, rank) is unique).
// No floating-point atomics anywhere.
//
// The geometry, the pair IoUs, det_row and the per-image sort live in evalgeom.h, shared with the matcher by strata (evalstrata.hip).
#include "accumulate.h"
#include "evalgeom.h"

namespace {

// GW = floats of geometry per object: 26 for circle24 / rect (the kernels as they were), 48 for poly24.  GS = the LDS row stride
// of the match kernel: 49 for poly24, so that the 64 lanes' rows fall into different banks.
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

template <int GW>
__global__ __launch_bounds__(256) void eval_match_kernel(const float* labels, int L, DetSrc src, const int32_t* count, int C,
                                                         int iou_type, const float* cs, const double* thr, int max_dets,
                                                         int64_t seq_base, uint64_t* skey, int P, int64_t* rec_key,
                                                         int32_t* rec_cls, int32_t* rec_p, int32_t* rec_tp, int32_t* rec_count,
                                                         int32_t* npig, int32_t* err) {
    constexpr int GS = GW == 48 ? 49 : GW;
    __shared__ float g_geo[EV_MAX_L][GS];
    __shared__ int g_cls[EV_MAX_L];
    __shared__ double thr_sh[EV_T];
    __shared__ float cs_sh[48];
    __shared__ int n_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* lab = labels + (long)b * L * EP24_LABEL_COLS;
    // GT rows: the first n, n = rows whose 51 values sum to > 0 (losses.py:190, as count_gt in assign.hip)
    if (tid == 0) n_sh = 0;
    if (tid < EV_T) thr_sh[tid] = fmin(thr[tid], 1.0 - 1e-10);
    if (tid < 48) cs_sh[tid] = cs[tid];
    __syncthreads();
    for (int r = tid; r < L; r += 256) {
        float s = 0.f;
        for (int c = 0; c < EP24_LABEL_COLS; ++c) s += lab[r * EP24_LABEL_COLS + c];
        if (s > 0.f) atomicAdd(&n_sh, 1);
    }
    __syncthreads();
    const int ng = n_sh;
    for (int i = tid; i < ng; i += 256) {
        const float* t = lab + (long)i * EP24_LABEL_COLS;
        const int c = (t[0] >= 0.f && t[0] < (float)C) ? (int)t[0] : -1;
        g_cls[i] = c;
        if (c >= 0) atomicAdd(&npig[c], 1);
        gt_geometry<GW>(t + 1, iou_type, g_geo[i]);
    }
    const int nd = count[b];
    if (nd > P || nd < 0) {                               // host sizes P from the plan; never expected
        if (tid == 0) atomicOr(err, 1);
        return;
    }
    // the image's detections in (class, score desc, p asc) order: bitonic sort of 64-bit keys in global scratch
    uint64_t* key = skey + (long)b * P;
    sort_image_dets(src, b, nd, C, key, tid);
    // one wave per class segment (segments dealt round-robin in sorted order)
    const int64_t seq = seq_base + b;
    int hcount = 0;
    for (int base = 0; base < nd; base += 64) {
        const int j = base + lane;
        const uint64_t kj = j < nd ? key[j] : ~0ull;
        const int cj = (int)(kj >> 48);
        const int cp = (j > 0 && j < nd) ? (int)(key[j - 1] >> 48) : -1;
        unsigned long long hm = __ballot(j < nd && cj != cp && cj != EV_NONE);
        while (hm) {
            const int hl = __ffsll((long long)hm) - 1;
            hm &= hm - 1;
            if ((hcount++ & 3) != w) continue;
            const int s0 = base + hl;
            const int c = __shfl(cj, hl, 64);
            // kept detections: the first min(len, max_dets) of the segment
            int m = 0;
            for (int q = 0; q < max_dets; q += 64) {
                const int jj = s0 + q + lane;
                const bool in = q + lane < max_dets && jj < nd && (int)(key[jj] >> 48) == c;
                m += __popcll(__ballot(in));
            }
            // this lane's GTs of class c: rows lane, lane + 64, lane + 128, lane + 192
            bool has[4];
            bool any = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = q * 64 + lane;
                has[q] = gi < ng && g_cls[gi] == c;
                any |= has[q];
            }
            any = __ballot(any) != 0;
            int rbase = 0;
            if (lane == 0) rbase = atomicAdd(rec_count, m);
            rbase = __shfl(rbase, 0, 64);
            unsigned matched[4] = {0u, 0u, 0u, 0u};
            for (int r = 0; r < m; ++r) {
                const uint64_t kr = key[s0 + r];
                const int p = (int)(kr & 0xFFFF);
                const uint32_t sbits = (uint32_t)(kr >> 16);
                int tpm = 0;
                if (any) {
                    float sc;
                    int cc;
                    const float* row = det_row(src, b, p, sc, cc, C);
                    float qg[GW];
                    det_geometry<GW>(row, iou_type, cs_sh, qg);
                    double iou[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) iou[q] = has[q] ? pair_iou<GW>(g_geo[q * 64 + lane], qg, iou_type) : -1.0;
                    for (int t = 0; t < EV_T; ++t) {
                        // pycocotools: the largest IoU >= min(t, 1 - 1e-10) among unmatched GTs, equal IoUs -> the later GT row
                        double best = thr_sh[t];
                        int bg = -1;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (has[q] && !((matched[q] >> t) & 1u) && iou[q] >= best) { best = iou[q]; bg = q * 64 + lane; }
                        if (__ballot(bg >= 0) == 0) continue;
                        for (int o = 32; o > 0; o >>= 1) {
                            const double ob = __shfl_xor(best, o, 64);
                            const int og = __shfl_xor(bg, o, 64);
                            if (og >= 0 && (bg < 0 || ob > best || (ob == best && og > bg))) { best = ob; bg = og; }
                        }
                        tpm |= 1 << t;
                        if ((bg & 63) == lane) matched[bg >> 6] |= 1u << t;
                    }
                }
                if (lane == 0) {
                    const int64_t o = (int64_t)rbase + r;
                    rec_key[o] = (int64_t)(((uint64_t)sbits << 32) | ((uint64_t)seq << 7) | (uint64_t)r);
                    rec_cls[o] = c;
                    rec_p[o] = p;
                    rec_tp[o] = tpm;
                }
            }
        }
    }
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
    if (B == 0) return EP24_OK;
    EP24_REQUIRE(labels && rows && row_off && count && ray_cs && iou_thr && sort_scratch && rec_key && rec_cls && rec_p && rec_tp &&
                 rec_count && npig && err && B > 0 && P > 0, EP24_E_ARG, "eval_match: bad arguments");
    EP24_REQUIRE((conf == nullptr) == (cls == nullptr), EP24_E_ARG, "eval_match: conf and cls come together");
    EP24_REQUIRE(ncols >= (conf ? 27 : 29), EP24_E_ARG, "eval_match: ncols=%d", ncols);
    EP24_REQUIRE(L >= 0 && L <= EV_MAX_L, EP24_E_UNSUPPORTED, "eval_match: %d GT rows per image (at most %d)", L, EV_MAX_L);
    EP24_REQUIRE(max_dets > 0 && max_dets <= EV_MAX_DETS, EP24_E_UNSUPPORTED, "eval_match: max_dets=%d (1..%d)", max_dets, EV_MAX_DETS);
    EP24_REQUIRE(num_classes > 0 && num_classes < EV_NONE, EP24_E_UNSUPPORTED, "eval_match: num_classes=%d (1..%d)", num_classes,
                 EV_NONE - 1);
    EP24_REQUIRE(P <= 65536 && (P & (P - 1)) == 0, EP24_E_UNSUPPORTED, "eval_match: P=%d (a power of two, at most 65536 detections per image)", P);
    EP24_REQUIRE(seq_base >= 0 && seq_base + B <= (1LL << 25), EP24_E_UNSUPPORTED, "eval_match: image sequence %lld + %d beyond 2^25",
                 (long long)seq_base, B);
    EP24_REQUIRE(iou_type >= 0 && iou_type <= 2, EP24_E_UNSUPPORTED, "eval_match: iou_type %d (0 circle24, 1 rect, 2 poly24)", iou_type);
    DetSrc src{rows, ncols, row_off, keep, keep_stride, conf, cls};
    if (iou_type == 2)
        hipLaunchKernelGGL(eval_match_kernel<48>, dim3(B), dim3(256), 0, S_, labels, L, src, count, num_classes, iou_type, ray_cs,
                           iou_thr, max_dets, seq_base, (uint64_t*)sort_scratch, P, rec_key, rec_cls, rec_p, rec_tp, rec_count, npig, err);
    else
        hipLaunchKernelGGL(eval_match_kernel<26>, dim3(B), dim3(256), 0, S_, labels, L, src, count, num_classes, iou_type, ray_cs,
                           iou_thr, max_dets, seq_base, (uint64_t*)sort_scratch, P, rec_key, rec_cls, rec_p, rec_tp, rec_count, npig, err);
    EP24_LAUNCH_CHECK("ep24_eval_match");
    return EP24_OK;
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
