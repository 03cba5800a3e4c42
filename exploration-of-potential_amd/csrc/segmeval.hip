// ep24 - COCO "segm" evaluation: the bookkeeping of pycocotools' COCOeval for iouType = "segm" on packed instance masks
// (include/ep24.h section E6; ep24.segmeval.SegmEvaluator).
//
//   segm_mask_stats   one workgroup per mask of a ragged table: box of the set pixels and their number, reduced in registers and LDS
//                     (no atomics, every output word written)
//   segm_iou          one wave per (detection, GT) pair of a group table: AND + popcount over the rows and words where the two boxes
//                     overlap, then ONE double division of exact integers - inter / area(DT) for a crowd GT, inter / union otherwise
//                     (rleIou); the wave finds its group by a binary search over the table's running offsets
//   segm_match        one wave per (image, category) group: evaluateImg for every area range and IoU threshold.  Lanes own GTs
//                     (g = lane, lane + 64, ...), detections are walked in the host's order; the first 64 GTs' state lives in
//                     registers, GTs beyond them keep their matched bits in caller scratch (one int64 per GT)
//   segm_accumulate   the accumulate kernel of accumulate.h (shared with evaluate.hip): one workgroup per (class, area range,
//                     maxDets) over the records ep24_eval_sort ordered: cumulative TP / valid counts, precision envelope from
//                     the right, the 101 recall look-ups, all in double
//
// Determinism: the only atomics are the integer sums of non-ignored GTs per (class, area range).  Records are written at the
// detection's own index, so nothing is appended.  No floating-point atomics.
#include "accumulate.h"

namespace {

constexpr int SE_T = 10;             // IoU thresholds
constexpr int SE_MAX_A = 4;          // area ranges: SE_MAX_A * SE_T matched bits fit one int64
constexpr int SE_MAX_M = 4;          // maxDets values
constexpr int SE_MAX_DETS = 128;     // detections per group: the rank takes 7 bits of the record key

// ---------------------------------------------------------------------------------------------- mask statistics
__global__ __launch_bounds__(256) void segm_mask_stats_kernel(const uint32_t* bits, const long long* tab, long N, int32_t* bbox,
                                                              int32_t* area) {
    __shared__ int sh[4][5];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long n = blockIdx.x; n < N; n += gridDim.x) {       // the trip count is the workgroup's: barriers inside are uniform
        const long long* t = tab + n * 4;
        const long long word0 = t[0], H = t[1], W = t[2];
        const bool ok = word0 >= 0 && H > 0 && W > 0 && H * W < (1LL << 31);
        int cnt = 0, xlo = ok ? (int)W : 0, ylo = ok ? (int)H : 0, xhi = -1, yhi = -1;
        if (ok) {
            const int WW = (int)((W + 31) >> 5);
            const long cells = (long)H * WW;
            const uint32_t* p = bits + word0;
            for (long i = tid; i < cells; i += 256) {
                const uint32_t word = p[i];
                if (word) {
                    const int y = (int)(i / WW), xw = (int)(i - (long)y * WW);
                    cnt += __popc(word);
                    xlo = min(xlo, 32 * xw + __ffs((int)word) - 1);
                    xhi = max(xhi, 32 * xw + 31 - __clz((int)word));
                    ylo = min(ylo, y);
                    yhi = max(yhi, y);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            xlo = min(xlo, __shfl_xor(xlo, o, 64));
            ylo = min(ylo, __shfl_xor(ylo, o, 64));
            xhi = max(xhi, __shfl_xor(xhi, o, 64));
            yhi = max(yhi, __shfl_xor(yhi, o, 64));
        }
        if (lane == 0) {
            sh[w][0] = cnt; sh[w][1] = xlo; sh[w][2] = ylo; sh[w][3] = xhi; sh[w][4] = yhi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q) {
                cnt += sh[q][0];
                xlo = min(xlo, sh[q][1]);
                ylo = min(ylo, sh[q][2]);
                xhi = max(xhi, sh[q][3]);
                yhi = max(yhi, sh[q][4]);
            }
            bbox[4 * n] = xlo;
            bbox[4 * n + 1] = ylo;
            bbox[4 * n + 2] = xhi;
            bbox[4 * n + 3] = yhi;
            area[n] = cnt;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- mask IoU of a group table
__global__ __launch_bounds__(256) void segm_iou_kernel(const uint32_t* bits, const long long* tab, long long N, const int32_t* bbox,
                                                       const int32_t* area, const uint8_t* crowd, const long long* grp, int J,
                                                       long long p0, long long pairs, double* iou, long long* inter) {
    const int lane = threadIdx.x & 63;
    const long long p = p0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= pairs) return;                                   // whole waves leave together
    // the last group whose first entry is at or before p (groups without pairs share their successor's offset)
    const long long base = grp[6];
    int lo = 0, hi = J - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (grp[(long)mid * 8 + 6] - base <= p) lo = mid; else hi = mid - 1;
    }
    const long long* t = grp + (long)lo * 8;
    const long long H = t[0], W = t[1], g0 = t[2], G = t[3], d0 = t[4], D = t[5], off = t[6];
    const long long q = p - (off - base);
    if (G <= 0 || D <= 0 || q < 0 || q >= G * D || H <= 0 || W <= 0 || H * W >= (1LL << 31)) return;
    const long long d = q / G, g = q - d * G;
    const long long mg = g0 + g, md = d0 + d;
    if (g0 < 0 || d0 < 0 || g0 + G > N || d0 + D > N) return;   // a group that names masks outside the table: nothing read or written
    const long long* tg = tab + mg * 4;
    const long long* td = tab + md * 4;
    long long cnt = 0;
    // a pair whose table rows are not the group's size reads no mask word
    if (tg[1] == H && tg[2] == W && td[1] == H && td[2] == W && tg[0] >= 0 && td[0] >= 0) {
        const int x0 = max(max(bbox[4 * mg], bbox[4 * md]), 0), y0 = max(max(bbox[4 * mg + 1], bbox[4 * md + 1]), 0);
        const int x1 = min(min(bbox[4 * mg + 2], bbox[4 * md + 2]), (int)W - 1);
        const int y1 = min(min(bbox[4 * mg + 3], bbox[4 * md + 3]), (int)H - 1);
        if (x0 <= x1 && y0 <= y1) {
            const int WW = (int)((W + 31) >> 5);
            const int w0 = x0 >> 5, nw = (x1 >> 5) - w0 + 1;
            const long cells = (long)(y1 - y0 + 1) * nw;
            const uint32_t* pa = bits + tg[0];
            const uint32_t* pb = bits + td[0];
            for (long i = lane; i < cells; i += 64) {
                const long r = i / nw;
                const long o = (y0 + r) * WW + w0 + (i - r * nw);
                cnt += __popc(pa[o] & pb[o]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        }
    }
    if (lane == 0) {
        const long long ad = area[md];
        const long long den = crowd[mg] ? ad : (long long)area[mg] + ad - cnt;
        iou[off + q] = cnt != 0 ? (double)cnt / (double)den : 0.0;
        if (inter) inter[off + q] = cnt;
    }
}

// ---------------------------------------------------------------------------------------------- evaluateImg
// A candidate GT of one detection at one (area range, threshold): the reference walks the GTs with the non-ignored first and stops
// at the first ignored one once it holds a non-ignored match, taking every GT whose IoU is >= the best so far.  That is: the largest
// IoU among the non-ignored candidates, else among the ignored ones, equal IoUs going to the later GT.
struct Cand {
    int ph;          // 0 non-ignored, 1 ignored, 2 none
    double v;
    long long g;
};
__device__ __forceinline__ bool cand_better(int ph, double v, long long g, const Cand& c) {
    return ph < c.ph || (ph == c.ph && (v > c.v || (v == c.v && g > c.g)));
}

__global__ __launch_bounds__(256) void segm_match_kernel(const long long* mgrp, int J, const double* iou, const uint8_t* crowd,
                                                         const uint8_t* ign0, const double* gt_area, const double* dt_area,
                                                         const int32_t* dt_rank, const double* area_rng, int NA, const double* thr,
                                                         int K, unsigned long long* scratch, int32_t* rec_m, long long* rec_key,
                                                         int32_t* rec_cls, int32_t* npig) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= J) return;                                       // whole waves leave together
    const long long* t8 = mgrp + j * 8;
    const long long g0 = t8[0], G = t8[1], d0 = t8[2], D = t8[3], off = t8[4], cls = t8[5], seq = t8[6];
    if (G < 0 || D < 0 || D > SE_MAX_DETS || cls < 0 || cls >= K || g0 < 0 || d0 < 0) return;   // the host checks; never expected
    double lo_[SE_MAX_A], hi_[SE_MAX_A], th[SE_T];
#pragma unroll
    for (int a = 0; a < SE_MAX_A; ++a) {
        lo_[a] = a < NA ? area_rng[2 * a] : 0.0;
        hi_[a] = a < NA ? area_rng[2 * a + 1] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < SE_T; ++t) th[t] = fmin(thr[t], 1.0 - 1e-10);
    // this lane's first GT in registers; the GTs beyond the first 64 keep their matched bits in scratch
    const bool has0 = lane < G;
    const double ga0 = has0 ? gt_area[g0 + lane] : 0.0;
    const bool ig0 = has0 && ign0[g0 + lane] != 0, cr0 = has0 && crowd[g0 + lane] != 0;
    unsigned long long m0 = 0ull;
    for (long long g = 64 + lane; g < G; g += 64) scratch[g0 + g] = 0ull;
    // the non-ignored GTs of every area range
#pragma unroll
    for (int a = 0; a < SE_MAX_A; ++a) {
        if (a >= NA) break;
        int cnt = 0;
        for (long long g = lane; g < G; g += 64) {
            const double ga = gt_area[g0 + g];
            cnt += !(ign0[g0 + g] != 0 || ga < lo_[a] || ga > hi_[a]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0 && cnt) atomicAdd(&npig[cls * NA + a], cnt);
    }
    for (int d = 0; d < (int)D; ++d) {
        const double* row = iou + off + (long long)d * G;
        const double da = dt_area[d0 + d];
        const double v0 = has0 ? row[lane] : -1.0;
        int res[SE_MAX_A] = {0, 0, 0, 0};
#pragma unroll
        for (int a = 0; a < SE_MAX_A; ++a) {
            if (a >= NA) break;
            const bool d_out = da < lo_[a] || da > hi_[a];
            const bool iga0 = ig0 || ga0 < lo_[a] || ga0 > hi_[a];
            int tpm = 0, igm = 0;
            for (int t = 0; t < SE_T; ++t) {
                const int bit = a * SE_T + t;
                Cand c{2, 0.0, -1};
                if (has0 && v0 >= th[t] && !(((m0 >> bit) & 1ull) && !cr0)) c = Cand{iga0 ? 1 : 0, v0, lane};
                for (long long g = 64 + lane; g < G; g += 64) {
                    const double v = row[g];
                    if (!(v >= th[t])) continue;
                    const bool cr = crowd[g0 + g] != 0;
                    if (((scratch[g0 + g] >> bit) & 1ull) && !cr) continue;
                    const double ga = gt_area[g0 + g];
                    const int ph = (ign0[g0 + g] != 0 || ga < lo_[a] || ga > hi_[a]) ? 1 : 0;
                    if (cand_better(ph, v, g, c)) c = Cand{ph, v, g};
                }
                const unsigned long long holders = __ballot(c.ph < 2);
                if (holders == 0) {                           // unmatched: ignored iff its own area lies outside the range
                    igm |= (int)d_out << t;
                    continue;
                }
                if (holders & (holders - 1)) {                // several lanes hold a candidate: the best of them, in every lane
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const int oph = __shfl_xor(c.ph, o, 64);
                        const double ov = __shfl_xor(c.v, o, 64);
                        const long long og = __shfl_xor(c.g, o, 64);
                        if (cand_better(oph, ov, og, c)) c = Cand{oph, ov, og};
                    }
                } else {                                      // one lane (the common case): its candidate, one read instead of six steps
                    const int src = __ffsll((long long)holders) - 1;
                    c = Cand{__shfl(c.ph, src, 64), __shfl(c.v, src, 64), __shfl(c.g, src, 64)};
                }
                tpm |= 1 << t;
                igm |= (c.ph == 1) << t;
                if ((int)(c.g & 63) == lane) {
                    if (c.g < 64) m0 |= 1ull << bit; else scratch[g0 + c.g] |= 1ull << bit;
                }
            }
            res[a] = tpm | (igm << 16);
        }
        if (lane == 0) {
            const long long n = d0 + d;
#pragma unroll
            for (int a = 0; a < SE_MAX_A; ++a)
                if (a < NA) rec_m[n * NA + a] = res[a];
            rec_key[n] = (long long)(((unsigned long long)(uint32_t)dt_rank[n] << 32) | ((unsigned long long)seq << 7) |
                                     (unsigned long long)d);
            rec_cls[n] = (int32_t)cls;
        }
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_segm_mask_stats(const uint32_t* bits, const int64_t* tab, int N, int32_t* bbox, int32_t* area, void* stream) {
    EP24_REQUIRE(N >= 0, EP24_E_UNSUPPORTED, "segm_mask_stats: N=%d", N);
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(bits && tab && bbox && area, EP24_E_ARG, "segm_mask_stats: null pointer");
    hipLaunchKernelGGL(segm_mask_stats_kernel, dim3((unsigned)(N < 65535 ? N : 65535)), dim3(256), 0, S_, bits, (const long long*)tab,
                       (long)N, bbox, area);
    EP24_LAUNCH_CHECK("ep24_segm_mask_stats");
    return EP24_OK;
}

extern "C" int ep24_segm_iou(const uint32_t* bits, const int64_t* tab, int N, const int32_t* bbox, const int32_t* area,
                             const uint8_t* gt_crowd, const int64_t* grp, int J, int64_t pairs, double* iou, int64_t* inter,
                             void* stream) {
    EP24_REQUIRE(J >= 0 && pairs >= 0 && N >= 0, EP24_E_UNSUPPORTED, "segm_iou: N=%d J=%d pairs=%lld", N, J, (long long)pairs);
    if (J == 0 || pairs == 0) return EP24_OK;
    EP24_REQUIRE(bits && tab && bbox && area && gt_crowd && grp && iou, EP24_E_ARG, "segm_iou: null pointer");
    const long long per = 4LL << 22;                          // pairs per launch: 2^22 workgroups of four waves
    for (long long p0 = 0; p0 < pairs; p0 += per) {
        const long long np = pairs - p0 < per ? pairs - p0 : per;
        hipLaunchKernelGGL(segm_iou_kernel, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, S_, bits, (const long long*)tab, (long long)N, bbox,
                           area, gt_crowd, (const long long*)grp, J, p0, (long long)pairs, iou, (long long*)inter);
    }
    EP24_LAUNCH_CHECK("ep24_segm_iou");
    return EP24_OK;
}

extern "C" int ep24_segm_match(const int64_t* mgrp, int J, const double* iou, const uint8_t* gt_crowd, const uint8_t* gt_ignore0,
                               const double* gt_area, const double* dt_area, const int32_t* dt_rank, const double* area_rng, int NA,
                               const double* iou_thr, int num_classes, int64_t* scratch, int32_t* rec_m, int64_t* rec_key,
                               int32_t* rec_cls, int32_t* npig, void* stream) {
    EP24_REQUIRE(J >= 0, EP24_E_UNSUPPORTED, "segm_match: J=%d", J);
    EP24_REQUIRE(NA >= 1 && NA <= SE_MAX_A, EP24_E_UNSUPPORTED, "segm_match: %d area ranges (1..%d)", NA, SE_MAX_A);
    EP24_REQUIRE(num_classes > 0, EP24_E_UNSUPPORTED, "segm_match: num_classes=%d", num_classes);
    if (J == 0) return EP24_OK;
    EP24_REQUIRE(mgrp && area_rng && iou_thr && npig, EP24_E_ARG, "segm_match: null pointer");
    // iou, the GT and detection arrays, scratch and the records may be null only when no group has a GT / a detection: the
    // kernel then never forms an address from them
    hipLaunchKernelGGL(segm_match_kernel, dim3((unsigned)((J + 3) / 4)), dim3(256), 0, S_, (const long long*)mgrp, J, iou, gt_crowd,
                       gt_ignore0, gt_area, dt_area, dt_rank, area_rng, NA, iou_thr, num_classes, (unsigned long long*)scratch, rec_m,
                       (long long*)rec_key, rec_cls, npig);
    EP24_LAUNCH_CHECK("ep24_segm_match");
    return EP24_OK;
}

extern "C" int ep24_segm_accumulate(const int32_t* order, const int64_t* rec_key, const int32_t* rec_cls, const int32_t* rec_m,
                                    int64_t n, const int32_t* npig, int num_classes, int NA, const int32_t* max_dets, int NM,
                                    const double* rec_thr, int64_t* cls_range, int32_t* ctp_scratch, double* env_scratch,
                                    double* precision, double* recall, void* stream) {
    EP24_REQUIRE(npig && max_dets && rec_thr && precision && recall, EP24_E_ARG, "segm_accumulate: null pointer");
    EP24_REQUIRE(n == 0 || (order && rec_key && rec_cls && rec_m && ctp_scratch && env_scratch), EP24_E_ARG,
                 "segm_accumulate: null record buffer");
    EP24_REQUIRE(num_classes > 0 && num_classes <= 65535 && n >= 0 && n <= 0x7FFFFFFFLL, EP24_E_UNSUPPORTED,
                 "segm_accumulate: num_classes=%d n=%lld", num_classes, (long long)n);
    EP24_REQUIRE(NA >= 1 && NA <= SE_MAX_A && NM >= 1 && NM <= SE_MAX_M, EP24_E_UNSUPPORTED,
                 "segm_accumulate: %d area ranges, %d maxDets (1..%d, 1..%d)", NA, NM, SE_MAX_A, SE_MAX_M);
    launch_accumulate(order, rec_key, rec_cls, rec_m, n, npig, num_classes, NA, max_dets, NM, rec_thr, ctp_scratch, env_scratch, precision,
                      recall, S_);
    EP24_LAUNCH_CHECK("ep24_segm_accumulate");
    return EP24_OK;
}
