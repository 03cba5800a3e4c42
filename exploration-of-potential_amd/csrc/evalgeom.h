// ep24 - what the two 24-point matchers share (evaluate.hip: one area range; evalstrata.hip: strata of object size and
// distortion zone): the geometry of a GT row and of a detection row for the three IoU types, the pair IoUs, where a detection
// row lives, and the per-image sort of the detections by (class, score desc, p asc).
#pragma once
#include "geom.h"
#include "poly24.h"

namespace {

constexpr int EV_T = 10;             // IoU thresholds
constexpr int EV_MAX_L = 256;        // GT rows per image
constexpr int EV_MAX_DETS = 128;     // detections per (image, class): the rank takes 7 bits of the record key
constexpr int EV_NONE = 0xFFFF;      // class field of a detection whose class is outside [0, C): sorted last, never recorded

// ascending order of the result = descending order of the score (total order on the fp32 bit patterns)
__device__ __forceinline__ uint32_t ord_desc(float s) {
    uint32_t u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

// GT geometry from a label row's 50 coordinates (centre, 24 vertices): circle24 = (cx, cy, r[24]) with the expressions of
// pairwise_kernel (loss.hip); rect = (x0, y0, x1, y1) = min / max over the vertices; poly24 (GW = 48) = the 24 vertices
template <int GW>
__device__ __forceinline__ void gt_geometry(const float* t50, int iou_type, float* out) {
    if constexpr (GW == 48) {
        for (int k = 0; k < 48; ++k) out[k] = t50[2 + k];
    } else if (iou_type == 0) {
        out[0] = t50[0];
        out[1] = t50[1];
        for (int k = 0; k < 24; ++k) {
            const float vx = t50[2 + 2 * k] - t50[0], vy = t50[3 + 2 * k] - t50[1];
            out[2 + k] = sqrtf(vx * vx + vy * vy);
        }
    } else {
        float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        for (int k = 0; k < 24; ++k) {
            const float px = t50[2 + 2 * k], py = t50[3 + 2 * k];
            x0 = fminf(x0, px); x1 = fmaxf(x1, px); y0 = fminf(y0, py); y1 = fmaxf(y1, py);
        }
        out[0] = x0; out[1] = y0; out[2] = x1; out[3] = y1;
    }
}

// Detection geometry from (cx, cy, r[24]): circle24 keeps it, rect = min / max over c + r_k * (cos, sin)(15 deg * k) with the
// cos / sin table cs[48] the host computes in float64 and rounds.  NOT post_prepare's NMS rectangle, which keeps the reference's
// theta * cos(theta) factors (boxes.py:31-33).  poly24 (GW = 48) keeps the 24 points themselves, product and sum in fp32 as for rect.
template <int GW>
__device__ __forceinline__ void det_geometry(const float* q26, int iou_type, const float* cs, float* out) {
    if constexpr (GW == 48) {
        poly24_det_vertices(q26, cs, out);
    } else if (iou_type == 0) {
        for (int k = 0; k < 26; ++k) out[k] = q26[k];
    } else {
        float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        for (int k = 0; k < 24; ++k) {
            const float px = q26[0] + q26[2 + k] * cs[k];
            const float py = q26[1] + q26[2 + k] * cs[24 + k];
            x0 = fminf(x0, px); x1 = fmaxf(x1, px); y0 = fminf(y0, py); y1 = fmaxf(y1, py);
        }
        out[0] = x0; out[1] = y0; out[2] = x1; out[3] = y1;
    }
}

// circle24: mean over the rays of inter / union of the two concentric-ray circles (ray_giou's iou term, geom.h), all fp32
__device__ __forceinline__ float circle24_iou(const float* g, const float* q) {
    const float ddx = g[0] - q[0], ddy = g[1] - q[1];
    const float d = sqrtf(ddx * ddx + ddy * ddy);
    float acc = 0.f;
    for (int k = 0; k < 24; ++k) {
        const float r1 = g[2 + k], r2 = q[2 + k];
        const float inter = ray_inter(r1, r2, d);
        const float area1 = EP24_PI_F * (r1 * r1), area2 = EP24_PI_F * (r2 * r2);
        acc += inter / (area1 + area2 - inter + 1e-6f);
    }
    return acc / 24.0f;
}

// rect: pycocotools-style box IoU in float64 (no +1)
__device__ __forceinline__ double rect_iou(const float* g, const float* q) {
    const double gx0 = g[0], gy0 = g[1], gx1 = g[2], gy1 = g[3];
    const double dx0 = q[0], dy0 = q[1], dx1 = q[2], dy1 = q[3];
    const double w = fmax(0.0, fmin(gx1, dx1) - fmax(gx0, dx0));
    const double h = fmax(0.0, fmin(gy1, dy1) - fmax(gy0, dy0));
    const double inter = w * h;
    const double ag = (gx1 - gx0) * (gy1 - gy0), ad = (dx1 - dx0) * (dy1 - dy0);
    return inter / (ag + ad - inter);
}

template <int GW>
__device__ __forceinline__ double pair_iou(const float* g, const float* q, int iou_type) {
    if constexpr (GW == 48) return poly24_iou(g, q);
    else return iou_type == 0 ? (double)circle24_iou(g, q) : rect_iou(g, q);
}

// Where detection r of image b lives: row = rows + (row_off[b] + a) * ncols with a = keep[b * keep_stride + r] (the NMS output of
// post_nms) or a = r (keep == null: a concatenation of postprocess rows).  class_conf / class come from conf / cls[row_off[b] + a]
// (post_prepare's arrays) or from the row's columns 27 / 28 (conf == null).  score = obj * class_conf in fp32, as post_prepare.
struct DetSrc {
    const float* rows;
    int ncols;
    const int64_t* row_off;
    const int32_t* keep;
    int64_t keep_stride;
    const float* conf;
    const int32_t* cls;
};

__device__ __forceinline__ const float* det_row(const DetSrc& s, int b, int r, float& score, int& c, int C) {
    const int64_t a = s.row_off[b] + (s.keep ? (int64_t)s.keep[(int64_t)b * s.keep_stride + r] : (int64_t)r);
    const float* row = s.rows + a * s.ncols;
    float cf;
    if (s.conf) {
        cf = s.conf[a];
        c = s.cls[a];
    } else {
        cf = row[27];
        const float fc = row[28];
        c = (fc >= 0.f && fc < (float)C) ? (int)fc : EV_NONE;
    }
    if (c < 0 || c >= C) c = EV_NONE;
    const float sc = row[26] * cf;
    score = sc == 0.f ? 0.f : sc;                          // -0 ranks with +0 (a tie, as in a comparison sort)
    return row;
}

// The nd detections of image b in (class, score desc, p asc) order: bitonic sort of 64-bit keys class << 48 | ordered score
// << 16 | p in global scratch key[P2], P2 the power of two >= nd; a workgroup of 256, every thread of it.  Ends on a barrier.
__device__ __forceinline__ void sort_image_dets(const DetSrc& src, int b, int nd, int C, uint64_t* key, int tid) {
    int P2 = 1;
    while (P2 < nd) P2 <<= 1;
    for (int i = tid; i < P2; i += 256) {
        uint64_t k = ~0ull;
        if (i < nd) {
            float s;
            int c;
            det_row(src, b, i, s, c, C);
            k = ((uint64_t)c << 48) | ((uint64_t)ord_desc(s) << 16) | (uint64_t)i;
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t ki = key[i], kl = key[l];
                    const bool up = (i & k) == 0;
                    if ((ki > kl) == up) { key[i] = kl; key[l] = ki; }
                }
            }
            __syncthreads();
        }
}

}  // namespace
