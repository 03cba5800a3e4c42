// ep24 - the 24-point matcher and what it is made of.  evaluate.hip runs its plain instance (one area range), evalstrata.hip the
// instance with strata of object size and distortion zone.  Here: the geometry of a GT row and of a detection row for the three IoU
// types, the pair IoUs, where a detection row lives, the per-image sort of the detections by (class, score desc, p asc), the measures
// of a stratum, the match kernel, and the host-side check and launch that both entry points go through.
#pragma once
#include "geom.h"
#include "lensmath.h"
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

// ---------------------------------------------------------------------------------------------- the measures of a stratum
constexpr int ES_MAX_NA = 8;         // strata per evaluation: one bit each in a GT's ignore mask
constexpr int ES_ZT_D = 16;          // doubles per image of the zone table

struct Strata {
    double v[ES_MAX_NA][4];
};

// 0.5 * |sum_k x_k y_{k+1} - x_{k+1} y_k| over 24 (x, y) pairs of fp32, promoted here; the sum starts from 0.0 and runs in k
__device__ __forceinline__ double shoelace24(const float* p) {
    double s = 0.0;
    for (int k = 0; k < 24; ++k) {
        const int k1 = k == 23 ? 0 : k + 1;
        const double x0 = p[2 * k], y0 = p[2 * k + 1], x1 = p[2 * k1], y1 = p[2 * k1 + 1];
        s += x0 * y1 - x1 * y0;
    }
    return 0.5 * fabs(s);
}

// zone value of a centre (X, Y) by the image's table row z = {kind, fx, fy, cx, cy, k1..k4, theta_max, thetad(theta_max), 0...}:
// kind 1 the normalised radius, kind 2 the incidence angle in degrees (+infinity beyond the field), anything else 0
__device__ __forceinline__ double zone_of(double X, double Y, const double* z) {
    const int kind = (int)z[0];
    const double x = (X - z[3]) / z[1], y = (Y - z[4]) / z[2];
    const double rd = sqrt(x * x + y * y);                    // not hypot: a plain IEEE sqrt that the host restates bit for bit
    if (kind == 1) return rd;
    if (kind == 2) {
        if (rd > z[10]) return INFINITY;
        const double th = lens_newton(fmin(rd, z[10]), z[5], z[6], z[7], z[8], z[9]);
        return th * (180.0 / 3.141592653589793);
    }
    return 0.0;
}

// bit a: the object lies outside stratum a
__device__ __forceinline__ unsigned outside_mask(double area, double zone, const Strata& st, int NA) {
    unsigned m = 0;
#pragma unroll
    for (int a = 0; a < ES_MAX_NA; ++a)
        if (a < NA && (area < st.v[a][0] || area > st.v[a][1] || zone < st.v[a][2] || zone >= st.v[a][3])) m |= 1u << a;
    return m;
}

// ---------------------------------------------------------------------------------------------- the match kernel
// What only the instance with strata takes.  The plain instance is the evaluation of one stratum that nothing lies outside of:
// NA = 1 at compile time, no measures, no ignore bits.
template <bool STRATA>
struct StrataArgs {
    static constexpr int NA = 1;
};
template <>
struct StrataArgs<true> {
    const double* scales;            // [B] input pixels per original pixel
    const double* zt;                // [B][ES_ZT_D]
    Strata st;
    int NA;
    double* rec_val;                 // [n][2] (area, zone) of the recorded detections, or null
};

// The wave's GT for one detection at one threshold.  ok(q): this lane's row q * 64 + lane may be picked.  pycocotools: the largest
// IoU >= thr among those, equal IoUs -> the later GT row.  False if no lane has a candidate, else the row in every lane's bg.
// SURE: the caller has seen a candidate already (the strata instance's own ballots), so the ballot that finds out is left away - with
// it the empty-handed exit of the threshold loop took a detour through a second block and NA = 8 measured 5.6 % slower.
template <bool SURE, typename Ok>
__device__ __forceinline__ bool pick_gt(const double (&iou)[4], double thr, int lane, int& bg, Ok ok) {
    double best = thr;
    bg = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (ok(q) && iou[q] >= best) { best = iou[q]; bg = q * 64 + lane; }
    if (!SURE && __ballot(bg >= 0) == 0) return false;
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int og = __shfl_xor(bg, o, 64);
        if (og >= 0 && (bg < 0 || ob > best || (ob == best && og > bg))) { best = ob; bg = og; }
    }
    return true;
}

// One workgroup per image: GT count / geometry into LDS, the image's detections sorted in global scratch, then one wave per class
// segment greedily matches the first max_dets detections against the class's GTs, four GT rows per lane, for all 10 IoU thresholds
// and appends one record per detection: rec_m[o][NA] = 10 TP bits | 10 ignore bits << 16 per stratum (plain: rec_m[o] = the TP bits).
// With strata a GT carries an 8-bit ignore mask; a detection's IoUs are computed once and serve every stratum, only the picks repeat.
// matched[4][NA / 2] lives in registers (16 bits per stratum: every index is a constant after unrolling).
// GW = floats of geometry per object: 26 for circle24 / rect, 48 for poly24.  GS = the LDS row stride: 49 for poly24, so that the 64
// lanes' rows fall into different banks.
template <int GW, bool STRATA>
__global__ __launch_bounds__(256) void eval_match_kernel(const float* labels, int L, DetSrc src, const int32_t* count, int C,
                                                         int iou_type, const float* cs, const double* thr, int max_dets,
                                                         int64_t seq_base, uint64_t* skey, int P, StrataArgs<STRATA> sa,
                                                         int64_t* rec_key, int32_t* rec_cls, int32_t* rec_p, int32_t* rec_m,
                                                         int32_t* rec_count, int32_t* npig, int32_t* err) {
    constexpr int GS = GW == 48 ? 49 : GW;
    constexpr int MA = STRATA ? ES_MAX_NA : 1;
    __shared__ float g_geo[EV_MAX_L][GS];
    __shared__ int g_cls[EV_MAX_L];
    __shared__ double thr_sh[EV_T];
    __shared__ float cs_sh[48];
    __shared__ int n_sh;
    // these two are referenced under STRATA only: the plain instance has no LDS for them
    __shared__ uint8_t g_ign[EV_MAX_L];                   // bit a: the GT lies outside stratum a
    __shared__ double zt_sh[ES_ZT_D];                     // the image's zone-table row
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* lab = labels + (long)b * L * EP24_LABEL_COLS;
    // GT rows: the first n, n = rows whose 51 values sum to > 0 (losses.py:190, as count_gt in assign.hip)
    if (tid == 0) n_sh = 0;
    if (tid < EV_T) thr_sh[tid] = fmin(thr[tid], 1.0 - 1e-10);
    if (tid < 48) cs_sh[tid] = cs[tid];
    [[maybe_unused]] double sc2 = 1.0;
    if constexpr (STRATA) {
        if (tid < ES_ZT_D) zt_sh[tid] = sa.zt[(long)b * ES_ZT_D + tid];
        sc2 = sa.scales[b] * sa.scales[b];
    }
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
        gt_geometry<GW>(t + 1, iou_type, g_geo[i]);
        unsigned out = 0u;
        if constexpr (STRATA) {
            out = outside_mask(shoelace24(t + 3) / sc2, zone_of((double)t[1], (double)t[2], zt_sh), sa.st, sa.NA);
            g_ign[i] = (uint8_t)out;
        }
        if (c >= 0)
            for (int a = 0; a < sa.NA; ++a)
                if (!((out >> a) & 1u)) atomicAdd(&npig[c * sa.NA + a], 1);
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
            // this lane's GTs of class c: rows lane, lane + 64, lane + 128, lane + 192, and their ignore masks
            bool has[4];
            [[maybe_unused]] unsigned ig[4];
            bool any = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = q * 64 + lane;
                has[q] = gi < ng && g_cls[gi] == c;
                if constexpr (STRATA) ig[q] = has[q] ? g_ign[gi] : 0u;
                any |= has[q];
            }
            any = __ballot(any) != 0;
            int rbase = 0;
            if (lane == 0) rbase = atomicAdd(rec_count, m);
            rbase = __shfl(rbase, 0, 64);
            unsigned matched[4][(MA + 1) / 2];                // bit t + 16 * (a & 1) of [q][a >> 1]: GT q is taken at (a, t)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int h = 0; h < (MA + 1) / 2; ++h) matched[q][h] = 0u;
            for (int r = 0; r < m; ++r) {
                const uint64_t kr = key[s0 + r];
                const int p = (int)(kr & 0xFFFF);
                const uint32_t sbits = (uint32_t)(kr >> 16);
                const int64_t o = (int64_t)rbase + r;
                double iou[4] = {-1.0, -1.0, -1.0, -1.0};
                [[maybe_unused]] double darea = 0.0, dzone = 0.0;
                [[maybe_unused]] unsigned dout = 0u;
                if (STRATA || any) {                          // plain: a segment without GTs of its class reads no detection row
                    float dsc;
                    int cc;
                    const float* row = det_row(src, b, p, dsc, cc, C);
                    float qg[GW];
                    if constexpr (STRATA) {
                        // the detection's own area and zone: the same in every lane.  poly24's geometry is these vertices
                        float dvs[GW == 48 ? 1 : 48];
                        float* dv = GW == 48 ? qg : dvs;
                        poly24_det_vertices(row, cs_sh, dv);
                        darea = shoelace24(dv) / sc2;
                        dzone = zone_of((double)row[0], (double)row[1], zt_sh);
                        dout = outside_mask(darea, dzone, sa.st, sa.NA);
                    }
                    if (any) {
                        if constexpr (!(STRATA && GW == 48)) det_geometry<GW>(row, iou_type, cs_sh, qg);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (has[q]) iou[q] = pair_iou<GW>(g_geo[q * 64 + lane], qg, iou_type);
                    }
                }
#pragma unroll
                for (int a = 0; a < MA; ++a) {
                    if (a >= sa.NA) continue;
                    int tpm = 0, igm = (dout >> a) & 1u ? 0x3FF : 0;      // unmatched: ignored iff the detection lies outside the stratum
                    if (any) {
                        for (int t = 0; t < EV_T; ++t) {
                            const double th = thr_sh[t];
                            const unsigned mbit = 1u << (t + 16 * (a & 1));
                            const auto open = [&](int q) { return has[q] && !(matched[q][a >> 1] & mbit); };
                            int bg;
                            bool useign = false;
                            if constexpr (STRATA) {
                                // evaluateImg in closed form: among the GTs not taken at (a, t) with iou >= min(thr, 1 - 1e-10) the
                                // maximum of (not ignored, iou, row)
                                bool cand[4], ca = false, cn = false;
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    cand[q] = open(q) && iou[q] >= th;
                                    ca |= cand[q];
                                    cn |= cand[q] && !((ig[q] >> a) & 1u);
                                }
                                if (__ballot(ca) == 0) continue;
                                useign = __ballot(cn) == 0;             // no non-ignored candidate: the best ignored one
                                pick_gt<true>(iou, th, lane, bg, [&](int q) { return cand[q] && (useign || !((ig[q] >> a) & 1u)); });
                            } else if (!pick_gt<false>(iou, th, lane, bg, open)) {
                                continue;
                            }
                            tpm |= 1 << t;
                            igm = useign ? (igm | (1 << t)) : (igm & ~(1 << t));
                            if ((bg & 63) == lane) matched[bg >> 6][a >> 1] |= mbit;
                        }
                    }
                    if (lane == 0) rec_m[o * sa.NA + a] = tpm | (igm << 16);
                }
                if (lane == 0) {
                    rec_key[o] = (int64_t)(((uint64_t)sbits << 32) | ((uint64_t)seq << 7) | (uint64_t)r);
                    rec_cls[o] = c;
                    rec_p[o] = p;
                    if constexpr (STRATA)
                        if (sa.rec_val) {
                            sa.rec_val[2 * o] = darea;
                            sa.rec_val[2 * o + 1] = dzone;
                        }
                }
            }
        }
    }
}

// The limits of both entry points (`name` is the entry's, for the message), where the detections live, and the launch of the
// instance for the IoU type's geometry.
template <bool STRATA>
static int eval_match_launch(const char* name, const float* labels, int L, int B, const float* rows, int ncols, const int64_t* row_off,
                             const int32_t* keep, int64_t keep_stride, const int32_t* count, const float* conf, const int32_t* cls,
                             int num_classes, int iou_type, const float* ray_cs, const double* iou_thr, int max_dets, int64_t seq_base,
                             int64_t* sort_scratch, int P, const StrataArgs<STRATA>& sa, int64_t* rec_key, int32_t* rec_cls,
                             int32_t* rec_p, int32_t* rec_m, int32_t* rec_count, int32_t* npig, int32_t* err, hipStream_t stream) {
    if (B == 0) return EP24_OK;
    EP24_REQUIRE(labels && rows && row_off && count && ray_cs && iou_thr && sort_scratch && rec_key && rec_cls && rec_p && rec_m &&
                 rec_count && npig && err && B > 0 && P > 0, EP24_E_ARG, "%s: bad arguments", name);
    EP24_REQUIRE((conf == nullptr) == (cls == nullptr), EP24_E_ARG, "%s: conf=%s without cls=%s: they come together", name,
                 conf ? "set" : "null", cls ? "set" : "null");
    EP24_REQUIRE(ncols >= (conf ? 27 : 29), EP24_E_ARG, "%s: ncols=%d", name, ncols);
    EP24_REQUIRE(L >= 0 && L <= EV_MAX_L, EP24_E_UNSUPPORTED, "%s: L=%d GT rows per image (at most %d)", name, L, EV_MAX_L);
    EP24_REQUIRE(max_dets > 0 && max_dets <= EV_MAX_DETS, EP24_E_UNSUPPORTED, "%s: max_dets=%d (1..%d)", name, max_dets, EV_MAX_DETS);
    EP24_REQUIRE(num_classes > 0 && num_classes < EV_NONE, EP24_E_UNSUPPORTED, "%s: num_classes=%d (1..%d)", name, num_classes,
                 EV_NONE - 1);
    EP24_REQUIRE(P <= 65536 && (P & (P - 1)) == 0, EP24_E_UNSUPPORTED, "%s: P=%d (a power of two, at most 65536 detections per image)",
                 name, P);
    EP24_REQUIRE(seq_base >= 0 && seq_base + B <= (1LL << 25), EP24_E_UNSUPPORTED, "%s: image sequence seq_base=%lld + %d beyond 2^25",
                 name, (long long)seq_base, B);
    EP24_REQUIRE(iou_type >= 0 && iou_type <= 2, EP24_E_UNSUPPORTED, "%s: iou_type=%d (0 circle24, 1 rect, 2 poly24)", name, iou_type);
    const DetSrc src{rows, ncols, row_off, keep, keep_stride, conf, cls};
    auto* kernel = iou_type == 2 ? eval_match_kernel<48, STRATA> : eval_match_kernel<26, STRATA>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, stream, labels, L, src, count, num_classes, iou_type, ray_cs, iou_thr, max_dets,
                       seq_base, (uint64_t*)sort_scratch, P, sa, rec_key, rec_cls, rec_p, rec_m, rec_count, npig, err);
    EP24_LAUNCH_CHECK(name);
    return EP24_OK;
}

}  // namespace
