// ep24 - evaluation of 24-point detections by strata of object size and distortion zone (include/ep24.h section E8; DESIGN.md
// section 7; ep24.evaluate.Evaluator24(strata=...)).  A stratum is {area_lo, area_hi, z_lo, z_hi}: an object lies outside it iff
// area < area_lo || area > area_hi || z < z_lo || z >= z_hi, and pycocotools' evaluateImg treats what lies outside as ignored.
//
//   eval_measure       area and zone of label rows or detection rows, one thread per row: for tests, tools and the host API
//   eval_match_strata  eval_match_kernel (evaluate.hip) with strata: one workgroup per image, GT geometry in LDS plus an 8-bit
//                      ignore mask per GT, one wave per class segment, four GT rows per lane.  A detection's IoUs are computed once
//                      and serve every stratum; only the wave reductions repeat, and a reduction whose ballot of candidates is empty
//                      is skipped.  matched[4][NA] lives in registers (16 bits per stratum: every index is a constant after unrolling)
//   eval_accumulate_strata  the accumulate kernel of accumulate.h over [C][NA][NM]
//
// All measures are double, every operation rounded on its own.  The only atomics are integer ones (npig, the append offset):
// every result is a bit-exact function of the inputs.
#include "accumulate.h"
#include "evalgeom.h"
#include "lensmath.h"

namespace {

constexpr int ES_MAX_NA = 8;         // strata per evaluation: one bit each in a GT's ignore mask
constexpr int ES_MAX_NM = 4;         // maxDets values per accumulate
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

// kind 0: label rows (class, centre, 24 vertices), kind 1: detection rows (centre, 24 radii, ...)
__global__ __launch_bounds__(256) void eval_measure_kernel(const float* rows, int ncols, int kind, const int32_t* image, int n, int B,
                                                           const double* scales, const double* zt, const float* cs, double* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* r = rows + (long)i * ncols;
    const int b = image[i];
    if (b < 0 || b >= B) {                                    // no table row to read: not a number, nothing read
        out[2 * (long)i] = out[2 * (long)i + 1] = __builtin_nan("");
        return;
    }
    float v[48];
    double X, Y;
    if (kind == 0) {
        for (int k = 0; k < 48; ++k) v[k] = r[3 + k];
        X = r[1]; Y = r[2];
    } else {
        poly24_det_vertices(r, cs, v);
        X = r[0]; Y = r[1];
    }
    const double s = scales[b];
    out[2 * (long)i] = shoelace24(v) / (s * s);
    out[2 * (long)i + 1] = zone_of(X, Y, zt + (long)b * ES_ZT_D);
}

template <int GW>
__global__ __launch_bounds__(256) void eval_match_strata_kernel(const float* labels, int L, DetSrc src, const int32_t* count, int C,
                                                                int iou_type, const float* cs, const double* thr, int max_dets,
                                                                int64_t seq_base, uint64_t* skey, int P, const double* scales,
                                                                const double* zt, Strata st, int NA, int64_t* rec_key,
                                                                int32_t* rec_cls, int32_t* rec_p, int32_t* rec_m, double* rec_val,
                                                                int32_t* rec_count, int32_t* npig, int32_t* err) {
    constexpr int GS = GW == 48 ? 49 : GW;
    __shared__ float g_geo[EV_MAX_L][GS];
    __shared__ int g_cls[EV_MAX_L];
    __shared__ uint8_t g_ign[EV_MAX_L];                       // bit a: the GT lies outside stratum a
    __shared__ double thr_sh[EV_T];
    __shared__ double zt_sh[ES_ZT_D];
    __shared__ float cs_sh[48];
    __shared__ int n_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* lab = labels + (long)b * L * EP24_LABEL_COLS;
    if (tid == 0) n_sh = 0;
    if (tid < EV_T) thr_sh[tid] = fmin(thr[tid], 1.0 - 1e-10);
    if (tid < 48) cs_sh[tid] = cs[tid];
    if (tid < ES_ZT_D) zt_sh[tid] = zt[(long)b * ES_ZT_D + tid];
    __syncthreads();
    for (int r = tid; r < L; r += 256) {
        float s = 0.f;
        for (int c = 0; c < EP24_LABEL_COLS; ++c) s += lab[r * EP24_LABEL_COLS + c];
        if (s > 0.f) atomicAdd(&n_sh, 1);
    }
    __syncthreads();
    const int ng = n_sh;
    const double sc = scales[b], sc2 = sc * sc;
    for (int i = tid; i < ng; i += 256) {
        const float* t = lab + (long)i * EP24_LABEL_COLS;
        const int c = (t[0] >= 0.f && t[0] < (float)C) ? (int)t[0] : -1;
        g_cls[i] = c;
        gt_geometry<GW>(t + 1, iou_type, g_geo[i]);
        const unsigned out = outside_mask(shoelace24(t + 3) / sc2, zone_of((double)t[1], (double)t[2], zt_sh), st, NA);
        g_ign[i] = (uint8_t)out;
        if (c >= 0)
            for (int a = 0; a < NA; ++a)
                if (!((out >> a) & 1u)) atomicAdd(&npig[c * NA + a], 1);
    }
    const int nd = count[b];
    if (nd > P || nd < 0) {                                   // host sizes P from the plan; never expected
        if (tid == 0) atomicOr(err, 1);
        return;
    }
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
            int m = 0;
            for (int q = 0; q < max_dets; q += 64) {
                const int jj = s0 + q + lane;
                const bool in = q + lane < max_dets && jj < nd && (int)(key[jj] >> 48) == c;
                m += __popcll(__ballot(in));
            }
            // this lane's GTs of class c: rows lane, lane + 64, lane + 128, lane + 192, and their ignore masks
            bool has[4];
            unsigned ig[4];
            bool any = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = q * 64 + lane;
                has[q] = gi < ng && g_cls[gi] == c;
                ig[q] = has[q] ? g_ign[gi] : 0u;
                any |= has[q];
            }
            any = __ballot(any) != 0;
            int rbase = 0;
            if (lane == 0) rbase = atomicAdd(rec_count, m);
            rbase = __shfl(rbase, 0, 64);
            unsigned matched[4][ES_MAX_NA / 2];               // bit t + 16 * (a & 1) of [q][a >> 1]: GT q is taken at (a, t)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int h = 0; h < ES_MAX_NA / 2; ++h) matched[q][h] = 0u;
            for (int r = 0; r < m; ++r) {
                const uint64_t kr = key[s0 + r];
                const int p = (int)(kr & 0xFFFF);
                const uint32_t sbits = (uint32_t)(kr >> 16);
                const int64_t o = (int64_t)rbase + r;
                float dsc;
                int cc;
                const float* row = det_row(src, b, p, dsc, cc, C);
                // the detection's own area and zone: the same in every lane
                float dv[48];
                poly24_det_vertices(row, cs_sh, dv);
                const double darea = shoelace24(dv) / sc2, dzone = zone_of((double)row[0], (double)row[1], zt_sh);
                const unsigned dout = outside_mask(darea, dzone, st, NA);
                double iou[4] = {-1.0, -1.0, -1.0, -1.0};
                if (any) {
                    float qs[GW == 48 ? 1 : GW];
                    const float* qg = dv;
                    if constexpr (GW != 48) {
                        det_geometry<GW>(row, iou_type, cs_sh, qs);
                        qg = qs;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (has[q]) iou[q] = pair_iou<GW>(g_geo[q * 64 + lane], qg, iou_type);
                }
#pragma unroll
                for (int a = 0; a < ES_MAX_NA; ++a) {
                    if (a >= NA) continue;
                    const bool dign = (dout >> a) & 1u;
                    int tpm = 0, igm = dign ? 0x3FF : 0;      // unmatched: ignored iff the detection lies outside the stratum
                    if (any) {
                        for (int t = 0; t < EV_T; ++t) {
                            // evaluateImg in closed form: among the GTs not taken at (a, t) with iou >= min(thr, 1 - 1e-10) the
                            // maximum of (not ignored, iou, row)
                            const double th = thr_sh[t];
                            const unsigned mbit = 1u << (t + 16 * (a & 1));
                            bool cand[4], ca = false, cn = false;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                cand[q] = has[q] && !(matched[q][a >> 1] & mbit) && iou[q] >= th;
                                ca |= cand[q];
                                cn |= cand[q] && !((ig[q] >> a) & 1u);
                            }
                            if (__ballot(ca) == 0) continue;
                            const bool useign = __ballot(cn) == 0;      // no non-ignored candidate: the best ignored one
                            double best = th;
                            int bg = -1;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (cand[q] && (useign || !((ig[q] >> a) & 1u)) && iou[q] >= best) { best = iou[q]; bg = q * 64 + lane; }
                            for (int x = 32; x > 0; x >>= 1) {
                                const double ob = __shfl_xor(best, x, 64);
                                const int og = __shfl_xor(bg, x, 64);
                                if (og >= 0 && (bg < 0 || ob > best || (ob == best && og > bg))) { best = ob; bg = og; }
                            }
                            tpm |= 1 << t;
                            igm = useign ? (igm | (1 << t)) : (igm & ~(1 << t));
                            if ((bg & 63) == lane) matched[bg >> 6][a >> 1] |= mbit;
                        }
                    }
                    if (lane == 0) rec_m[o * NA + a] = tpm | (igm << 16);
                }
                if (lane == 0) {
                    rec_key[o] = (int64_t)(((uint64_t)sbits << 32) | ((uint64_t)seq << 7) | (uint64_t)r);
                    rec_cls[o] = c;
                    rec_p[o] = p;
                    if (rec_val) {
                        rec_val[2 * o] = darea;
                        rec_val[2 * o + 1] = dzone;
                    }
                }
            }
        }
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_eval_measure(const float* rows, int ncols, int row_kind, const int32_t* image, int n, const double* scales,
                                 const double* zt, int B, const float* ray_cs, double* out, void* stream) {
    EP24_REQUIRE(n >= 0, EP24_E_ARG, "eval_measure: n=%d", n);
    EP24_REQUIRE(row_kind == 0 || row_kind == 1, EP24_E_ARG, "eval_measure: row_kind %d (0 label rows, 1 detection rows)", row_kind);
    EP24_REQUIRE(ncols >= (row_kind == 0 ? EP24_LABEL_COLS : 26), EP24_E_ARG, "eval_measure: ncols=%d", ncols);
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(rows && image && scales && zt && ray_cs && out && B > 0, EP24_E_ARG, "eval_measure: bad arguments");
    hipLaunchKernelGGL(eval_measure_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S_, rows, ncols, row_kind, image, n, B,
                       scales, zt, ray_cs, out);
    EP24_LAUNCH_CHECK("ep24_eval_measure");
    return EP24_OK;
}

extern "C" int ep24_eval_match_strata(const float* labels, int L, int B, const float* rows, int ncols, const int64_t* row_off,
                                      const int32_t* keep, int64_t keep_stride, const int32_t* count, const float* conf,
                                      const int32_t* cls, int num_classes, int iou_type, const float* ray_cs, const double* iou_thr,
                                      int max_dets, int64_t seq_base, int64_t* sort_scratch, int P, const double* scales,
                                      const double* zt, const double* strata, int NA, int64_t* rec_key, int32_t* rec_cls,
                                      int32_t* rec_p, int32_t* rec_m, double* rec_val, int32_t* rec_count, int32_t* npig,
                                      int32_t* err, void* stream) {
    EP24_REQUIRE(NA >= 1 && NA <= ES_MAX_NA, EP24_E_UNSUPPORTED, "eval_match_strata: NA=%d strata (1..%d)", NA, ES_MAX_NA);
    EP24_REQUIRE(strata, EP24_E_ARG, "eval_match_strata: strata is null");
    Strata st;
    for (int a = 0; a < ES_MAX_NA; ++a)
        for (int k = 0; k < 4; ++k) st.v[a][k] = a < NA ? strata[a * 4 + k] : 0.0;
    for (int a = 0; a < NA; ++a)
        EP24_REQUIRE(st.v[a][0] <= st.v[a][1] && st.v[a][2] <= st.v[a][3], EP24_E_ARG,
                     "eval_match_strata: strata[%d] = {%g, %g, %g, %g}: a range needs lo <= hi", a, st.v[a][0], st.v[a][1], st.v[a][2],
                     st.v[a][3]);
    if (B == 0) return EP24_OK;
    EP24_REQUIRE(labels && rows && row_off && count && ray_cs && iou_thr && sort_scratch && scales && zt && rec_key && rec_cls && rec_p &&
                 rec_m && rec_count && npig && err && B > 0 && P > 0, EP24_E_ARG, "eval_match_strata: bad arguments");
    EP24_REQUIRE((conf == nullptr) == (cls == nullptr), EP24_E_ARG, "eval_match_strata: conf and cls come together");
    EP24_REQUIRE(ncols >= (conf ? 27 : 29), EP24_E_ARG, "eval_match_strata: ncols=%d", ncols);
    EP24_REQUIRE(L >= 0 && L <= EV_MAX_L, EP24_E_UNSUPPORTED, "eval_match_strata: L=%d GT rows per image (at most %d)", L, EV_MAX_L);
    EP24_REQUIRE(max_dets > 0 && max_dets <= EV_MAX_DETS, EP24_E_UNSUPPORTED, "eval_match_strata: max_dets=%d (1..%d)", max_dets,
                 EV_MAX_DETS);
    EP24_REQUIRE(num_classes > 0 && num_classes < EV_NONE, EP24_E_UNSUPPORTED, "eval_match_strata: num_classes=%d (1..%d)", num_classes,
                 EV_NONE - 1);
    EP24_REQUIRE(P <= 65536 && (P & (P - 1)) == 0, EP24_E_UNSUPPORTED,
                 "eval_match_strata: P=%d (a power of two, at most 65536 detections per image)", P);
    EP24_REQUIRE(seq_base >= 0 && seq_base + B <= (1LL << 25), EP24_E_UNSUPPORTED,
                 "eval_match_strata: image sequence seq_base %lld + %d beyond 2^25", (long long)seq_base, B);
    EP24_REQUIRE(iou_type >= 0 && iou_type <= 2, EP24_E_UNSUPPORTED, "eval_match_strata: iou_type %d (0 circle24, 1 rect, 2 poly24)",
                 iou_type);
    DetSrc src{rows, ncols, row_off, keep, keep_stride, conf, cls};
    if (iou_type == 2)
        hipLaunchKernelGGL(eval_match_strata_kernel<48>, dim3(B), dim3(256), 0, S_, labels, L, src, count, num_classes, iou_type, ray_cs,
                           iou_thr, max_dets, seq_base, (uint64_t*)sort_scratch, P, scales, zt, st, NA, rec_key, rec_cls, rec_p, rec_m,
                           rec_val, rec_count, npig, err);
    else
        hipLaunchKernelGGL(eval_match_strata_kernel<26>, dim3(B), dim3(256), 0, S_, labels, L, src, count, num_classes, iou_type, ray_cs,
                           iou_thr, max_dets, seq_base, (uint64_t*)sort_scratch, P, scales, zt, st, NA, rec_key, rec_cls, rec_p, rec_m,
                           rec_val, rec_count, npig, err);
    EP24_LAUNCH_CHECK("ep24_eval_match_strata");
    return EP24_OK;
}

extern "C" int ep24_eval_accumulate_strata(const int32_t* order, const int64_t* rec_key, const int32_t* rec_cls, const int32_t* rec_m,
                                           int64_t n, const int32_t* npig, int num_classes, int NA, const int32_t* max_dets, int NM,
                                           const double* rec_thr, int32_t* ctp_scratch, double* env_scratch, double* precision,
                                           double* recall, void* stream) {
    EP24_REQUIRE(NA >= 1 && NA <= ES_MAX_NA, EP24_E_UNSUPPORTED, "eval_accumulate_strata: NA=%d strata (1..%d)", NA, ES_MAX_NA);
    EP24_REQUIRE(NM >= 1 && NM <= ES_MAX_NM, EP24_E_UNSUPPORTED, "eval_accumulate_strata: NM=%d maxDets values (1..%d)", NM, ES_MAX_NM);
    EP24_REQUIRE(num_classes > 0 && num_classes < EV_NONE, EP24_E_UNSUPPORTED, "eval_accumulate_strata: num_classes=%d (1..%d)",
                 num_classes, EV_NONE - 1);
    EP24_REQUIRE(n >= 0 && npig && max_dets && rec_thr && precision && recall, EP24_E_ARG, "eval_accumulate_strata: bad arguments");
    EP24_REQUIRE(n == 0 || (order && rec_key && rec_cls && rec_m && ctp_scratch && env_scratch), EP24_E_ARG,
                 "eval_accumulate_strata: null record buffer");
    launch_accumulate(order, rec_key, rec_cls, rec_m, n, npig, num_classes, NA, max_dets, NM, rec_thr, ctp_scratch, env_scratch,
                      precision, recall, S_);
    EP24_LAUNCH_CHECK("ep24_eval_accumulate_strata");
    return EP24_OK;
}
