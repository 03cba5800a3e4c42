// ep24 - evaluation of 24-point detections by strata of object size and distortion zone (include/ep24.h section E8; DESIGN.md
// section 7; ep24.evaluate.Evaluator24(strata=...)).  A stratum is {area_lo, area_hi, z_lo, z_hi}: an object lies outside it iff
// area < area_lo || area > area_hi || z < z_lo || z >= z_hi, and pycocotools' evaluateImg treats what lies outside as ignored.
//
//   eval_measure       area and zone of label rows or detection rows, one thread per row: for tests, tools and the host API
//   eval_match_strata  the STRATA = true instance of eval_match_kernel (evalgeom.h, where the measures of a stratum live too): the
//                      strata rows are checked here, every other limit and the launch are eval_match_launch's
//   eval_accumulate_strata  the accumulate kernel of accumulate.h over [C][NA][NM]
//
// All measures are double, every operation rounded on its own.  The only atomics are integer ones (npig, the append offset):
// every result is a bit-exact function of the inputs.
#include "accumulate.h"
#include "evalgeom.h"

namespace {

constexpr int ES_MAX_NM = 4;         // maxDets values per accumulate

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
    StrataArgs<true> sa{scales, zt, {}, NA, rec_val};
    for (int a = 0; a < ES_MAX_NA; ++a)
        for (int k = 0; k < 4; ++k) sa.st.v[a][k] = a < NA ? strata[a * 4 + k] : 0.0;
    for (int a = 0; a < NA; ++a)
        EP24_REQUIRE(sa.st.v[a][0] <= sa.st.v[a][1] && sa.st.v[a][2] <= sa.st.v[a][3], EP24_E_ARG,
                     "eval_match_strata: strata[%d] = {%g, %g, %g, %g}: a range needs lo <= hi", a, sa.st.v[a][0], sa.st.v[a][1],
                     sa.st.v[a][2], sa.st.v[a][3]);
    EP24_REQUIRE(B == 0 || (scales && zt), EP24_E_ARG, "eval_match_strata: scales or zt is null");
    return eval_match_launch("eval_match_strata", labels, L, B, rows, ncols, row_off, keep, keep_stride, count, conf, cls, num_classes,
                             iou_type, ray_cs, iou_thr, max_dets, seq_base, sort_scratch, P, sa, rec_key, rec_cls, rec_p, rec_m, rec_count,
                             npig, err, S_);
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
