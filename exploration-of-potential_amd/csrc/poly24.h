// ep24 - exact area IoU of two 24-gons ("poly24", iou_type 2 of the evaluator).
//
// Signed trapezoid decomposition: with s_e = sign(x1 - x0) of an edge and h_e(x) its height above a common baseline, the
// indicator of a simple polygon A above the baseline is -sigma_A * sum_e s_e [x in e][y < h_e(x)] (sigma = sign of the shoelace
// area), so  |A and B| = sigma_A sigma_B * sum_e sum_f s_e s_f * integral over the common x range of min(h_e, h_f).
// No inside tests, no sorting, continuous in the vertices: coincident edges, shared vertices and identical polygons are ordinary
// cases.  Everything is double; the library is built with -ffp-contract=off, so every product and sum rounds on its own.
//
// The computation comes in three pieces (poly24_prepare, poly24_edge_accumulate, poly24_finish) that poly24_inter runs in a row on
// one lane.  ep24_paste_labels (csrc/paste.hip) spreads the middle piece over 24 lanes, one edge of `a` each.
#pragma once
#include "common.h"

// The 24 points of a detection (cx, cy, r[24]) as (x, y) pairs: c + r_k * (cos, sin)(15 deg * k) with the table cs[48] the host
// computes in float64 and rounds; product and sum are separate fp32 operations.  The one place the evaluator (det_geometry<48>)
// and the polygon NMS form them.
__device__ __forceinline__ void poly24_det_vertices(const float* q26, const float* cs, float* out) {
    for (int k = 0; k < 24; ++k) {
        out[2 * k] = q26[0] + q26[2 + k] * cs[k];
        out[2 * k + 1] = q26[1] + q26[2 + k] * cs[24 + k];
    }
}

// height of the edge (xa, ha) -> (xb, hb), xa < xb, at x
__device__ __forceinline__ double poly24_height(double x, double xa, double ha, double xb, double hb) {
    return ha + ((x - xa) * (hb - ha)) / (xb - xa);
}

// What poly24_prepare found: a NaN coordinate, vertex boxes that do not overlap with positive width and height, or a pair to intersect
enum { POLY24_NAN = 0, POLY24_APART = 1, POLY24_MEET = 2 };

// a, b: 24 vertices each as (x, y) pairs of fp32, promoted here.  For a pair to intersect: *yb = the baseline of the heights and
// *sa, *sb = the signed shoelace areas of a and b.
__device__ __forceinline__ int poly24_prepare(const float* a, const float* b, double* yb_out, double* sa_out, double* sb_out) {
    double axl = INFINITY, axh = -INFINITY, ayl = INFINITY, ayh = -INFINITY;
    double bxl = INFINITY, bxh = -INFINITY, byl = INFINITY, byh = -INFINITY;
    bool nan = false;
    for (int k = 0; k < 24; ++k) {
        const double ax = a[2 * k], ay = a[2 * k + 1], bx = b[2 * k], by = b[2 * k + 1];
        nan |= ax != ax || ay != ay || bx != bx || by != by;
        axl = fmin(axl, ax); axh = fmax(axh, ax); ayl = fmin(ayl, ay); ayh = fmax(ayh, ay);
        bxl = fmin(bxl, bx); bxh = fmax(bxh, bx); byl = fmin(byl, by); byh = fmax(byh, by);
    }
    if (nan) return POLY24_NAN;
    if (!(fmin(axh, bxh) - fmax(axl, bxl) > 0.0 && fmin(ayh, byh) - fmax(ayl, byl) > 0.0)) return POLY24_APART;
    // the shoelace areas and the heights are taken relative to (xb, yb), the low corner of the joint box: a translation, exact in
    // real arithmetic, that keeps the rounding relative to the objects' size and not to their position in the image
    const double xb = fmin(axl, bxl), yb = fmin(ayl, byl);
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < 24; ++k) {
        const int k1 = k == 23 ? 0 : k + 1;
        const double ax0 = (double)a[2 * k] - xb, ay0 = (double)a[2 * k + 1] - yb;
        const double ax1 = (double)a[2 * k1] - xb, ay1 = (double)a[2 * k1 + 1] - yb;
        sa += ax0 * ay1 - ax1 * ay0;
        const double bx0 = (double)b[2 * k] - xb, by0 = (double)b[2 * k + 1] - yb;
        const double bx1 = (double)b[2 * k1] - xb, by1 = (double)b[2 * k1 + 1] - yb;
        sb += bx0 * by1 - bx1 * by0;
    }
    sa *= 0.5;
    sb *= 0.5;
    *yb_out = yb;
    *sa_out = sa;
    *sb_out = sb;
    return POLY24_MEET;
}

// S += the signed terms of edge i of a against the 24 edges of b, in the order of b's edges
__device__ __forceinline__ void poly24_edge_accumulate(const float* a, const float* b, int i, double yb, double& S) {
    const int i1 = i == 23 ? 0 : i + 1;
    const double ex0 = a[2 * i], ex1 = a[2 * i1];
    if (ex0 == ex1) return;
    const double eh0 = (double)a[2 * i + 1] - yb, eh1 = (double)a[2 * i1 + 1] - yb;
    const bool er = ex1 > ex0;                            // left to right as stored
    const double exa = er ? ex0 : ex1, eha = er ? eh0 : eh1, exb = er ? ex1 : ex0, ehb = er ? eh1 : eh0;
    for (int j = 0; j < 24; ++j) {
        const int j1 = j == 23 ? 0 : j + 1;
        const double fx0 = b[2 * j], fx1 = b[2 * j1];
        if (fx0 == fx1) continue;
        const double fh0 = (double)b[2 * j + 1] - yb, fh1 = (double)b[2 * j1 + 1] - yb;
        const bool fr = fx1 > fx0;
        const double fxa = fr ? fx0 : fx1, fha = fr ? fh0 : fh1, fxb = fr ? fx1 : fx0, fhb = fr ? fh1 : fh0;
        const double xl = fmax(exa, fxa), xr = fmin(exb, fxb);
        if (!(xl < xr)) continue;
        const double al = poly24_height(xl, exa, eha, exb, ehb), ar = poly24_height(xr, exa, eha, exb, ehb);
        const double bl = poly24_height(xl, fxa, fha, fxb, fhb), br = poly24_height(xr, fxa, fha, fxb, fhb);
        const double dl = al - bl, dr = ar - br;
        const double ml = fmin(al, bl), mr = fmin(ar, br);
        double term;
        if ((dl < 0.0 && dr > 0.0) || (dl > 0.0 && dr < 0.0)) {
            // the edges cross inside the range: two trapezoids under min(e, f) that meet at the crossing height
            const double t = dl / (dl - dr);
            const double xm = xl + t * (xr - xl), hm = al + t * (ar - al);
            term = 0.5 * (ml + hm) * (xm - xl) + 0.5 * (hm + mr) * (xr - xm);
        } else {
            term = 0.5 * (ml + mr) * (xr - xl);
        }
        S += (er == fr) ? term : -term;
    }
}

// the intersection area from the sum S of all terms and the signed areas; *aa, *ab = the absolute areas
__device__ __forceinline__ double poly24_finish(double S, double sa, double sb, double* aa_out, double* ab_out) {
    const double aa = fabs(sa), ab = fabs(sb);
    const double sg = ((sa < 0.0) != (sb < 0.0)) ? -S : S;
    *aa_out = aa;
    *ab_out = ab;
    return fmin(fmax(sg, 0.0), fmin(aa, ab));
}

// The intersection area of two 24-gons and their absolute shoelace areas (*aa of a, *ab of b).  Any NaN coordinate: NaN and NaN
// areas.  Vertex boxes that do not overlap with positive width and height: exactly 0.0, and the areas, which are then not needed,
// are left at 0.0.
__device__ inline double poly24_inter(const float* a, const float* b, double* aa_out, double* ab_out) {
    double yb, sa, sb;
    const int kind = poly24_prepare(a, b, &yb, &sa, &sb);
    if (kind != POLY24_MEET) {
        *aa_out = *ab_out = kind == POLY24_NAN ? __builtin_nan("") : 0.0;
        return *aa_out;
    }
    double S = 0.0;
    for (int i = 0; i < 24; ++i) poly24_edge_accumulate(a, b, i, yb, S);
    return poly24_finish(S, sa, sb, aa_out, ab_out);
}

// Area IoU.  Any NaN coordinate gives NaN (it never matches); vertex boxes that do not overlap with positive width and height
// give exactly 0.0.
__device__ inline double poly24_iou(const float* a, const float* b) {
    double aa, ab;
    const double inter = poly24_inter(a, b, &aa, &ab);
    if (inter != inter) return inter;                         // a NaN coordinate (fmin / fmax in poly24_finish never return one)
    const double uni = aa + ab - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}
