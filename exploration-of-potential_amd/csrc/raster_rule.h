// ep24 - the crossing rule of the polygon rasteriser, shared by ep24_poly24_raster (csrc/mask.hip) and the "poly24" region of
// ep24_featmap_response (csrc/featmap.hip): one definition, so the two cannot drift apart.
//
// A point (px, py) is inside a polygon iff an odd number of COUNTING edges cross its row to the right of it.  With yc = py the
// edge (x0, y0) -> (x1, y1) counts iff (y0 <= yc) != (y1 <= yc); its crossing is x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) in
// double, evaluated as written (the library is built with -ffp-contract=off), and it lies to the right iff px < crossing.  A NaN
// coordinate never counts or never compares: such an edge contributes nothing.  Left and top boundaries are in, right and bottom out.
#pragma once
#include "common.h"

// true iff the edge counts for the row yc; *xc is then its crossing
__device__ __forceinline__ bool raster_edge_crossing(double x0, double y0, double x1, double y1, double yc, double* xc) {
    const bool counts = (y0 <= yc) != (y1 <= yc);
    if (counts) *xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0);
    return counts;
}

// the rule for one point against n vertices held as (x, y) pairs of doubles (any address space the caller can index)
template <typename V>
__device__ __forceinline__ bool raster_point_inside(const V& v, int n, double px, double py) {
    bool in = false;
    for (int k = 0; k < n; ++k) {
        const int k1 = k == n - 1 ? 0 : k + 1;
        double xc;
        if (raster_edge_crossing(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1], py, &xc) && px < xc) in = !in;
    }
    return in;
}
