// ep24 - COCO segmentations -> instance masks on the GPU: what pycocotools' annToMask (rleFrPoly, rleMerge as a union,
// rleDecode; rleDecode alone for an RLE) computes on the host, written straight into the buffer ep24_ray24 reads.
//
// rleFrPoly walks a polygon's edges at 5x scale into a dense point sequence, keeps the points where the x coordinate
// changes and lands on a pixel centre line ("boundary points": a column x and the row y from which the column's value
// flips), sorts them and takes differences.  Per pixel that is: mask(y, x) = parity of the polygon's boundary points
// (x, y') with y' <= y.  So nothing is sorted here:
//   poly_xor   one thread per dense point; a boundary point (x, y) flips bit b of mask byte [y][x], b = the polygon's
//              index within its annotation modulo 7, with an atomic XOR on the aligned 32-bit word (masks start at any
//              byte).  XOR commutes: the bytes do not depend on the order the threads arrive in.
//   poly_scan  one thread per column walks down with a running XOR of bits 0..6 and writes "any bit set" - the union
//              of up to 7 polygons.  Bit 7 carries the union of the earlier rounds of an annotation with more than 7
//              polygons: every round but an annotation's last writes its result there, the last writes 0 / 1.
//   rle        one thread per column: the number of run ends at or before the column's first column-major position by
//              binary search in the prefix sums, then down the column run by run; its parity is the pixel.  (A
//              search per pixel is twelve times slower on 427 x 640 masks: DESIGN section 7.)
// The arithmetic that decides a point is the C code's double sequence, operation by operation (-ffp-contract=off).
#include "common.h"

namespace {

struct Pt { int u, v; };

// point d of edge e = {xs, ys, xe, ye, ...}: rleFrPoly's upsample-and-walk loop body
__device__ __forceinline__ Pt edge_point(const int* e, int d) {
    int xs = e[0], ys = e[1], xe = e[2], ye = e[3];
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    if (dx == 0 && dy == 0) return {xs, ys};                          // s = 0 / 0; one point whose v no one reads
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    if (dx >= dy) {
        const double s = (double)(ye - ys) / (double)dx;
        const int t = flip ? dx - d : d;
        return {t + xs, (int)(((double)ys + s * (double)t) + .5)};
    }
    const double s = (double)(xe - xs) / (double)dy;
    const int t = flip ? dy - d : d;
    return {(int)(((double)xs + s * (double)t) + .5), t + ys};
}

// edges[ne][8] int32 = {xs, ys, xe, ye, annotation, bit, first edge of its polygon, 0}; start[ne + 1] = first dense
// point of every edge (start[0] need not be 0: a round is a slice of the batch's edge table)
__global__ __launch_bounds__(256) void poly_xor_kernel(uint32_t* words, long total, const long long* desc, const int* edges,
                                                       const long long* start, int ne) {
    const long long q0 = start[0], npts = start[ne] - q0;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < npts; g += (long long)gridDim.x * 256) {
        const long long q = q0 + g;
        int lo = 0, hi = ne - 1;                                     // last edge with start[e] <= q
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (start[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const int* e = edges + (long)lo * 8;
        const int d = (int)(q - start[lo]);
        if (d == 0 && e[6]) continue;                                // the polygon's first point has no predecessor
        const Pt a = edge_point(e, d);
        const Pt b = d ? edge_point(e, d - 1) : edge_point(e - 8, (int)(start[lo] - start[lo - 1]) - 1);
        if (a.u == b.u) continue;
        double xd = (double)(a.u < b.u ? a.u : a.u - 1);
        xd = (xd + .5) / 5 - .5;
        const long long* dsc = desc + (long)e[4] * 6;
        const int H = (int)dsc[1], W = (int)dsc[2];
        if (floor(xd) != xd || xd < 0 || xd > (double)(W - 1)) continue;
        double yd = (double)(a.v < b.v ? a.v : b.v);
        yd = (yd + .5) / 5 - .5;
        if (yd < 0) yd = 0; else if (yd > (double)H) yd = (double)H;
        const int x = (int)xd, y = (int)ceil(yd);
        if (y >= H) continue;                                        // a flip below the last row changes nothing
        const long byte = dsc[0] + (long)y * dsc[5] + x;
        if (byte < 0 || byte >= total) continue;
        atomicXor(words + (byte >> 2), 1u << (8 * (int)(byte & 3) + e[5]));
    }
}

// items[n] = annotation * 2 + (this is the annotation's last round); blockIdx.y = item, one thread per column
__global__ __launch_bounds__(64) void poly_scan_kernel(uint8_t* masks, long total, const long long* desc, const int* items) {
    const int it = items[blockIdx.y];
    const long long* dsc = desc + (long)(it >> 1) * 6;
    const int H = (int)dsc[1], W = (int)dsc[2];
    const long ld = dsc[5];
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W || dsc[0] < 0 || dsc[0] + (long)(H - 1) * ld + W > total) return;
    uint8_t* col = masks + dsc[0] + x;
    const bool last = it & 1;
    unsigned run = 0;
    int y = 0;
    for (; y + 8 <= H; y += 8) {                                     // eight rows in flight, then their stores
        unsigned v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = col[(long)(y + i) * ld];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            run ^= v[i] & 0x7Fu;
            const unsigned on = (run != 0) | (v[i] >> 7);
            col[(long)(y + i) * ld] = (uint8_t)(last ? on : on << 7);
        }
    }
    for (; y < H; ++y) {
        const unsigned v = col[(long)y * ld];
        run ^= v & 0x7Fu;
        const unsigned on = (run != 0) | (v >> 7);
        col[(long)y * ld] = (uint8_t)(last ? on : on << 7);
    }
}

// runs[n][3] int64 = {annotation, first entry in ends, number of runs}; ends = inclusive prefix sums of the counts
__global__ __launch_bounds__(64) void rle_kernel(uint8_t* masks, long total, const long long* desc, const long long* runs,
                                                 const long long* ends) {
    const long long* r = runs + (long)blockIdx.y * 3;
    const long long* dsc = desc + r[0] * 6;
    const int H = (int)dsc[1], W = (int)dsc[2], n = (int)r[2];
    const long ld = dsc[5];
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W || dsc[0] < 0 || dsc[0] + (long)(H - 1) * ld + W > total) return;
    const long long* end = ends + r[1];
    const long long never = 0x7FFFFFFFFFFFFFFFLL;
    long long q = (long long)x * H;
    int lo = 0, hi = n;                                              // number of runs that end at or before q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (end[mid] <= q) lo = mid + 1; else hi = mid;
    }
    long long next = lo < n ? end[lo] : never;
    uint8_t* col = masks + dsc[0] + x;
    for (int y = 0; y < H; ++y, ++q) {
        while (next <= q) { ++lo; next = lo < n ? end[lo] : never; }   // also over empty runs
        col[(long)y * ld] = (uint8_t)(lo & 1);
    }
}

}  // namespace

extern "C" int ep24_cocomask_poly_xor(uint8_t* masks, int64_t total, const int64_t* desc, const int32_t* edges,
                                      const int64_t* start, int ne, int64_t npts, void* stream) {
    if (ne == 0 || npts == 0) return EP24_OK;
    EP24_REQUIRE(masks && desc && edges && start && ne > 0 && npts > 0 && total > 0, EP24_E_ARG, "cocomask_poly_xor: bad arguments");
    EP24_REQUIRE(((uintptr_t)masks & 3) == 0 && (total & 3) == 0, EP24_E_ARG,
                 "cocomask_poly_xor: the mask buffer and its length must be multiples of 4 bytes");
    const long blocks = (npts + 255) / 256;
    hipLaunchKernelGGL(poly_xor_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t*)masks, (long)total, (const long long*)desc, edges, (const long long*)start, ne);
    EP24_LAUNCH_CHECK("ep24_cocomask_poly_xor");
    return EP24_OK;
}

extern "C" int ep24_cocomask_poly_scan(uint8_t* masks, int64_t total, const int64_t* desc, const int32_t* items, int n, int max_w,
                                       void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(masks && desc && items && n > 0 && n <= 65535 && max_w > 0 && total > 0, EP24_E_ARG,
                 "cocomask_poly_scan: bad arguments");
    hipLaunchKernelGGL(poly_scan_kernel, dim3((max_w + 63) / 64, n), dim3(64), 0, (hipStream_t)stream, masks, (long)total,
                       (const long long*)desc, items);
    EP24_LAUNCH_CHECK("ep24_cocomask_poly_scan");
    return EP24_OK;
}

extern "C" int ep24_cocomask_rle(uint8_t* masks, int64_t total, const int64_t* desc, const int64_t* runs, const int64_t* ends, int n,
                                 int max_w, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(masks && desc && runs && ends && n > 0 && n <= 65535 && max_w > 0 && total > 0, EP24_E_ARG,
                 "cocomask_rle: bad arguments");
    hipLaunchKernelGGL(rle_kernel, dim3((max_w + 63) / 64, n), dim3(64), 0, (hipStream_t)stream, masks, (long)total,
                       (const long long*)desc, (const long long*)runs, (const long long*)ends);
    EP24_LAUNCH_CHECK("ep24_cocomask_rle");
    return EP24_OK;
}
