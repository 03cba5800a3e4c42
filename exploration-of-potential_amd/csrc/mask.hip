// ep24 - instance masks of 24-point polygons: rasteriser, byte <-> bit packing and mask IoU.
//
// Packed mask: uint32 [N][H][WW], WW = ceil(W / 32); pixel x is bit x & 31 of word x >> 5, bits at x >= W are zero.
//   poly24_vertices  (cx, cy, 24 radii) rows -> [n][24][2] vertices, c / ratio + (r_k / ratio) * (cos, sin)(15 deg k) in fp32
//   poly24_raster    one wave per (object, row): lanes 0..23 find the row's edge crossings, every lane then builds words as the
//                    XOR over the counting edges of "the bits left of the crossing"
//   mask_pack_u8     one wave per (object, row): a ballot over 64 pixels gives two words
//   mask_unpack_u8   one thread per pixel
//   mask_iou         one wave per (A, B) pair: AND + popcount over the rows and words of the two boxes' overlap only
//
// Pixel rule of the rasteriser: the centre of pixel (x, y) is the point (x, y) (augment.hip's convention: pixel i covers
// [i - 0.5, i + 0.5)).  With yc = (double)y the edge (x0, y0) -> (x1, y1) counts iff (y0 <= yc) != (y1 <= yc), its crossing is
// xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) in double, evaluated as written, and pixel x is set iff an odd number of counting
// edges have (double)x < xc.  For an integer x that is x < ceil(xc), so the word w of the row is the XOR over the counting edges
// of prefix(clamp(ceil(xc) - 32 w, 0, 32)), prefix(k) = the k lowest bits.  Left and top boundaries are in, right and bottom out.
//
// Determinism: box and area are integer atomics (min, max, add) over the rows of an object - the order does not matter.
#include "common.h"
#include "raster_rule.h"

namespace {

__device__ __forceinline__ uint32_t prefix_bits(int k) { return k >= 32 ? 0xFFFFFFFFu : (k <= 0 ? 0u : ((1u << k) - 1u)); }

__global__ __launch_bounds__(256) void poly24_vertices_kernel(const float* det, int ncols, int n, const float* cs, float ratio,
                                                              float* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * 24) return;
    const long o = i / 24;
    const int k = (int)(i - o * 24);
    const float* q = det + o * ncols;
    const float cx = q[0] / ratio, cy = q[1] / ratio, r = q[2 + k] / ratio;
    out[2 * i] = cx + r * cs[k];
    out[2 * i + 1] = cy + r * cs[24 + k];
}

// bbox[n] = (W, H, -1, -1): the empty marker and the identity of the min / max atomics; area[n] = 0
__global__ __launch_bounds__(256) void mask_stats_init_kernel(int32_t* bbox, int32_t* area, int N, int H, int W) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    bbox[4 * i] = W;
    bbox[4 * i + 1] = H;
    bbox[4 * i + 2] = -1;
    bbox[4 * i + 3] = -1;
    area[i] = 0;
}

// the wave's row y of object n holds cnt set pixels (this lane's share) between xlo and xhi (this lane's; W and -1 for none)
__device__ __forceinline__ void row_stats(int32_t* bbox, int32_t* area, long n, int y, int cnt, int xlo, int xhi, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        xlo = min(xlo, __shfl_xor(xlo, o, 64));
        xhi = max(xhi, __shfl_xor(xhi, o, 64));
    }
    if (lane == 0 && cnt > 0) {
        atomicAdd(&area[n], cnt);
        atomicMin(&bbox[4 * n], xlo);
        atomicMin(&bbox[4 * n + 1], y);
        atomicMax(&bbox[4 * n + 2], xhi);
        atomicMax(&bbox[4 * n + 3], y);
    }
}

__global__ __launch_bounds__(256) void poly24_raster_kernel(const float* verts, long rows, int H, int W, int WW, uint32_t* bits,
                                                            int32_t* bbox, int32_t* area) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= rows) return;                                  // whole waves leave together
    const long n = wid / H;
    const int y = (int)(wid - n * H);
    const double yc = (double)y;
    int c = 0;                                                // clamp(ceil(xc), 0, W) of a counting edge, 0 otherwise (and for a NaN)
    bool counts = false;
    if (lane < 24) {
        const float* v = verts + n * 48;
        const int k1 = lane == 23 ? 0 : lane + 1;
        const double x0 = v[2 * lane], y0 = v[2 * lane + 1], x1 = v[2 * k1], y1 = v[2 * k1 + 1];
        double xc;
        counts = raster_edge_crossing(x0, y0, x1, y1, yc, &xc);       // the rule itself: raster_rule.h
        if (counts) {
            const double cd = ceil(xc);
            c = cd > 0.0 ? (cd < (double)W ? (int)cd : W) : 0;
        }
    }
    const bool any = __ballot(counts) != 0;                   // rows outside the polygon's y range: zeros, no edge work
    uint32_t* row = bits + wid * WW;
    int cnt = 0, xlo = W, xhi = -1;
    for (int w0 = 0; w0 < WW; w0 += 64) {
        const int w = w0 + lane;
        uint32_t word = 0u;
        if (any)
            for (int k = 0; k < 24; ++k) word ^= prefix_bits(__shfl(c, k, 64) - 32 * w);
        if (w < WW) {
            row[w] = word;
            if (word) {
                cnt += __popc(word);
                xlo = min(xlo, 32 * w + __ffs((int)word) - 1);
                xhi = max(xhi, 32 * w + 31 - __clz((int)word));
            }
        }
    }
    if (any) row_stats(bbox, area, n, y, cnt, xlo, xhi, lane);
}

__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* src, long rows, int H, int W, int WW, uint32_t* bits,
                                                        int32_t* bbox, int32_t* area) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= rows) return;
    const long n = wid / H;
    const int y = (int)(wid - n * H);
    const uint8_t* s = src + wid * W;
    uint32_t* row = bits + wid * WW;
    int cnt = 0, xlo = W, xhi = -1;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool on = x < W && s[x] != 0;
        const unsigned long long m = __ballot(on);
        const int w = (x0 >> 5) + lane;                       // lanes 0 and 1 store the two words
        if (lane < 2 && w < WW) row[w] = (uint32_t)(m >> (32 * lane));
        if (on) {
            cnt += 1;
            xlo = min(xlo, x);
            xhi = max(xhi, x);
        }
    }
    row_stats(bbox, area, n, y, cnt, xlo, xhi, lane);
}

__global__ __launch_bounds__(256) void mask_unpack_kernel(const uint32_t* bits, long total, int W, int WW, uint8_t* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long r = i / W;
    const int x = (int)(i - r * W);
    out[i] = (uint8_t)((bits[r * WW + (x >> 5)] >> (x & 31)) & 1u);
}

__global__ __launch_bounds__(256) void mask_iou_kernel(const uint32_t* a, const int32_t* a_bbox, const int32_t* a_area, int G,
                                                       const uint32_t* b, const int32_t* b_bbox, const int32_t* b_area, int D, int H,
                                                       int W, int WW, int64_t* inter, double* iou) {
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long)G * D) return;
    const int g = (int)(pair / D), d = (int)(pair - (long)g * D);
    // overlap of the two boxes, kept inside the canvas whatever the caller's boxes say
    const int x0 = max(max(a_bbox[4 * g], b_bbox[4 * d]), 0), y0 = max(max(a_bbox[4 * g + 1], b_bbox[4 * d + 1]), 0);
    const int x1 = min(min(a_bbox[4 * g + 2], b_bbox[4 * d + 2]), W - 1), y1 = min(min(a_bbox[4 * g + 3], b_bbox[4 * d + 3]), H - 1);
    long long cnt = 0;
    if (x0 <= x1 && y0 <= y1) {
        const int w0 = x0 >> 5, nw = (x1 >> 5) - w0 + 1;
        const long cells = (long)(y1 - y0 + 1) * nw;
        const uint32_t* pa = a + (long)g * H * WW;
        const uint32_t* pb = b + (long)d * H * WW;
        for (long i = lane; i < cells; i += 64) {
            const long r = i / nw;
            const long o = (y0 + r) * WW + w0 + (i - r * nw);
            cnt += __popc(pa[o] & pb[o]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) {
        const long long uni = (long long)a_area[g] + (long long)b_area[d] - cnt;
        inter[pair] = cnt;
        iou[pair] = uni != 0 ? (double)cnt / (double)uni : 0.0;
    }
}

}  // namespace

#define S_ (hipStream_t) stream

static bool mask_shape_ok(long N, int H, int W) {
    return N >= 0 && H > 0 && W > 0 && (long)H * W <= 0x7FFFFFFFL && N * H <= 0x7FFFFFFFL * 4;
}

extern "C" int ep24_poly24_vertices(const float* det, int ncols, int n, const float* ray_cs, float ratio, float* verts, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(det && ray_cs && verts && n > 0 && ncols >= 26, EP24_E_ARG, "poly24_vertices: bad arguments");
    hipLaunchKernelGGL(poly24_vertices_kernel, dim3((unsigned)(((long)n * 24 + 255) / 256)), dim3(256), 0, S_, det, ncols, n, ray_cs,
                       ratio, verts);
    EP24_LAUNCH_CHECK("ep24_poly24_vertices");
    return EP24_OK;
}

extern "C" int ep24_poly24_raster(const float* verts, int N, int H, int W, uint32_t* bits, int32_t* bbox, int32_t* area, void* stream) {
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(verts && bits && bbox && area && N > 0, EP24_E_ARG, "poly24_raster: bad arguments");
    EP24_REQUIRE(mask_shape_ok(N, H, W), EP24_E_UNSUPPORTED, "poly24_raster: N=%d H=%d W=%d (H * W < 2^31, N * H < 2^33)", N, H, W);
    const long rows = (long)N * H;
    hipLaunchKernelGGL(mask_stats_init_kernel, dim3((N + 255) / 256), dim3(256), 0, S_, bbox, area, N, H, W);
    hipLaunchKernelGGL(poly24_raster_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S_, verts, rows, H, W, (W + 31) / 32, bits,
                       bbox, area);
    EP24_LAUNCH_CHECK("ep24_poly24_raster");
    return EP24_OK;
}

extern "C" int ep24_mask_pack_u8(const uint8_t* masks, int N, int H, int W, uint32_t* bits, int32_t* bbox, int32_t* area, void* stream) {
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(masks && bits && bbox && area && N > 0, EP24_E_ARG, "mask_pack_u8: bad arguments");
    EP24_REQUIRE(mask_shape_ok(N, H, W), EP24_E_UNSUPPORTED, "mask_pack_u8: N=%d H=%d W=%d (H * W < 2^31, N * H < 2^33)", N, H, W);
    const long rows = (long)N * H;
    hipLaunchKernelGGL(mask_stats_init_kernel, dim3((N + 255) / 256), dim3(256), 0, S_, bbox, area, N, H, W);
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S_, masks, rows, H, W, (W + 31) / 32, bits, bbox,
                       area);
    EP24_LAUNCH_CHECK("ep24_mask_pack_u8");
    return EP24_OK;
}

extern "C" int ep24_mask_unpack_u8(const uint32_t* bits, int N, int H, int W, uint8_t* masks, void* stream) {
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(bits && masks && N > 0, EP24_E_ARG, "mask_unpack_u8: bad arguments");
    EP24_REQUIRE(mask_shape_ok(N, H, W) && (long)N * H * W <= 0x7FFFFFFFL * 256, EP24_E_UNSUPPORTED,
                 "mask_unpack_u8: N=%d H=%d W=%d (H * W < 2^31, N * H * W < 2^39)", N, H, W);
    const long total = (long)N * H * W;
    hipLaunchKernelGGL(mask_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_, bits, total, W, (W + 31) / 32, masks);
    EP24_LAUNCH_CHECK("ep24_mask_unpack_u8");
    return EP24_OK;
}

extern "C" int ep24_mask_iou(const uint32_t* a_bits, const int32_t* a_bbox, const int32_t* a_area, int G, const uint32_t* b_bits,
                             const int32_t* b_bbox, const int32_t* b_area, int D, int H, int W, int64_t* inter, double* iou,
                             void* stream) {
    if ((long)G * D == 0) return EP24_OK;
    EP24_REQUIRE(a_bits && a_bbox && a_area && b_bits && b_bbox && b_area && inter && iou && G > 0 && D > 0, EP24_E_ARG,
                 "mask_iou: bad arguments");
    EP24_REQUIRE(mask_shape_ok(G, H, W) && mask_shape_ok(D, H, W) && (long)G * D <= 0x7FFFFFFFL * 4, EP24_E_UNSUPPORTED,
                 "mask_iou: G=%d D=%d H=%d W=%d (H * W < 2^31, G * D < 2^33)", G, D, H, W);
    hipLaunchKernelGGL(mask_iou_kernel, dim3((unsigned)(((long)G * D + 3) / 4)), dim3(256), 0, S_, a_bits, a_bbox, a_area, G, b_bits,
                       b_bbox, b_area, D, H, W, (W + 31) / 32, inter, iou);
    EP24_LAUNCH_CHECK("ep24_mask_iou");
    return EP24_OK;
}
