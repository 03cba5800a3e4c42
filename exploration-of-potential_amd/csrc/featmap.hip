// ep24 - feature-map response study (the contract is in include/ep24.h, E4).
//
//   featmap_mean      channel mean of bf16 NHWC rows: a sub-wave of G lanes per row (G = the power of two that holds C / 8 sixteen-byte
//                     chunks, at most 64), 256 / G rows per workgroup, a lane adds its chunks' eight values in index order, then a
//                     xor-shuffle tree over the G lanes.  No LDS, no atomics; the order is a function of C alone.
//   featmap_range     one workgroup per map: fminf / fmaxf over the cells (NaNs drop out), shuffles, then the four waves through LDS
//   featmap_render    one thread per 4 adjacent output pixels of one row: colour index of the cell, look-up, optional blend over the
//                     network input, 12 bytes as three dwords where the address allows it
//   featmap_response  one workgroup per (image, label row): the region's cells in a fixed thread-strided order, double sums
//
// The fp32 arithmetic is scalar and every operation rounds on its own (-ffp-contract=off).
#include "common.h"
#include "raster_rule.h"

namespace {

constexpr float LIM = 1048576.0f;                             // 2^20

__device__ __forceinline__ float bf_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

// G lanes per row, G in {1, 2, ..., 64}; chunks = C / 8
template <int G>
__global__ __launch_bounds__(256) void featmap_mean_kernel(const uint16_t* __restrict__ x, int64_t ld, int64_t M, int chunks, float fC,
                                                           float* __restrict__ out) {
    constexpr int RPW = 256 / G;                              // rows per workgroup
    const int sub = threadIdx.x % G;
    const int64_t r0 = (int64_t)(threadIdx.x / G);
    for (int64_t base = (int64_t)blockIdx.x * RPW; base < M; base += (int64_t)gridDim.x * RPW) {   // base is uniform: whole waves loop together
        const int64_t r = base + r0;
        float acc = 0.0f;
        if (r < M) {
            const uint16_t* row = x + r * ld;
            for (int c = sub; c < chunks; c += G) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + (int64_t)c * 8);      // 16 bytes: eight bf16
                acc += bf_lo(v.x);
                acc += bf_hi(v.x);
                acc += bf_lo(v.y);
                acc += bf_hi(v.y);
                acc += bf_lo(v.z);
                acc += bf_hi(v.z);
                acc += bf_lo(v.w);
                acc += bf_hi(v.w);
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);                  // every lane of the wave takes part
        if (sub == 0 && r < M) out[r] = acc / fC;
    }
}

__global__ __launch_bounds__(256) void featmap_range_kernel(const float* __restrict__ maps, int64_t cells, float* __restrict__ range) {
    __shared__ float slo[4], shi[4];
    const float* m = maps + (int64_t)blockIdx.x * cells;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < cells; i += 256) {
        const float v = m[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        slo[threadIdx.x >> 6] = lo;
        shi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        range[2 * (int64_t)blockIdx.x] = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
        range[2 * (int64_t)blockIdx.x + 1] = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    }
}

__device__ __forceinline__ int color_index(float v, float lo, float hi) {
    const float t = (v - lo) / (hi - lo);
    const float q = t * 256.0f;
    if (!(hi > lo) || !(q >= 0.0f)) return 0;
    return q >= 255.0f ? 255 : (int)q;
}

__device__ __forceinline__ uint32_t base_byte(float b) { return !(b >= 0.0f) ? 0u : (b >= 255.0f ? 255u : (uint32_t)(int)b); }

__global__ __launch_bounds__(256) void featmap_render_kernel(const float* __restrict__ maps, int H, int W, int scale,
                                                             const float* __restrict__ range, const uint8_t* __restrict__ lut,
                                                             const float* __restrict__ base, int alpha, uint8_t* __restrict__ out,
                                                             int quads, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // (n, Y, quad)
    if (i >= total) return;
    const int HS = H * scale, WS = W * scale;
    const int64_t ny = i / quads;
    const int X0 = (int)(i - ny * quads) * 4;
    const int64_t n = ny / HS;
    const int Y = (int)(ny - n * HS);
    const int npx = min(4, WS - X0);
    const float lo = range[2 * n], hi = range[2 * n + 1];
    const float* mrow = maps + (n * H + Y / scale) * W;
    uint32_t pix[4] = {0u, 0u, 0u, 0u};
    int cell = -1;
    uint32_t col = 0u;
    for (int j = 0; j < npx; ++j) {
        const int X = X0 + j, cx = X / scale;
        if (cx != cell) {                                             // adjacent pixels mostly share their cell
            cell = cx;
            const uint8_t* c = lut + 3 * color_index(mrow[cx], lo, hi);
            col = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
        }
        uint32_t p = col;
        if (base) {
            p = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const uint32_t b = base_byte(base[((n * 3 + ch) * HS + Y) * WS + X]);
                const uint32_t q = (col >> (8 * ch)) & 255u;
                p |= ((b * (uint32_t)(256 - alpha) + q * (uint32_t)alpha + 128u) >> 8) << (8 * ch);
            }
        }
        pix[j] = p;
    }
    uint8_t* o = out + (ny * WS + X0) * 3;
    if (npx == 4 && (((uintptr_t)o) & 3) == 0) {                      // 12 aligned bytes: three dword stores
        uint32_t* o4 = (uint32_t*)o;
        o4[0] = pix[0] | (pix[1] << 24);
        o4[1] = (pix[1] >> 8) | (pix[2] << 16);
        o4[2] = (pix[2] >> 16) | (pix[3] << 8);
    } else {
        for (int j = 0; j < npx; ++j) {
            o[3 * j] = (uint8_t)pix[j];
            o[3 * j + 1] = (uint8_t)(pix[j] >> 8);
            o[3 * j + 2] = (uint8_t)(pix[j] >> 16);
        }
    }
}

__global__ __launch_bounds__(256) void featmap_response_kernel(const float* __restrict__ maps, int H, int W, int stride,
                                                               const float* __restrict__ labels, int L, int mode,
                                                               double* __restrict__ sum, int32_t* __restrict__ count,
                                                               double* __restrict__ mean) {
    __shared__ double vert[48];
    __shared__ double wsum[4];
    __shared__ int wcnt[4];
    const int64_t row = blockIdx.x;                                   // b * L + l
    const int64_t b = row / L;
    const float* q = labels + row * 51;
    // every thread forms the same sum, bounds and verdict from the same 51 values: the branches below are uniform
    float tot = 0.0f;
    for (int k = 0; k < 51; ++k) tot += q[k];
    if (!(tot > 0.0f)) {                                              // padding (also a NaN sum): leaves at once
        if (threadIdx.x == 0) {
            sum[row] = 0.0;
            count[row] = 0;
            mean[row] = 0.0;
        }
        return;
    }
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    bool ok = true;
    for (int k = 0; k < 24; ++k) {
        const float vx = q[3 + 2 * k], vy = q[4 + 2 * k];
        ok = ok && fabsf(vx) < LIM && fabsf(vy) < LIM;                // false for NaN and infinities too
        xmin = fminf(xmin, vx);
        xmax = fmaxf(xmax, vx);
        ymin = fminf(ymin, vy);
        ymax = fmaxf(ymax, vy);
    }
    int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    if (ok) {
        const float s = (float)stride;
        x0 = (int)(xmin / s);
        x1 = (int)(xmax / s);
        y0 = (int)(ymin / s);
        y1 = (int)(ymax / s);
        if (mode == 1) {                                              // a cell centre inside the polygon lies inside its box: one cell of margin
            x0 -= 1;
            y0 -= 1;
            x1 += 2;
            y1 += 2;
        }
        x0 = min(max(x0, 0), W);
        x1 = min(max(x1, 0), W);
        y0 = min(max(y0, 0), H);
        y1 = min(max(y1, 0), H);
    }
    if (mode == 1 && threadIdx.x < 48) vert[threadIdx.x] = (double)q[3 + threadIdx.x];
    __syncthreads();
    const int w = max(x1 - x0, 0), h = max(y1 - y0, 0);
    const int cells = w * h;                                          // H, W <= 16384: below 2^31
    const float* m = maps + b * H * W;
    const double sd = (double)stride;
    double acc = 0.0;
    int cnt = 0;
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int ci = c / w;
        const int i = y0 + ci, j = x0 + (c - ci * w);
        bool in = true;
        if (mode == 1) in = raster_point_inside(vert, 24, ((double)j + 0.5) * sd, ((double)i + 0.5) * sd);
        if (in) {
            acc += (double)m[(int64_t)i * W + j];
            cnt += 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = acc;
        wcnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s4 = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        const int c4 = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        sum[row] = c4 > 0 ? s4 : 0.0;
        count[row] = c4;
        mean[row] = c4 > 0 ? s4 / (double)c4 : 0.0;
    }
}

template <int G>
void launch_mean(const void* x, int64_t ld, int64_t M, int C, float* out, hipStream_t s) {
    constexpr int RPW = 256 / G;
    const int64_t blocks = (M + RPW - 1) / RPW;
    const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));                 // beyond it the workgroups stride over the rows
    hipLaunchKernelGGL(featmap_mean_kernel<G>, dim3(grid), dim3(256), 0, s, (const uint16_t*)x, ld, M, C / 8, (float)C, out);
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_featmap_mean_bf16(const void* x, int64_t ld, int64_t M, int C, float* out, void* stream) {
    EP24_REQUIRE(M >= 0, EP24_E_ARG, "featmap_mean_bf16: M=%lld", (long long)M);
    EP24_REQUIRE(C >= 8 && C % 8 == 0 && ld >= C && ld % 8 == 0 && (((uintptr_t)x) & 15) == 0, EP24_E_UNSUPPORTED,
                 "featmap_mean_bf16: C=%d ld=%lld x=%p (C and ld multiples of 8, C >= 8, ld >= C, x 16-byte aligned)", C, (long long)ld, x);
    if (M == 0) return EP24_OK;
    EP24_REQUIRE(x && out, EP24_E_ARG, "featmap_mean_bf16: null pointer");
    const int chunks = C / 8;
    if (chunks <= 1) launch_mean<1>(x, ld, M, C, out, S_);
    else if (chunks <= 2) launch_mean<2>(x, ld, M, C, out, S_);
    else if (chunks <= 4) launch_mean<4>(x, ld, M, C, out, S_);
    else if (chunks <= 8) launch_mean<8>(x, ld, M, C, out, S_);
    else if (chunks <= 16) launch_mean<16>(x, ld, M, C, out, S_);
    else if (chunks <= 32) launch_mean<32>(x, ld, M, C, out, S_);
    else launch_mean<64>(x, ld, M, C, out, S_);
    EP24_LAUNCH_CHECK("ep24_featmap_mean_bf16");
    return EP24_OK;
}

extern "C" int ep24_featmap_range(const float* maps, int N, int64_t cells, float* range, void* stream) {
    EP24_REQUIRE(N >= 0 && cells >= 0, EP24_E_ARG, "featmap_range: N=%d cells=%lld", N, (long long)cells);
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(range && (maps || cells == 0), EP24_E_ARG, "featmap_range: null pointer");
    hipLaunchKernelGGL(featmap_range_kernel, dim3((unsigned)N), dim3(256), 0, S_, maps, cells, range);
    EP24_LAUNCH_CHECK("ep24_featmap_range");
    return EP24_OK;
}

extern "C" int ep24_featmap_render(const float* maps, int N, int H, int W, int scale, const float* range, const uint8_t* lut,
                                   const float* base, int alpha, uint8_t* out, void* stream) {
    EP24_REQUIRE(N >= 0 && alpha >= 0 && alpha <= 255, EP24_E_ARG, "featmap_render: N=%d alpha=%d", N, alpha);
    EP24_REQUIRE(scale >= 1 && scale <= EP24_FEATMAP_MAX_SCALE && H >= 1 && W >= 1 && (int64_t)H * scale <= EP24_DRAW_MAX_SIDE &&
                     (int64_t)W * scale <= EP24_DRAW_MAX_SIDE,
                 EP24_E_UNSUPPORTED, "featmap_render: H=%d W=%d scale=%d (scale 1..%d, sides 1..%d)", H, W, scale, EP24_FEATMAP_MAX_SCALE,
                 EP24_DRAW_MAX_SIDE);
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(maps && range && lut && out, EP24_E_ARG, "featmap_render: null pointer");
    const int quads = (W * scale + 3) / 4;
    const int64_t total = (int64_t)N * H * scale * quads;
    EP24_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFLL, EP24_E_UNSUPPORTED, "featmap_render: N=%d: too many pixels for one launch", N);
    hipLaunchKernelGGL(featmap_render_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_, maps, H, W, scale, range, lut, base,
                       alpha, out, quads, total);
    EP24_LAUNCH_CHECK("ep24_featmap_render");
    return EP24_OK;
}

extern "C" int ep24_featmap_response(const float* maps, int B, int H, int W, int stride, const float* labels, int L, int mode,
                                     double* sum, int32_t* count, double* mean, void* stream) {
    EP24_REQUIRE(B >= 0 && L >= 0 && stride >= 1 && (mode == 0 || mode == 1), EP24_E_ARG, "featmap_response: B=%d L=%d stride=%d mode=%d",
                 B, L, stride, mode);
    EP24_REQUIRE(H >= 1 && W >= 1 && H <= EP24_DRAW_MAX_SIDE && W <= EP24_DRAW_MAX_SIDE && (int64_t)B * L <= 0x7FFFFFFFLL,
                 EP24_E_UNSUPPORTED, "featmap_response: H=%d W=%d (1..%d) B*L=%lld", H, W, EP24_DRAW_MAX_SIDE, (long long)B * L);
    if ((int64_t)B * L == 0) return EP24_OK;
    EP24_REQUIRE(maps && labels && sum && count && mean, EP24_E_ARG, "featmap_response: null pointer");
    hipLaunchKernelGGL(featmap_response_kernel, dim3((unsigned)((int64_t)B * L)), dim3(256), 0, S_, maps, H, W, stride, labels, L, mode,
                       sum, count, mean);
    EP24_LAUNCH_CHECK("ep24_featmap_response");
    return EP24_OK;
}
