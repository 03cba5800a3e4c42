// ep24 - the arithmetic half of the baseline JPEG decoder ("JPEG decode"): what libjpeg's default decode path computes
// after the Huffman stage, for a whole batch of images of any sizes and samplings in two launches.  The bit-serial Huffman stage is
// csrc/jpeg_host.cpp (libep24jpeg.so, on the host, in the loader processes); its int16 coefficients are what travels over PCIe.
//
//   jpeg_idct_kernel   coefficients x quantisation table -> one uint8 sample plane per component (MCU-padded): jpeg_idct_islow
//                      (CONST_BITS 13, PASS1_BITS 2), columns first (descale 11), then rows (descale 18), + 128, clamp.
//                      8 lanes per block: a lane fetches one 16-byte coefficient row and the 16-byte row of the table, the 8 lanes
//                      transpose through LDS in front of either pass (rows of 9 dwords, blocks 72 dwords apart: every access of a
//                      32-lane group falls on 32 different banks), a lane stores the 8 bytes of one sample row.
//   jpeg_color_kernel  planes -> uint8 HWC: crop, "fancy" triangle upsampling of 2:1 chroma (replication when a chroma row has at
//                      most 2 samples), 16-bit fixed-point YCbCr -> RGB / BGR, clamp.  An image is a flat run of H*W*3 bytes at a
//                      4-byte aligned offset; a lane makes 4 consecutive pixels of it = 3 whole dwords (the last lane of an image
//                      whose pixel count is no multiple of 4 writes bytes).
//
// All integer, all in wrapping unsigned 32-bit with arithmetic shifts of the reinterpreted value: bit-equal to libjpeg for every file
// a conforming encoder writes, defined (if unspecified) for every other coefficient value.  The image index is found by a binary
// search of the lane's item in a cumulative table - no image index sits in a grid dimension.
#include "common.h"

namespace {

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the largest i in [0, n) with tab[i * stride] <= v (tab[0] == 0 <= v)
__device__ __forceinline__ int find_item(const long long* tab, int stride, int n, long long v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[(long)mid * stride] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ u32 descale(u32 v, int n) { return (u32)((int)(v + (1u << (n - 1))) >> n); }

// one 8-point pass of jpeg_idct_islow on x[0..7], in place
__device__ __forceinline__ void idct8(u32* x, int n) {
    u32 z1 = (x[2] + x[6]) * 4433u;
    const u32 t2 = z1 - x[6] * 15137u;
    const u32 t3 = z1 + x[2] * 6270u;
    const u32 t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u32 a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    u32 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u32 z5 = (z3 + z4) * 9633u;
    a0 *= 2446u;
    a1 *= 16819u;
    a2 *= 25172u;
    a3 *= 12299u;
    z1 *= (u32)-7373;
    z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    x[0] = descale(t10 + a3, n);
    x[7] = descale(t10 - a3, n);
    x[1] = descale(t11 + a2, n);
    x[6] = descale(t11 - a2, n);
    x[2] = descale(t12 + a1, n);
    x[5] = descale(t12 - a1, n);
    x[3] = descale(t13 + a0, n);
    x[4] = descale(t13 - a0, n);
}

__device__ __forceinline__ u32 clamp_u8(int v) { return (u32)min(max(v, 0), 255); }

#define JPEG_BLK_LDS 72       // dwords between two blocks in LDS: 8 rows of 9, and 72 = 8 mod 32

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const unsigned short* __restrict__ qt, int nqt,
                                                        const long long* __restrict__ pdesc, int np, long long total,
                                                        uint8_t* __restrict__ planes) {
    __shared__ u32 lds[32 * JPEG_BLK_LDS];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const long long blk = (long long)blockIdx.x * 32 + lb;
    const bool on = blk < total;
    u32* L = lds + lb * JPEG_BLK_LDS;
    u32 x[8];
    long long first = 0;
    int bw = 1;
    if (on) {
        const long long* d = pdesc + 4L * find_item(pdesc, 4, np, blk);
        first = d[0];
        bw = max((int)d[1], 1);
        int qi = (int)d[2];
        if (qi < 0 || qi >= nqt) qi = 0;
        const i16x8 c = *reinterpret_cast<const i16x8*>(coef + blk * 64 + r * 8);
        const u16x8 q = *reinterpret_cast<const u16x8*>(qt + qi * 64 + r * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (u32)(int)c[i] * (u32)q[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) L[r * 9 + i] = x[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = L[k * 9 + r];          // column r
    idct8(x, 11);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) L[k * 9 + r] = x[k];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = L[r * 9 + i];          // row r of the pass-1 result
    idct8(x, 18);
    if (on) {
        u32x2 o;
        o[0] = clamp_u8((int)x[0] + 128) | (clamp_u8((int)x[1] + 128) << 8) | (clamp_u8((int)x[2] + 128) << 16) | (clamp_u8((int)x[3] + 128) << 24);
        o[1] = clamp_u8((int)x[4] + 128) | (clamp_u8((int)x[5] + 128) << 8) | (clamp_u8((int)x[6] + 128) << 16) | (clamp_u8((int)x[7] + 128) << 24);
        const long long local = blk - first;
        const long long by = local / bw, bx = local - by * bw;
        const long long off = first * 64 + ((by * 8 + r) * bw + bx) * 8;
        if (off >= 0 && off + 8 <= total * 64)               // a descriptor that does not tile its plane cannot write outside the buffer
            *reinterpret_cast<u32x2*>(planes + off) = o;
    }
}

// one chroma sample at output pixel (y, x): mode 1 as it is, 2 = h2v1, 3 = h2v2
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ P, int stride, int dw, int dh, int mode, int y, int x) {
    if (mode == 1) return P[(long)y * stride + x];
    const int i = x >> 1, odd = x & 1;
    const int i2 = odd ? min(i + 1, dw - 1) : max(i - 1, 0);
    if (mode == 2) {
        const uint8_t* row = P + (long)y * stride;
        if (dw <= 2) return row[i];
        return (3 * row[i] + row[i2] + 1 + odd) >> 2;
    }
    const int rr = y >> 1;
    const uint8_t* r0 = P + (long)rr * stride;
    if (dw <= 2) return r0[i];
    const int nb = (y & 1) ? min(rr + 1, dh - 1) : max(rr - 1, 0);
    const uint8_t* r1 = P + (long)nb * stride;
    const int cs = 3 * r0[i] + r1[i], cn = 3 * r0[i2] + r1[i2];
    return (3 * cs + cn + 8 - odd) >> 4;
}

// the chroma samples of FOUR pixels (y, x .. x + 3) of one row, modes 2 and 3 with dw > 2: the four pixels sit over chroma columns
// k = x >> 1 .. k + 2 and look one column to either side, so four (clamped) columns are loaded once - 4 or 8 bytes instead of 8 or 16 -
// and the vertical sums of h2v2 are made once per column.  The five values an even / odd / even / odd / even run of pixels starting at
// column k takes are computed; an even x uses the first four, an odd x the last four.
__device__ __forceinline__ void chroma_quad(const uint8_t* __restrict__ P, int stride, int dw, int dh, int mode, int y, int x, int* out4) {
    const int k = x >> 1, e = x & 1;
    const int c0 = max(k - 1, 0), c1 = k, c2 = min(k + 1, dw - 1), c3 = min(k + 2, dw - 1);
    int S0, S1, S2, S3, re, ro, sh;
    if (mode == 2) {
        const uint8_t* row = P + (long)y * stride;
        S0 = row[c0], S1 = row[c1], S2 = row[c2], S3 = row[c3];
        re = 1, ro = 2, sh = 2;
    } else {
        const int rr = y >> 1;
        const int nb = (y & 1) ? min(rr + 1, dh - 1) : max(rr - 1, 0);
        const uint8_t* r0 = P + (long)rr * stride;
        const uint8_t* r1 = P + (long)nb * stride;
        S0 = 3 * r0[c0] + r1[c0], S1 = 3 * r0[c1] + r1[c1], S2 = 3 * r0[c2] + r1[c2], S3 = 3 * r0[c3] + r1[c3];
        re = 8, ro = 7, sh = 4;
    }
    const int v0 = (3 * S1 + S0 + re) >> sh, v1 = (3 * S1 + S2 + ro) >> sh, v2 = (3 * S2 + S1 + re) >> sh, v3 = (3 * S2 + S3 + ro) >> sh,
              v4 = (3 * S3 + S2 + re) >> sh;
    out4[0] = e ? v1 : v0;
    out4[1] = e ? v2 : v1;
    out4[2] = e ? v3 : v2;
    out4[3] = e ? v4 : v3;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, const long long* __restrict__ idesc, int n,
                                                         long long total, uint8_t* __restrict__ out, long long out_bytes, int bgr) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const long long* d = idesc + 12L * find_item(idesc, 12, n, g);
    const long long gl = g - d[0];
    const int H = (int)d[2], W = max((int)d[3], 1), mode = (int)d[4];
    const uint8_t* Yp = planes + d[5];
    const uint8_t* Cb = planes + d[7];
    const uint8_t* Cr = planes + d[8];
    const int ys = (int)d[6], cst = (int)d[9], dw = (int)d[10], dh = (int)d[11];
    const int npix = H * W;
    const int p0 = (int)(gl * 4);
    int y = p0 / W, x = p0 - y * W;
    u32 px[12];
    // four pixels of one row over subsampled chroma: their chroma columns are loaded once (chroma_quad)
    const bool quad = mode >= 2 && dw > 2 && x + 3 < W && p0 + 4 <= npix;
    int cbq[4] = {0, 0, 0, 0}, crq[4] = {0, 0, 0, 0};
    if (quad) {
        chroma_quad(Cb, cst, dw, dh, mode, y, x, cbq);
        chroma_quad(Cr, cst, dw, dh, mode, y, x, crq);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        u32 c0 = 0, c1 = 0, c2 = 0;
        if (p0 + j < npix) {
            const int Y = Yp[(long)y * ys + x];
            if (mode == 0) {
                c0 = c1 = c2 = (u32)Y;
            } else {
                const int cb = (quad ? cbq[j] : chroma_at(Cb, cst, dw, dh, mode, y, x)) - 128;
                const int cr = (quad ? crq[j] : chroma_at(Cr, cst, dw, dh, mode, y, x)) - 128;
                const u32 R = clamp_u8(Y + ((int)((u32)(91881 * cr) + 32768u) >> 16));
                const u32 B = clamp_u8(Y + ((int)((u32)(116130 * cb) + 32768u) >> 16));
                const u32 G = clamp_u8(Y + ((int)((u32)(-22554 * cb - 46802 * cr) + 32768u) >> 16));
                c0 = bgr ? B : R;
                c1 = G;
                c2 = bgr ? R : B;
            }
        }
        px[3 * j] = c0;
        px[3 * j + 1] = c1;
        px[3 * j + 2] = c2;
        if (++x == W) x = 0, ++y;
    }
    const long long off = d[1] + gl * 12;
    const int cnt = min(npix - p0, 4);
    if (cnt <= 0 || off < 0 || off + 3 * cnt > out_bytes) return;       // a descriptor that lies cannot write outside the buffer
    uint8_t* o = out + off;
    if (cnt == 4 && !(off & 3)) {
        u32* o32 = reinterpret_cast<u32*>(o);
        o32[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        o32[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        o32[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * cnt) o[k] = (uint8_t)px[k];
    }
}

}  // namespace

extern "C" int ep24_jpeg_idct(const void* coef, const void* qt, int nqt, const int64_t* plane_desc, int n_planes, int64_t total_blocks,
                              uint8_t* planes, void* stream) {
    EP24_REQUIRE(n_planes >= 0 && total_blocks >= 0, EP24_E_ARG, "jpeg_idct: negative count (%d planes, %lld blocks)", n_planes, (long long)total_blocks);
    if (n_planes == 0 || total_blocks == 0) return EP24_OK;
    EP24_REQUIRE(coef && qt && plane_desc && planes && nqt > 0, EP24_E_ARG, "jpeg_idct: null pointer");
    EP24_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)planes % 8 == 0, EP24_E_ARG,
                 "jpeg_idct: coefficients and tables must be 16-byte aligned, planes 8-byte aligned");
    EP24_REQUIRE(total_blocks <= 32LL * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_idct: %lld blocks are beyond one launch", (long long)total_blocks);
    const long long groups = (total_blocks + 31) / 32;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, (const short*)coef, (const unsigned short*)qt,
                       nqt, (const long long*)plane_desc, n_planes, (long long)total_blocks, planes);
    EP24_LAUNCH_CHECK("ep24_jpeg_idct");
    return EP24_OK;
}

extern "C" int ep24_jpeg_color(const uint8_t* planes, const int64_t* image_desc, int n, int64_t total_groups, uint8_t* out, int64_t out_bytes,
                               int bgr, void* stream) {
    EP24_REQUIRE(n >= 0 && total_groups >= 0 && out_bytes >= 0, EP24_E_ARG, "jpeg_color: negative count");
    if (n == 0 || total_groups == 0) return EP24_OK;
    EP24_REQUIRE(planes && image_desc && out, EP24_E_ARG, "jpeg_color: null pointer");
    EP24_REQUIRE((uintptr_t)out % 4 == 0, EP24_E_ARG, "jpeg_color: the output buffer must be 4-byte aligned");
    EP24_REQUIRE(total_groups <= 256LL * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_color: %lld pixel groups are beyond one launch", (long long)total_groups);
    const long long groups = (total_groups + 255) / 256;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, planes, (const long long*)image_desc, n,
                       (long long)total_groups, out, (long long)out_bytes, bgr);
    EP24_LAUNCH_CHECK("ep24_jpeg_color");
    return EP24_OK;
}
