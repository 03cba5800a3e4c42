// ep24 - the arithmetic half of the baseline JPEG encoder ("JPEG encode"): what libjpeg's default compress path computes in
// front of its Huffman stage, for a whole batch of images of any sizes and samplings in two launches.  The bit-serial Huffman stage
// is csrc/jpeg_host.cpp (libep24jpeg.so, on the host); int16 coefficients are what travels over PCIe.
//
//   jpeg_sample_kernel  uint8 HWC images, read where they lie (address and row stride in the descriptor) -> one uint8 sample plane per
//                       component over the component's REAL block grid: 16-bit fixed-point RGB / BGR -> YCbCr, h2v1 / h2v2 chroma
//                       downsampling with libjpeg's alternating bias, and its edge rules as clamps of the source coordinates (columns
//                       and rows of the image repeat; the DOWNSAMPLED rows repeat down to the block grid).  A lane makes 8 samples of
//                       one plane row: 8 luma samples, or 8 Cb and 8 Cr samples from the same pixels.
//   jpeg_fdct_kernel    planes x quantisation tables -> int16 coefficients over the MCU-padded grid in ep24_jpeg_idct's layout:
//                       jpeg_fdct_islow on samples - 128 (CONST_BITS 13, PASS1_BITS 2: rows first, << 2 / descale 11, then columns,
//                       descale 2 / 15), then sign(t) * ((|t| + 4 qt) / (8 qt)) by a reciprocal (jpeg_quant.h).  jpeg_idct_kernel's shape: 8 lanes per block, a lane
//                       fetches one 8-byte sample row and stores one 16-byte coefficient row, the 8 lanes transpose through LDS in
//                       front of the column pass and behind it (rows of 9 dwords, blocks 72 dwords apart).  The lanes of a dummy block
//                       (MCU padding right of or below the real grid) recompute the block its DC comes from and store that DC alone:
//                       no third launch, no ordering between workgroups.
//
// All integer.  The image and the plane are found by a binary search of the lane's item in a cumulative table - no image index sits
// in a grid dimension.  A store (and a plane read) that a descriptor would send outside its buffer is dropped.
#include "common.h"
#include "jpeg_quant.h"

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

// rgb_ycc_convert: FIX(x) = int(x * 65536 + 0.5)
__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

__device__ __forceinline__ u32 pack4(const int* v) { return (u32)v[0] | ((u32)v[1] << 8) | ((u32)v[2] << 16) | ((u32)v[3] << 24); }

__device__ __forceinline__ void store8(uint8_t* planes, long long bytes, long long off, const int* v) {
    if (off < 0 || off + 8 > bytes || (off & 7)) return;     // a descriptor that lies cannot write outside the buffer
    u32x2 o;
    o[0] = pack4(v);
    o[1] = pack4(v + 4);
    *reinterpret_cast<u32x2*>(planes + off) = o;
}

#define JPEG_ENC_DESC 8       // int64 per row of either descriptor table

// N consecutive pixels (x0 .. x0 + N - 1, clamped to the last column) of one image row as 0x00c2c1c0 each.  A run that lies inside the
// row and starts on a dword is fetched as 3 N / 4 dwords; any other run (the right edge, a view that starts anywhere) byte by byte.
template <int N>
__device__ __forceinline__ void load_pixels(const uint8_t* __restrict__ row, int x0, int W, u32* px) {
    const uint8_t* p = row + 3L * x0;
    if (x0 + N <= W && !(reinterpret_cast<uintptr_t>(p) & 3)) {
        u32 w[3 * N / 4];
#pragma unroll
        for (int i = 0; i < 3 * N / 4; ++i) w[i] = reinterpret_cast<const u32*>(p)[i];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int i = (3 * k) >> 2, sft = (3 * k) & 3;       // sft 2 and 3 straddle two dwords (never the last pixel: 3 N - 3 = 1 mod 4)
            px[k] = (sft < 2 ? w[i] >> (8 * sft) : __builtin_amdgcn_alignbyte(w[i + (sft >= 2 ? 1 : 0)], w[i], sft)) & 0xffffffu;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint8_t* q = row + 3L * min(x0 + k, W - 1);
            px[k] = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16);
        }
    }
}

// 8 chroma samples (Cb into out[0..8), Cr into out[8..16)) from FX x FY pixels each
template <int FX, int FY>
__device__ __forceinline__ void chroma8(const uint8_t* __restrict__ src, long long stride, int H, int W, int pye, int gx, int bgr, int* out) {
    int cb[8], cr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) cb[i] = cr[i] = 0;
#pragma unroll
    for (int j = 0; j < FY; ++j) {
        u32 px[8 * FX];
        load_pixels<8 * FX>(src + (long long)min(pye * FY + j, H - 1) * stride, gx * 8 * FX, W, px);
#pragma unroll
        for (int k = 0; k < 8 * FX; ++k) {
            const int c0 = px[k] & 255, gg = (px[k] >> 8) & 255, c2 = px[k] >> 16;
            const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
            cb[k / FX] += ycc_cb(r, gg, b);
            cr[k / FX] += ycc_cr(r, gg, b);
        }
    }
    // h2v1: bias 0, 1, 0, 1 ... and >> 1; h2v2: bias 1, 2, 1, 2 ... and >> 2, along the output columns (8 gx + i has i's parity)
    constexpr int SH = (FX == 2) + (FY == 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int bias = SH == 0 ? 0 : (SH - 1) + (i & 1);
        out[i] = (cb[i] + bias) >> SH;
        out[8 + i] = (cr[i] + bias) >> SH;
    }
}

__global__ __launch_bounds__(256) void jpeg_sample_kernel(const long long* __restrict__ idesc, int n, long long total,
                                                          uint8_t* __restrict__ planes, long long plane_bytes) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const long long* d = idesc + (long)JPEG_ENC_DESC * find_item(idesc, JPEG_ENC_DESC, n, g);
    const long long gl = g - d[0];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d[1]);
    const long long stride = d[2];
    const int H = max((int)d[3], 1), W = max((int)d[4], 1), mode = (int)d[5] & 255, bgr = (int)(d[5] >> 8) & 1;
    const long long poff = d[6];
    const int fx = mode >= 2 ? 2 : 1, fy = mode == 3 ? 2 : 1;
    const int wby = (W + 7) >> 3, hby = (H + 7) >> 3;
    const int ch = (H + fy - 1) / fy;
    const int wbc = ((W + fx - 1) / fx + 7) >> 3, hbc = (ch + 7) >> 3;
    const long long gy = (long long)hby * 8 * wby;
    int out[16];
    if (gl < gy) {
        const int py = (int)(gl / wby), gx = (int)(gl - (long long)py * wby);
        const uint8_t* row = src + (long long)min(py, H - 1) * stride;      // the last row repeats downward, the last column to the right
        if (mode == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = row[min(gx * 8 + i, W - 1)];
        } else {
            u32 px[8];
            load_pixels<8>(row, gx * 8, W, px);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c0 = px[i] & 255, gg = (px[i] >> 8) & 255, c2 = px[i] >> 16;
                out[i] = ycc_y(bgr ? c2 : c0, gg, bgr ? c0 : c2);
            }
        }
        store8(planes, plane_bytes, poff + ((long long)py * wby + gx) * 8, out);
        return;
    }
    if (mode == 0) return;
    const long long gc = gl - gy;
    if (gc >= (long long)hbc * 8 * wbc) return;
    const int py = (int)(gc / wbc), gx = (int)(gc - (long long)py * wbc);
    const int pye = min(py, ch - 1);                        // the DOWNSAMPLED rows repeat down to the block grid
    if (mode == 3) chroma8<2, 2>(src, stride, H, W, pye, gx, bgr, out);
    else if (mode == 2) chroma8<2, 1>(src, stride, H, W, pye, gx, bgr, out);
    else chroma8<1, 1>(src, stride, H, W, pye, gx, bgr, out);
    const long long ob = poff + 64LL * wby * hby + ((long long)py * wbc + gx) * 8;
    store8(planes, plane_bytes, ob, out);
    store8(planes, plane_bytes, ob + 64LL * wbc * hbc, out + 8);
}

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// one 8-point pass of jpeg_fdct_islow on x[0..7], in place: the row pass (first) scales up by 4, the column pass takes it out again
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* x) {
    const int n = FIRST ? 11 : 15;
    const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
    const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    x[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    x[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    x[2] = descale(z1 + t13 * 6270, n);
    x[6] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    x[7] = descale(a4 + z1 + z3, n);
    x[5] = descale(a5 + z2 + z4, n);
    x[3] = descale(a6 + z2 + z3, n);
    x[1] = descale(a7 + z1 + z4, n);
}

#define JPEG_BLK_LDS 72       // dwords between two blocks in LDS: 8 rows of 9, and 72 = 8 mod 32

__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const uint8_t* __restrict__ planes, long long plane_bytes,
                                                        const unsigned short* __restrict__ qt, int nqt, const long long* __restrict__ pdesc,
                                                        int np, long long total, short* __restrict__ coef) {
    __shared__ int lds[32 * JPEG_BLK_LDS];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const long long blk = (long long)blockIdx.x * 32 + lb;
    const bool on = blk < total;
    int* L = lds + lb * JPEG_BLK_LDS;
    int x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0;
    bool real = false;
    int qi = 0;
    if (on) {
        const long long* d = pdesc + (long)JPEG_ENC_DESC * find_item(pdesc, JPEG_ENC_DESC, np, blk);
        const int bw = max((int)d[1], 1), wb = max((int)d[4], 1), hb = max((int)d[5], 1), hc = max((int)d[6], 1);
        qi = (int)d[2];
        if (qi < 0 || qi >= nqt) qi = 0;
        const long long local = blk - d[0];
        const int by = (int)(local / bw), bx = (int)(local - (long long)by * bw);
        real = by < hb && bx < wb;
        // a dummy block takes the DC of the block to its left; in a dummy block row, that of the last block of the row above in its MCU
        // (itself possibly a dummy).  Followed to its end: the last real row, and the last real column at or left of that block.
        const int sy = min(by, hb - 1);
        const int sx = by < hb ? min(bx, wb - 1) : min(bx / hc * hc + hc - 1, wb - 1);
        const long long off = d[3] + (((long long)sy * 8 + r) * wb + sx) * 8;
        if (off >= 0 && off + 8 <= plane_bytes && !(off & 7)) {
            const u32x2 s = *reinterpret_cast<const u32x2*>(planes + off);
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = (int)((s[i >> 2] >> (8 * (i & 3))) & 255u) - 128;
        }
    }
    fdct8<true>(x);                                         // row r
#pragma unroll
    for (int i = 0; i < 8; ++i) L[r * 9 + i] = x[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = L[k * 9 + r];          // column r of the row pass's result
    fdct8<false>(x);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) L[k * 9 + r] = x[k];
    __syncthreads();
    if (!on) return;
    const u16x8 q = *reinterpret_cast<const u16x8*>(qt + qi * 64 + r * 8);
    i16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int t = L[r * 9 + i];                         // row r of the coefficients: natural order
        // |t| <= 8 * 1 024 * 1.4 here, far inside ep24_quant_div's proven range; the hardware reciprocal is within 1 ulp
        const int v = (int)ep24_quant_div((u32)abs(t) + 4u * q[i], __builtin_amdgcn_rcpf((float)(8u * max((u32)q[i], 1u))));
        const bool keep = real || (r == 0 && i == 0);
        o[i] = (short)(keep ? (t < 0 ? -v : v) : 0);
    }
    *reinterpret_cast<i16x8*>(coef + blk * 64 + r * 8) = o;
}

}  // namespace

extern "C" int ep24_jpeg_sample(const int64_t* image_desc, int n, int64_t total_groups, uint8_t* planes, int64_t plane_bytes, void* stream) {
    EP24_REQUIRE(n >= 0 && total_groups >= 0 && plane_bytes >= 0, EP24_E_ARG, "jpeg_sample: negative count");
    if (n == 0 || total_groups == 0) return EP24_OK;
    EP24_REQUIRE(image_desc && planes, EP24_E_ARG, "jpeg_sample: null pointer");
    EP24_REQUIRE((uintptr_t)planes % 8 == 0 && (uintptr_t)image_desc % 8 == 0, EP24_E_ARG, "jpeg_sample: planes and descriptors must be 8-byte aligned");
    EP24_REQUIRE(total_groups <= 256LL * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_sample: %lld sample groups are beyond one launch", (long long)total_groups);
    const long long groups = (total_groups + 255) / 256;
    hipLaunchKernelGGL(jpeg_sample_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, (const long long*)image_desc, n,
                       (long long)total_groups, planes, (long long)plane_bytes);
    EP24_LAUNCH_CHECK("ep24_jpeg_sample");
    return EP24_OK;
}

extern "C" int ep24_jpeg_fdct(const uint8_t* planes, int64_t plane_bytes, const void* qt, int nqt, const int64_t* plane_desc, int n_planes,
                              int64_t total_blocks, void* coef, void* stream) {
    EP24_REQUIRE(n_planes >= 0 && total_blocks >= 0 && plane_bytes >= 0, EP24_E_ARG, "jpeg_fdct: negative count (%d planes, %lld blocks)", n_planes,
                 (long long)total_blocks);
    if (n_planes == 0 || total_blocks == 0) return EP24_OK;
    EP24_REQUIRE(planes && qt && plane_desc && coef && nqt > 0, EP24_E_ARG, "jpeg_fdct: null pointer");
    EP24_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)planes % 8 == 0 && (uintptr_t)plane_desc % 8 == 0, EP24_E_ARG,
                 "jpeg_fdct: coefficients and tables must be 16-byte aligned, planes and descriptors 8-byte aligned");
    EP24_REQUIRE(total_blocks <= 32LL * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_fdct: %lld blocks are beyond one launch", (long long)total_blocks);
    const long long groups = (total_blocks + 31) / 32;
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, planes, (long long)plane_bytes,
                       (const unsigned short*)qt, nqt, (const long long*)plane_desc, n_planes, (long long)total_blocks, (short*)coef);
    EP24_LAUNCH_CHECK("ep24_jpeg_fdct");
    return EP24_OK;
}
