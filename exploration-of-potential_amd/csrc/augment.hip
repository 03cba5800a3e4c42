// ep24 - training augmentation on the GPU for 24-point labels: mosaic, random affine, mirror and HSV in two launches per batch.
//
// The reference's 24p TrainTransform accepts flip_prob / hsv_prob and ignores them, and its mosaic / random_affine code
// (yolox_24p/data/) handles boxes only: a 24-point label is a centre plus 24 vertices on rays 15 degrees apart, and a rotated,
// sheared or cropped polygon no longer has its vertices on those rays.  Here the image half samples the raw uint8 sources
// straight into the network input (up to four tiles of a mosaic canvas, seen through the inverse affine map), and the label
// half maps every polygon forward and RE-CASTS the 24 rays from the new centre through it.
//
// Conventions:
//   - a tile is one source image, resized by s = min(S_h/h, S_w/w) as preproc does and placed on the canvas at [lx1,lx2) x [ly1,ly2);
//     padw / padh is where the resized image's (0,0) lands on the canvas (negative when the tile is cropped on that side);
//   - canvas pixel i covers [i - 0.5, i + 0.5): an output pixel belongs to the tile whose region holds its NEAREST canvas pixel;
//   - everything that decides a pixel is double or integer, so with HSV off the image is a bit-exact function of its inputs;
//   - labels: canvas X = (v*w)*s + padw, output c' = A*c + t, mirrored x -> S_w - x (continuous, the reference _mirror's
//     width - x), while the image mirrors pixel columns x -> S_w - 1 - x.
// Deviations from cv2: warpAffine interpolates the already resized uint8 mosaic a second time in 5-bit fixed point; here every
// output pixel is ONE fixed-point bilinear sample (resize.h) of its source.  cvtColor rounds HSV to uint8 before the gains are
// added and BGR to uint8 afterwards; here the HSV triple stays in fp32 and the BGR result is written unrounded.
#include "common.h"
#include "resize.h"

namespace {

constexpr int TILE_I = 16;      // int64 words per tile descriptor
constexpr int TILE_D = 3;       // doubles per tile: scale_x, scale_y, s
constexpr int PAR_D = 16;       // doubles per output image

// BGR (0..255) -> HSV (H in [0,180), S and V in [0,255]) -> gains -> BGR, all fp32 and unrounded
__device__ __forceinline__ void hsv_shift(float& b, float& g, float& r, float dh, float ds, float dv) {
    const float v = fmaxf(fmaxf(b, g), r), mn = fminf(fminf(b, g), r);
    const float diff = v - mn;
    const float s = v > 0.f ? (diff * 255.f) / v : 0.f;
    float h = 0.f;
    if (diff > 0.f) {
        if (v == r) h = (60.f * (g - b)) / diff;
        else if (v == g) h = 120.f + (60.f * (b - r)) / diff;
        else h = 240.f + (60.f * (r - g)) / diff;
    }
    if (h < 0.f) h += 360.f;
    float H = h * 0.5f + dh;
    H = H - 180.f * floorf(H / 180.f);
    const float S = fminf(fmaxf(s + ds, 0.f), 255.f);
    const float V = fminf(fmaxf(v + dv, 0.f), 255.f);
    const float hh = H / 30.f;
    int i = (int)floorf(hh);
    i = i > 5 ? 5 : (i < 0 ? 0 : i);
    const float f = hh - (float)i;
    const float sn = S / 255.f;
    const float p = V * (1.f - sn), q = V * (1.f - sn * f), t = V * (1.f - sn * (1.f - f));
    switch (i) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ tiles,
                                                         const double* __restrict__ tscale, const double* __restrict__ params,
                                                         const int* __restrict__ flags, float* __restrict__ out, int S_h, int S_w) {
    const int n = blockIdx.y;
    const long long* T = tiles + (long)n * 4 * TILE_I;
    const double* TS = tscale + (long)n * 4 * TILE_D;
    const double* P = params + (long)n * PAR_D;
    const double i00 = P[6], i01 = P[7], i02 = P[8], i10 = P[9], i11 = P[10], i12 = P[11];
    const float dh = (float)P[12], ds = (float)P[13], dv = (float)P[14];
    const bool mirror = flags[2 * n] != 0, hsv = flags[2 * n + 1] != 0;
    const int plane = S_h * S_w;
    float* o = out + (long)n * 3 * plane;
    const int quads = plane >> 2;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
        const int i = q << 2;
        const int y = i / S_w, xb = i - y * S_w;
        f32x4 v0 = {114.f, 114.f, 114.f, 114.f}, v1 = v0, v2 = v0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = xb + j;
            const int xm = mirror ? S_w - 1 - x : x;
            const double u = (i00 * (double)xm + i01 * (double)y) + i02;
            const double v = (i10 * (double)xm + i11 * (double)y) + i12;
            int own = -1;
#pragma unroll
            for (int t = 3; t >= 0; --t) {                         // the FIRST owning tile wins (regions are disjoint anyway)
                const long long* d = T + t * TILE_I;
                if (u >= (double)d[6] - 0.5 && u < (double)d[8] - 0.5 && v >= (double)d[7] - 0.5 && v < (double)d[9] - 0.5) own = t;
            }
            if (own < 0) continue;
            const long long* d = T + own * TILE_I;
            const uint8_t* src = images + d[0];
            const int sh = (int)d[1], sw = (int)d[2];
            const long ld = d[3];
            const float fx = (float)(((u - (double)d[10]) + 0.5) * TS[own * TILE_D] - 0.5);
            const float fy = (float)(((v - (double)d[11]) + 0.5) * TS[own * TILE_D + 1] - 0.5);
            int x0, x1, ax0, ax1, y0, y1, by0, by1;
            lin_coef_at(fx, sw, x0, x1, ax0, ax1);
            lin_coef_at(fy, sh, y0, y1, by0, by1);
            const uint8_t* r0 = src + (long)y0 * ld;
            const uint8_t* r1 = src + (long)y1 * ld;
            float c0 = (float)lin_mix_u8(r0[x0 * 3 + 0], r0[x1 * 3 + 0], r1[x0 * 3 + 0], r1[x1 * 3 + 0], ax0, ax1, by0, by1);
            float c1 = (float)lin_mix_u8(r0[x0 * 3 + 1], r0[x1 * 3 + 1], r1[x0 * 3 + 1], r1[x1 * 3 + 1], ax0, ax1, by0, by1);
            float c2 = (float)lin_mix_u8(r0[x0 * 3 + 2], r0[x1 * 3 + 2], r1[x0 * 3 + 2], r1[x1 * 3 + 2], ax0, ax1, by0, by1);
            if (hsv) hsv_shift(c0, c1, c2, dh, ds, dv);            // channel 0 is B (cv2.imread order); padding stays 114
            v0[j] = c0; v1[j] = c1; v2[j] = c2;
        }
        __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(o + i));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(o + plane + i));
        __builtin_nontemporal_store(v2, reinterpret_cast<f32x4*>(o + 2 * plane + i));
    }
}

constexpr int CHUNK = 10;       // candidates per pass: 10 x 24 (object, ray) pairs on 256 threads

__device__ __forceinline__ double box_exit(double x, double y, double dx, double dy, double x1, double y1, double x2, double y2) {
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    const double tx = dx > 0.0 ? (x2 - x) / dx : (dx < 0.0 ? (x1 - x) / dx : inf);
    const double ty = dy > 0.0 ? (y2 - y) / dy : (dy < 0.0 ? (y1 - y) / dy : inf);
    return tx < ty ? tx : ty;
}

// One workgroup per output image.  Candidates are the label rows of tile 0, then tile 1, ... (at most max_labels per tile); they are
// processed CHUNK at a time and the survivors are appended in that order, so the output does not depend on any scheduling.
__global__ __launch_bounds__(256) void augment_labels_kernel(const double* __restrict__ rows, const long long* __restrict__ tiles,
                                                             const double* __restrict__ tscale, const double* __restrict__ params,
                                                             const int* __restrict__ flags, const double* __restrict__ rot,
                                                             int S_h, int S_w, double margin, float* __restrict__ out,
                                                             int* __restrict__ out_count, int max_labels) {
    __shared__ double sP[CHUNK][25][2];        // output-space centre (index 0) and vertices
    __shared__ double sC[CHUNK][2];            // canvas-space centre
    __shared__ double sN[CHUNK][24][2];        // re-cast vertices
    __shared__ double sCls[CHUNK];
    __shared__ int sTile[CHUNK], sKeep[CHUNK];
    __shared__ int sCnt[5], sKept;
    const int n = blockIdx.x, tid = threadIdx.x;
    const long long* T = tiles + (long)n * 4 * TILE_I;
    const double* TS = tscale + (long)n * 4 * TILE_D;
    const double* P = params + (long)n * PAR_D;
    const double a00 = P[0], a01 = P[1], t0 = P[2], a10 = P[3], a11 = P[4], t1 = P[5];
    const double i00 = P[6], i01 = P[7], i10 = P[9], i11 = P[10];
    const bool mirror = flags[2 * n] != 0;
    const double W = (double)S_w, H = (double)S_h;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    float* o = out + (long)n * max_labels * 51;
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < 4; ++t) {
            sCnt[t] = acc;
            long long c = T[t * TILE_I + 13] - T[t * TILE_I + 12];
            c = c < 0 ? 0 : (c > max_labels ? max_labels : c);
            acc += (int)c;
        }
        sCnt[4] = acc;
        sKept = 0;
    }
    __syncthreads();
    const int ncand = sCnt[4];
    for (int base = 0; base < ncand; base += CHUNK) {
        // A: polygon and centre of every candidate of the chunk into output space
        if (tid < CHUNK * 25) {
            const int c = tid / 25, j = tid - c * 25, g = base + c;
            if (g < ncand) {
                int t = 0;
                while (t < 3 && g >= sCnt[t + 1]) ++t;
                const long long* d = T + t * TILE_I;
                const double* row = rows + (d[12] + (g - sCnt[t])) * 51;
                const double s = TS[t * TILE_D + 2];
                const double X = (row[1 + 2 * j] * (double)d[2]) * s + (double)d[10];
                const double Y = (row[2 + 2 * j] * (double)d[1]) * s + (double)d[11];
                double ox = (a00 * X + a01 * Y) + t0;
                const double oy = (a10 * X + a11 * Y) + t1;
                if (mirror) ox = W - ox;
                sP[c][j][0] = ox; sP[c][j][1] = oy;
                if (j == 0) {
                    sC[c][0] = X; sC[c][1] = Y;
                    sTile[c] = t;
                    sCls[c] = row[0];
                    const bool in_out = ox >= margin && ox <= W - margin && oy >= margin && oy <= H - margin;
                    const bool in_tile = X >= (double)d[6] + margin && X <= (double)d[8] - margin &&
                                         Y >= (double)d[7] + margin && Y <= (double)d[9] - margin;
                    sKeep[c] = in_out && in_tile;
                }
            }
        }
        __syncthreads();
        // B: ray k of candidate c against the 24 edges, the output rectangle and the tile's region
        if (tid < CHUNK * 24) {
            const int c = tid / 24, k = tid - c * 24;
            if (base + c < ncand && sKeep[c]) {
                const double dx = rot[2 * k], dy = rot[2 * k + 1];
                const double cx = sP[c][0][0], cy = sP[c][0][1];
                double best = inf;
                double px = sP[c][1][0], py = sP[c][1][1];
                double sp = dx * (py - cy) - dy * (px - cx);
                for (int j = 0; j < 24; ++j) {
                    const int jn = j == 23 ? 1 : j + 2;
                    const double qx = sP[c][jn][0], qy = sP[c][jn][1];
                    const double sq = dx * (qy - cy) - dy * (qx - cx);
                    // the edge meets the ray's line iff its ends are on opposite sides of it (ends included: u in [0,1] closed).  The side
                    // of a vertex is ONE number shared by both of its edges, so a ray through a vertex cannot fall between them.
                    if ((sp <= 0.0 && sq >= 0.0) || (sp >= 0.0 && sq <= 0.0)) {
                        if (sp == sq) {                            // both ends on the line
                            const double tp = dx * (px - cx) + dy * (py - cy), tq = dx * (qx - cx) + dy * (qy - cy);
                            if (tp >= 0.0 && tp < best) best = tp;
                            if (tq >= 0.0 && tq < best) best = tq;
                        } else {
                            const double u = sp / (sp - sq);
                            const double ix = px + u * (qx - px), iy = py + u * (qy - py);
                            const double t = dx * (ix - cx) + dy * (iy - cy);
                            if (t >= 0.0 && t < best) best = t;
                        }
                    }
                    px = qx; py = qy; sp = sq;
                }
                const double e_out = box_exit(cx, cy, dx, dy, 0.0, 0.0, W, H);
                if (e_out < best) best = e_out;
                const long long* d = T + sTile[c] * TILE_I;
                const double mdx = mirror ? -dx : dx;
                const double e_tile = box_exit(sC[c][0], sC[c][1], i00 * mdx + i01 * dy, i10 * mdx + i11 * dy, (double)d[6], (double)d[7],
                                               (double)d[8], (double)d[9]);
                if (e_tile < best) best = e_tile;
                sN[c][k][0] = cx + best * dx;
                sN[c][k][1] = cy + best * dy;
            }
        }
        __syncthreads();
        // C: the reference TrainTransform's mask_b filter, min(width, height) > 1 of the new vertices
        if (tid < CHUNK && base + tid < ncand && sKeep[tid]) {
            double x1 = inf, y1 = inf, x2 = -inf, y2 = -inf;
            for (int k = 0; k < 24; ++k) {
                x1 = fmin(x1, sN[tid][k][0]); x2 = fmax(x2, sN[tid][k][0]);
                y1 = fmin(y1, sN[tid][k][1]); y2 = fmax(y2, sN[tid][k][1]);
            }
            sKeep[tid] = fmin(x2 - x1, y2 - y1) > 1.0;
        }
        __syncthreads();
        // D: append the survivors in candidate order
        const int kept0 = sKept;
        const int in_chunk = min(CHUNK, ncand - base);
        for (int e = tid; e < in_chunk * 51; e += 256) {
            const int c = e / 51, col = e - c * 51;
            if (!sKeep[c]) continue;
            int slot = kept0;
            for (int b = 0; b < c; ++b) slot += sKeep[b];
            if (slot >= max_labels) continue;
            double v;
            if (col == 0) v = sCls[c];
            else if (col < 3) v = sP[c][0][col - 1];
            else v = sN[c][(col - 3) >> 1][(col - 3) & 1];
            o[slot * 51 + col] = (float)v;
        }
        __syncthreads();
        if (tid == 0) {
            int k = kept0;
            for (int b = 0; b < in_chunk; ++b) k += sKeep[b];
            sKept = k;
        }
        __syncthreads();
    }
    const int kept = sKept;
    for (int e = min(kept, max_labels) * 51 + tid; e < max_labels * 51; e += 256) o[e] = 0.f;
    if (tid == 0) out_count[n] = kept;
}

}  // namespace

extern "C" int ep24_augment_u8(const uint8_t* images, const int64_t* tiles, const double* tile_scales, const double* params,
                               const int32_t* flags, int n, float* out, int S_h, int S_w, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(images && tiles && tile_scales && params && flags && out && n > 0 && n <= 65535 && S_h > 0 && S_w > 0, EP24_E_ARG,
                 "augment_u8: bad arguments");
    EP24_REQUIRE(S_w % 4 == 0 && (uintptr_t)out % 16 == 0, EP24_E_ARG, "augment_u8: the network input width must be a multiple of 4 (it is a multiple of 32)");
    int bx = (S_h * S_w / 4 + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(augment_u8_kernel, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)tiles, tile_scales,
                       params, (const int*)flags, out, S_h, S_w);
    EP24_LAUNCH_CHECK("ep24_augment_u8");
    return EP24_OK;
}

extern "C" int ep24_augment_labels(const double* rows, const int64_t* tiles, const double* tile_scales, const double* params,
                                   const int32_t* flags, const double* rot, int n, int S_h, int S_w, double min_margin, float* out,
                                   int32_t* out_count, int max_labels, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(rows && tiles && tile_scales && params && flags && rot && out && out_count && n > 0 && S_h > 0 && S_w > 0 &&
                     max_labels > 0 && min_margin >= 0.0, EP24_E_ARG, "augment_labels: bad arguments");
    hipLaunchKernelGGL(augment_labels_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, rows, (const long long*)tiles, tile_scales,
                       params, (const int*)flags, rot, S_h, S_w, min_margin, out, (int*)out_count, max_labels);
    EP24_LAUNCH_CHECK("ep24_augment_labels");
    return EP24_OK;
}
