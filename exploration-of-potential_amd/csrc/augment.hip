// ep24 - training augmentation on the GPU for 24-point labels: mosaic, random affine, mixup, mirror and HSV in two launches per batch.
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
//
// Mixup (MosaicDetection.mixup; the *_mix entry points, the MIX instantiations below): an output image may have a PARTNER, one more
// source of the same batch.  The reference letterboxes it onto an S canvas (padding 114), resizes that canvas by a jitter factor to
// Wj x Hj, mirrors it, pastes it on a zero canvas of at least S_h x S_w, crops an S_h x S_w window at (x_off, y_off) and averages
// the window with the mosaic; its labels move as boxes.  Here, in the frame before the final mirror (xm, y):
//   px = xm + x_off, py = y + y_off;  px >= Wj or py >= Hj: the partner value is 0 (the zero canvas);
//   pxf = flip ? Wj-1-px : px;  u = (pxf+0.5)*(S_w/Wj) - 0.5, v = (py+0.5)*(S_h/Hj) - 0.5: the letterbox canvas, by the same
//   nearest-canvas-pixel rule: -0.5 <= u < rw-0.5 and -0.5 <= v < rh-0.5 is the partner image, sampled ONCE as a tile with padw =
//   padh = 0 is; everything else inside the jittered canvas is 114;
//   out = (a + b) >> 1 on the integer pixel values (a = the mosaic's pixel before HSV, 114 where no tile owns it): the reference's
//   0.5*a + 0.5*b followed by astype(uint8), exactly.  HSV then recolours a pixel iff a tile or the partner image owns it.
// The same deviation from cv2 as above: one sample of the raw source, not resize (letterbox) followed by resize (jitter).
// Labels: the partner is a fifth candidate source behind the four tiles with its own map, canvas X = (v*w)*s -> output
// diag(+-Wj/S_w, Hj/S_h)*(X, Y) + (flip ? Wj - x_off : -x_off, -y_off), and its own region [0,rw] x [0,rh]; same keep rules, same
// re-cast.  An image whose mixup flag is 0 takes exactly the path of the plain instantiation.
#include "common.h"
#include "resize.h"

namespace {

constexpr int TILE_I = 16;      // int64 words per tile descriptor
constexpr int TILE_D = 3;       // doubles per tile: scale_x, scale_y, s
constexpr int PAR_D = 16;       // doubles per output image
constexpr int MIX_I = 16;       // int64 words per mixup descriptor
constexpr int MIX_D = 12;       // doubles per mixup descriptor

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

// one fixed-point bilinear sample (resize.h) of a raw HWC source at the float coordinate (fx, fy)
__device__ __forceinline__ void sample_bgr(const uint8_t* src, int sh, int sw, long ld, float fx, float fy, int& c0, int& c1, int& c2) {
    int x0, x1, ax0, ax1, y0, y1, by0, by1;
    lin_coef_at(fx, sw, x0, x1, ax0, ax1);
    lin_coef_at(fy, sh, y0, y1, by0, by1);
    const uint8_t* r0 = src + (long)y0 * ld;
    const uint8_t* r1 = src + (long)y1 * ld;
    c0 = lin_mix_u8(r0[x0 * 3 + 0], r0[x1 * 3 + 0], r1[x0 * 3 + 0], r1[x1 * 3 + 0], ax0, ax1, by0, by1);
    c1 = lin_mix_u8(r0[x0 * 3 + 1], r0[x1 * 3 + 1], r1[x0 * 3 + 1], r1[x1 * 3 + 1], ax0, ax1, by0, by1);
    c2 = lin_mix_u8(r0[x0 * 3 + 2], r0[x1 * 3 + 2], r1[x0 * 3 + 2], r1[x1 * 3 + 2], ax0, ax1, by0, by1);
}

// MIX = false is ep24_augment_u8; MIX = true adds the partner image of ep24_augment_mix_u8 (mixi / mixd: include/ep24.h)
template <bool MIX>
__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ tiles,
                                                         const double* __restrict__ tscale, const double* __restrict__ params,
                                                         const int* __restrict__ flags, const long long* __restrict__ mixi,
                                                         const double* __restrict__ mixd, float* __restrict__ out, int S_h, int S_w) {
    const int n = blockIdx.y;
    const long long* T = tiles + (long)n * 4 * TILE_I;
    const double* TS = tscale + (long)n * 4 * TILE_D;
    const double* P = params + (long)n * PAR_D;
    const double i00 = P[6], i01 = P[7], i02 = P[8], i10 = P[9], i11 = P[10], i12 = P[11];
    const float dh = (float)P[12], ds = (float)P[13], dv = (float)P[14];
    const bool mirror = flags[2 * n] != 0, hsv = flags[2 * n + 1] != 0;
    // the partner of this image (uniform over the block)
    bool mix = false, mflip = false;
    const uint8_t* msrc = nullptr;
    int msh = 0, msw = 0;
    long mld = 0;
    long long Wj = 0, Hj = 0, xoff = 0, yoff = 0;
    double mrw = 0.0, mrh = 0.0, jx = 0.0, jy = 0.0, msx = 0.0, msy = 0.0;
    if constexpr (MIX) {
        const long long* X = mixi + (long)n * MIX_I;
        const double* XD = mixd + (long)n * MIX_D;
        mix = X[0] != 0;
        if (mix) {
            msrc = images + X[1];
            msh = (int)X[2]; msw = (int)X[3]; mld = X[4];
            mrw = (double)X[5]; mrh = (double)X[6];
            Wj = X[7]; Hj = X[8]; xoff = X[9]; yoff = X[10];
            mflip = X[11] != 0;
            jx = XD[0]; jy = XD[1]; msx = XD[2]; msy = XD[3];
        }
    }
    const int plane = S_h * S_w;
    float* o = out + (long)n * 3 * plane;
    const int quads = plane >> 2;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
        const int i = q << 2;
        const int y = i / S_w, xb = i - y * S_w;
        f32x4 v0, v1, v2;
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
            int a0 = 114, a1 = 114, a2 = 114;                      // padding stays 114
            bool owned = own >= 0;
            if (owned) {
                const long long* d = T + own * TILE_I;
                const float fx = (float)(((u - (double)d[10]) + 0.5) * TS[own * TILE_D] - 0.5);
                const float fy = (float)(((v - (double)d[11]) + 0.5) * TS[own * TILE_D + 1] - 0.5);
                sample_bgr(images + d[0], (int)d[1], (int)d[2], (long)d[3], fx, fy, a0, a1, a2);
            }
            if constexpr (MIX) {
                if (mix) {
                    int b0 = 0, b1 = 0, b2 = 0;                    // outside the jittered canvas: the reference's zero canvas
                    const long long px = (long long)xm + xoff, py = (long long)y + yoff;
                    if (px >= 0 && px < Wj && py >= 0 && py < Hj) {
                        b0 = b1 = b2 = 114;                        // the letterbox padding, resized with the canvas
                        const long long pxf = mflip ? Wj - 1 - px : px;
                        const double pu = ((double)pxf + 0.5) * jx - 0.5;
                        const double pv = ((double)py + 0.5) * jy - 0.5;
                        if (pu >= -0.5 && pu < mrw - 0.5 && pv >= -0.5 && pv < mrh - 0.5) {
                            const float fx = (float)((pu + 0.5) * msx - 0.5);
                            const float fy = (float)((pv + 0.5) * msy - 0.5);
                            sample_bgr(msrc, msh, msw, mld, fx, fy, b0, b1, b2);
                            owned = true;
                        }
                    }
                    a0 = (a0 + b0) >> 1; a1 = (a1 + b1) >> 1; a2 = (a2 + b2) >> 1;
                }
            }
            float c0 = (float)a0, c1 = (float)a1, c2 = (float)a2;
            if (hsv && owned) hsv_shift(c0, c1, c2, dh, ds, dv);   // channel 0 is B (cv2.imread order); padding and black keep their value
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
// MIX = true (ep24_augment_mix_labels): the rows of the mixup partner follow as source 4, with the partner's own diagonal map
// (mixd[5..10]) in place of A, t, A^-1 and [0,rw] x [0,rh] in place of the tile's region.
template <bool MIX>
__global__ __launch_bounds__(256) void augment_labels_kernel(const double* __restrict__ rows, const long long* __restrict__ tiles,
                                                             const double* __restrict__ tscale, const double* __restrict__ params,
                                                             const int* __restrict__ flags, const long long* __restrict__ mixi,
                                                             const double* __restrict__ mixd, const double* __restrict__ rot,
                                                             int S_h, int S_w, double margin, float* __restrict__ out,
                                                             int* __restrict__ out_count, int max_labels) {
    __shared__ double sP[CHUNK][25][2];        // output-space centre (index 0) and vertices
    __shared__ double sC[CHUNK][2];            // canvas-space centre
    __shared__ double sN[CHUNK][24][2];        // re-cast vertices
    __shared__ double sCls[CHUNK];
    __shared__ int sTile[CHUNK], sKeep[CHUNK];
    __shared__ int sCnt[6], sKept;
    const int n = blockIdx.x, tid = threadIdx.x;
    const long long* X = MIX ? mixi + (long)n * MIX_I : nullptr;
    const double* XD = MIX ? mixd + (long)n * MIX_D : nullptr;
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
        if constexpr (MIX) {
            if (X[0] != 0) {
                long long c = X[13] - X[12];
                c = c < 0 ? 0 : (c > max_labels ? max_labels : c);
                acc += (int)c;
            }
        }
        sCnt[5] = acc;
        sKept = 0;
    }
    __syncthreads();
    const int ncand = sCnt[5];
    for (int base = 0; base < ncand; base += CHUNK) {
        // A: polygon and centre of every candidate of the chunk into output space
        if (tid < CHUNK * 25) {
            const int c = tid / 25, j = tid - c * 25, g = base + c;
            if (g < ncand) {
                int t = 0;
                while (t < (MIX ? 4 : 3) && g >= sCnt[t + 1]) ++t;
                const double* row;
                double cx, cy, ox, oy, rx1, ry1, rx2, ry2;         // canvas point, output point, the source's canvas region
                if (MIX && t == 4) {
                    row = rows + (X[12] + (g - sCnt[4])) * 51;
                    cx = (row[1 + 2 * j] * (double)X[3]) * XD[4];
                    cy = (row[2 + 2 * j] * (double)X[2]) * XD[4];
                    ox = XD[5] * cx + XD[7];
                    oy = XD[6] * cy + XD[8];
                    rx1 = 0.0; ry1 = 0.0; rx2 = (double)X[5]; ry2 = (double)X[6];
                } else {
                    const long long* d = T + t * TILE_I;
                    row = rows + (d[12] + (g - sCnt[t])) * 51;
                    const double s = TS[t * TILE_D + 2];
                    cx = (row[1 + 2 * j] * (double)d[2]) * s + (double)d[10];
                    cy = (row[2 + 2 * j] * (double)d[1]) * s + (double)d[11];
                    ox = (a00 * cx + a01 * cy) + t0;
                    oy = (a10 * cx + a11 * cy) + t1;
                    rx1 = (double)d[6]; ry1 = (double)d[7]; rx2 = (double)d[8]; ry2 = (double)d[9];
                }
                if (mirror) ox = W - ox;
                sP[c][j][0] = ox; sP[c][j][1] = oy;
                if (j == 0) {
                    sC[c][0] = cx; sC[c][1] = cy;
                    sTile[c] = t;
                    sCls[c] = row[0];
                    const bool in_out = ox >= margin && ox <= W - margin && oy >= margin && oy <= H - margin;
                    const bool in_tile = cx >= rx1 + margin && cx <= rx2 - margin && cy >= ry1 + margin && cy <= ry2 - margin;
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
                const double mdx = mirror ? -dx : dx;
                double e_tile;
                if (MIX && sTile[c] == 4) {
                    e_tile = box_exit(sC[c][0], sC[c][1], XD[9] * mdx, XD[10] * dy, 0.0, 0.0, (double)X[5], (double)X[6]);
                } else {
                    const long long* d = T + sTile[c] * TILE_I;
                    e_tile = box_exit(sC[c][0], sC[c][1], i00 * mdx + i01 * dy, i10 * mdx + i11 * dy, (double)d[6], (double)d[7],
                                      (double)d[8], (double)d[9]);
                }
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
    hipLaunchKernelGGL(augment_u8_kernel<false>, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)tiles,
                       tile_scales, params, (const int*)flags, (const long long*)nullptr, (const double*)nullptr, out, S_h, S_w);
    EP24_LAUNCH_CHECK("ep24_augment_u8");
    return EP24_OK;
}

extern "C" int ep24_augment_mix_u8(const uint8_t* images, const int64_t* tiles, const double* tile_scales, const double* params,
                                   const int32_t* flags, const int64_t* mix, const double* mix_scales, int n, float* out, int S_h,
                                   int S_w, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(images && tiles && tile_scales && params && flags && mix && mix_scales && out && n > 0 && n <= 65535 && S_h > 0 &&
                     S_w > 0, EP24_E_ARG, "augment_mix_u8: bad arguments");
    EP24_REQUIRE(S_w % 4 == 0 && (uintptr_t)out % 16 == 0, EP24_E_ARG, "augment_mix_u8: the network input width must be a multiple of 4 (it is a multiple of 32)");
    int bx = (S_h * S_w / 4 + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(augment_u8_kernel<true>, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)tiles,
                       tile_scales, params, (const int*)flags, (const long long*)mix, mix_scales, out, S_h, S_w);
    EP24_LAUNCH_CHECK("ep24_augment_mix_u8");
    return EP24_OK;
}

extern "C" int ep24_augment_labels(const double* rows, const int64_t* tiles, const double* tile_scales, const double* params,
                                   const int32_t* flags, const double* rot, int n, int S_h, int S_w, double min_margin, float* out,
                                   int32_t* out_count, int max_labels, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(rows && tiles && tile_scales && params && flags && rot && out && out_count && n > 0 && S_h > 0 && S_w > 0 &&
                     max_labels > 0 && min_margin >= 0.0, EP24_E_ARG, "augment_labels: bad arguments");
    hipLaunchKernelGGL(augment_labels_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, rows, (const long long*)tiles,
                       tile_scales, params, (const int*)flags, (const long long*)nullptr, (const double*)nullptr, rot, S_h, S_w,
                       min_margin, out, (int*)out_count, max_labels);
    EP24_LAUNCH_CHECK("ep24_augment_labels");
    return EP24_OK;
}

extern "C" int ep24_augment_mix_labels(const double* rows, const int64_t* tiles, const double* tile_scales, const double* params,
                                       const int32_t* flags, const int64_t* mix, const double* mix_scales, const double* rot, int n,
                                       int S_h, int S_w, double min_margin, float* out, int32_t* out_count, int max_labels,
                                       void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(rows && tiles && tile_scales && params && flags && mix && mix_scales && rot && out && out_count && n > 0 && S_h > 0 &&
                     S_w > 0 && max_labels > 0 && min_margin >= 0.0, EP24_E_ARG, "augment_mix_labels: bad arguments");
    hipLaunchKernelGGL(augment_labels_kernel<true>, dim3(n), dim3(256), 0, (hipStream_t)stream, rows, (const long long*)tiles,
                       tile_scales, params, (const int*)flags, (const long long*)mix, mix_scales, rot, S_h, S_w, min_margin, out,
                       (int*)out_count, max_labels);
    EP24_LAUNCH_CHECK("ep24_augment_mix_labels");
    return EP24_OK;
}
