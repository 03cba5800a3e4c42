// ep24 - overlay of 24-point detections on a uint8 image (the contract is in include/ep24.h, E3).
//
//   draw24_prepare  one thread per detection row -> one primitive record of EP24_DRAW_REC_WORDS int32 words (every word written)
//   draw24_paint    one 256-thread workgroup per 64 x 16 pixel tile, a thread owns 4 adjacent pixels of one row.  The records are
//                   taken 256 at a time in row order: each thread tests one record's box against the tile, a ballot prefix compacts
//                   the hits into an LDS list (still in row order), then every thread walks the list over its own pixels.
//
// A pure gather: a pixel is read and written by exactly one thread, in place; no scatter, no atomics.  Every decision is an integer
// one (the fill's crossing is the rasteriser's float64 rule on integer vertices: csrc/mask.hip), and a pixel's walk over the list is
// in row order whatever the scheduling, so the image is a bit-exact function of the inputs.
//
// Integer widths: vertices are clamped to [0, W] x [0, H] with H, W <= 16384 and a tested pixel lies on the canvas, so for an edge
// d = Q - P, w = X - P every component is within +-2^14: d.d, w.d and the cross product stay below 2^30 in int32 and only the square of
// the cross product (< 2^60) is formed in int64 - the same values the contract's int64 arithmetic gives.  Centre and text origin can
// lie 2^20 away: their tests compare the differences against the small bounds before anything is squared.
#include "common.h"

namespace {

constexpr int RW = EP24_DRAW_REC_WORDS;
// record words
constexpr int R_SKIP = 0, R_XC = 1, R_YC = 2, R_VERT = 3 /* 24 x (x, y) */, R_COLOR = 51, R_LEN = 52, R_LABEL = 53 /* 6 words */,
              R_BOX = 59 /* x0, y0, x1, y1 inclusive */, R_PAD = 63;
constexpr float LIM = 1048576.0f;                            // 2^20

__global__ __launch_bounds__(256) void draw24_prepare_kernel(const float* __restrict__ det, int n, float ratio, float conf,
                                                             const float* __restrict__ cs, int H, int W,
                                                             const uint8_t* __restrict__ colors, int C,
                                                             const uint8_t* __restrict__ labels, const int32_t* __restrict__ label_len,
                                                             int s, int show_scores, int32_t* __restrict__ rec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* q = det + i * 29;
    int32_t* r = rec + i * RW;
    const float score = q[26] * q[27];
    const float fc = q[28];
    const float cx = q[0] / ratio, cy = q[1] / ratio;
    bool skip = !(score >= conf) || !(fabsf(cx) < LIM) || !(fabsf(cy) < LIM) || !(fc > -1.0f && fc < (float)C);
    float rad[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        rad[k] = q[2 + k] / ratio;
        skip = skip || !(fabsf(rad[k]) < LIM);
    }
    if (skip) {
        r[R_SKIP] = 1;
        for (int k = 1; k < RW; ++k) r[k] = 0;
        r[R_BOX + 2] = -1;                                   // the empty box
        r[R_BOX + 3] = -1;
        return;
    }
    const int cls = (int)fc;
    const int xc = (int)cx, yc = (int)cy;
    int x0 = xc - 4, x1 = xc + 4, y0 = yc - 4, y1 = yc + 4;
    r[R_SKIP] = 0;
    r[R_XC] = xc;
    r[R_YC] = yc;
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const float fr = (float)(int)rad[k];
        const float px = (float)xc + fr * cs[k], py = (float)yc + fr * cs[24 + k];
        const int vx = (int)fminf(fmaxf(px, 0.0f), (float)W), vy = (int)fminf(fmaxf(py, 0.0f), (float)H);
        r[R_VERT + 2 * k] = vx;
        r[R_VERT + 2 * k + 1] = vy;
        x0 = min(x0, vx - 2);
        x1 = max(x1, vx + 2);
        y0 = min(y0, vy - 2);
        y1 = max(y1, vy + 2);
    }
    r[R_COLOR] = (int)colors[3 * cls] | ((int)colors[3 * cls + 1] << 8) | ((int)colors[3 * cls + 2] << 16);
    // label bytes: the class's entry, then " dd" with show_scores; bytes outside 32..126 become '?'
    const int len0 = min(max(label_len[cls], 0), 24);
    const int len = show_scores ? min(len0 + 3, 24) : len0;
    const float s100 = score * 100.0f;
    const int pct = s100 >= 99.0f ? 99 : (s100 > 0.0f ? (int)s100 : 0);
    for (int wd = 0; wd < 6; ++wd) {
        uint32_t word = 0;
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * wd + b;
            int ch = 0;
            if (j < len0) {
                ch = labels[24 * cls + j];
                if (ch < 32 || ch > 126) ch = '?';
            } else if (j < len) {
                ch = j == len0 ? ' ' : (j == len0 + 1 ? '0' + pct / 10 : '0' + pct % 10);
            }
            word |= (uint32_t)ch << (8 * b);
        }
        r[R_LABEL + wd] = (int)word;
    }
    r[R_LEN] = len;
    if (len > 0) {
        const int tx = xc + 3, ty = yc - 3 - 7 * s;
        x0 = min(x0, tx);
        x1 = max(x1, tx + 6 * s * len - 1);
        y0 = min(y0, ty);
        y1 = max(y1, ty + 7 * s - 1);
    }
    r[R_BOX] = x0;
    r[R_BOX + 1] = y0;
    r[R_BOX + 2] = x1;
    r[R_BOX + 3] = y1;
    r[R_PAD] = 0;
}

__device__ __forceinline__ uint32_t blend(uint32_t pix, uint32_t col, int a) {
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t p = (pix >> (8 * c)) & 255u, q = (col >> (8 * c)) & 255u;
        out |= ((p * (uint32_t)(256 - a) + q * (uint32_t)a + 128u) >> 8) << (8 * c);
    }
    return out;
}

// one record over the thread's quad: pixels (px + j, py), j < 4, the ones with bit j of `live` set lie on the canvas
__device__ __forceinline__ void paint_record(const int32_t* __restrict__ r, const uint8_t* __restrict__ font, int px, int py, int live,
                                             int fill_alpha, int s, uint32_t (&pix)[4], bool& touched) {
    const int bx0 = r[R_BOX], by0 = r[R_BOX + 1], bx1 = r[R_BOX + 2], by1 = r[R_BOX + 3];
    if (py < by0 || py > by1 || px + 3 < bx0 || px > bx1) return;         // the box holds everything the row can cover
    const int xc = r[R_XC], yc = r[R_YC];
    bool cov[4], par[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dx = px + j - xc, dy = py - yc;
        cov[j] = abs(dx) <= 4 && abs(dy) <= 4 && dx * dx + dy * dy <= 16;
        par[j] = false;
    }
    const double yd = (double)py;
    int qx = r[R_VERT], qy = r[R_VERT + 1];
    for (int k = 0; k < 24; ++k) {
        const int k1 = k == 23 ? 0 : k + 1;
        const int ax = qx, ay = qy;                                       // P = v_k
        qx = r[R_VERT + 2 * k1];                                          // Q = v_(k + 1)
        qy = r[R_VERT + 2 * k1 + 1];
        const int dx = qx - ax, dy = qy - ay, L2 = dx * dx + dy * dy, wy = py - ay;
        bool counts = false;
        double xcross = 0.0;
        if (fill_alpha > 0) {
            counts = (ay <= py) != (qy <= py);
            if (counts) xcross = (double)ax + ((yd - (double)ay) * (double)dx) / (double)dy;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int wx = px + j - ax;
            const int t = wx * dx + wy * dy;
            bool c;
            if (t <= 0) {
                c = wx * wx + wy * wy <= 1;
            } else if (t >= L2) {
                const int ex = px + j - qx, ey = py - qy;
                c = ex * ex + ey * ey <= 1;
            } else {
                const long long cr = (long long)(dx * wy - dy * wx);
                c = cr * cr <= (long long)L2;
            }
            c = c || wx * wx + wy * wy <= 4;                              // the vertex disc of P
            cov[j] = cov[j] || c;
            if (counts && (double)(px + j) < xcross) par[j] = !par[j];
        }
    }
    const int m = min(max(r[R_LEN], 0), 24);
    const int v = py - (yc - 3 - 7 * s);
    if (m > 0 && v >= 0 && v < 7 * s) {
        const int vr = v / s, tx = xc + 3, cell = 6 * s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = px + j - tx;
            if (u >= 0 && u < cell * m) {
                const int g = u / cell, cu = (u - g * cell) / s;
                if (cu < 5) {
                    int ch = (r[R_LABEL + (g >> 2)] >> (8 * (g & 3))) & 255;
                    if (ch < 32 || ch > 126) ch = '?';                   // prepare wrote printable bytes; never index outside the font
                    if ((font[(ch - 32) * 7 + vr] >> (4 - cu)) & 1) cov[j] = true;
                }
            }
        }
    }
    const uint32_t col = (uint32_t)r[R_COLOR];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((live >> j) & 1)) continue;
        if (cov[j]) {
            pix[j] = col;
            touched = true;
        } else if (par[j]) {
            pix[j] = blend(pix[j], col, fill_alpha);
            touched = true;
        }
    }
}

__global__ __launch_bounds__(256) void draw24_paint_kernel(uint8_t* img, int H, int W, const int32_t* __restrict__ rec, int n,
                                                           const uint8_t* __restrict__ font, int fill_alpha, int s) {
    __shared__ int list[256];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;
    const int tx1 = min(tx0 + 63, W - 1), ty1 = min(ty0 + 15, H - 1);
    const int px = tx0 + ((tid & 15) << 2), py = ty0 + (tid >> 4);
    const int npx = (py < H && px < W) ? min(4, W - px) : 0;
    const int live = (1 << npx) - 1;
    uint8_t* base = img + ((long)py * W + px) * 3;                         // formed for every thread, touched only with npx > 0
    const bool wide = npx == 4 && (((uintptr_t)base) & 3) == 0;            // 12 aligned bytes: three dword accesses
    uint32_t pix[4] = {0u, 0u, 0u, 0u};
    bool loaded = false, touched = false;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int ri = c0 + tid;
        bool hit = false;
        if (ri < n) {
            const int32_t* r = rec + (long)ri * RW;
            hit = r[R_SKIP] == 0 && r[R_BOX] <= tx1 && r[R_BOX + 2] >= tx0 && r[R_BOX + 1] <= ty1 && r[R_BOX + 3] >= ty0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcnt[wv] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = wcnt[w];
            before += w < wv ? c : 0;
            total += c;
        }
        if (hit) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = ri;
        __syncthreads();
        if (total > 0 && npx > 0) {                                        // total is the same in every thread of the workgroup
            if (!loaded) {
                loaded = true;
                if (wide) {
                    const uint32_t* b4 = (const uint32_t*)base;
                    const uint32_t d0 = b4[0], d1 = b4[1], d2 = b4[2];
                    pix[0] = d0 & 0xFFFFFFu;
                    pix[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
                    pix[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
                    pix[3] = d2 >> 8;
                } else {
                    for (int j = 0; j < npx; ++j)
                        pix[j] = (uint32_t)base[3 * j] | ((uint32_t)base[3 * j + 1] << 8) | ((uint32_t)base[3 * j + 2] << 16);
                }
            }
            for (int i = 0; i < total; ++i) {
                const int rj = __builtin_amdgcn_readfirstlane(list[i]);   // one address for the whole wave: a uniform record pointer
                paint_record(rec + (long)rj * RW, font, px, py, live, fill_alpha, s, pix, touched);
            }
        }
        __syncthreads();                                                   // the next chunk rewrites list and wcnt
    }
    if (!touched) return;
    if (wide) {
        uint32_t* b4 = (uint32_t*)base;
        b4[0] = pix[0] | (pix[1] << 24);
        b4[1] = (pix[1] >> 8) | (pix[2] << 16);
        b4[2] = (pix[2] >> 16) | (pix[3] << 8);
    } else {
        for (int j = 0; j < npx; ++j) {
            base[3 * j] = (uint8_t)pix[j];
            base[3 * j + 1] = (uint8_t)(pix[j] >> 8);
            base[3 * j + 2] = (uint8_t)(pix[j] >> 16);
        }
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_draw24_prepare(const float* det, int n, float ratio, float conf, const float* ray_cs, int H, int W,
                                   const uint8_t* colors, int num_classes, const uint8_t* labels, const int32_t* label_len,
                                   int font_scale, int show_scores, int32_t* rec, void* stream) {
    EP24_REQUIRE(n >= 0 && num_classes >= 1 && ratio > 0.0f && ratio < INFINITY && conf == conf, EP24_E_ARG,
                 "draw24_prepare: n=%d num_classes=%d ratio=%g conf=%g", n, num_classes, (double)ratio, (double)conf);
    EP24_REQUIRE(H >= 1 && W >= 1 && H <= EP24_DRAW_MAX_SIDE && W <= EP24_DRAW_MAX_SIDE && font_scale >= 1 &&
                     font_scale <= EP24_DRAW_MAX_FONT_SCALE && num_classes <= (1 << 24),
                 EP24_E_UNSUPPORTED, "draw24_prepare: H=%d W=%d (1..%d) font_scale=%d (1..%d) num_classes=%d", H, W, EP24_DRAW_MAX_SIDE,
                 font_scale, EP24_DRAW_MAX_FONT_SCALE, num_classes);
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(det && ray_cs && colors && labels && label_len && rec, EP24_E_ARG, "draw24_prepare: null pointer");
    hipLaunchKernelGGL(draw24_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S_, det, n, ratio, conf, ray_cs, H, W,
                       colors, num_classes, labels, label_len, font_scale, show_scores ? 1 : 0, rec);
    EP24_LAUNCH_CHECK("ep24_draw24_prepare");
    return EP24_OK;
}

extern "C" int ep24_draw24_paint(uint8_t* image, int H, int W, const int32_t* rec, int n, const uint8_t* font, int fill_alpha,
                                 int font_scale, void* stream) {
    EP24_REQUIRE(n >= 0 && fill_alpha >= 0 && fill_alpha <= 255, EP24_E_ARG, "draw24_paint: n=%d fill_alpha=%d", n, fill_alpha);
    EP24_REQUIRE(H >= 1 && W >= 1 && H <= EP24_DRAW_MAX_SIDE && W <= EP24_DRAW_MAX_SIDE && font_scale >= 1 &&
                     font_scale <= EP24_DRAW_MAX_FONT_SCALE,
                 EP24_E_UNSUPPORTED, "draw24_paint: H=%d W=%d (1..%d) font_scale=%d (1..%d)", H, W, EP24_DRAW_MAX_SIDE, font_scale,
                 EP24_DRAW_MAX_FONT_SCALE);
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(image && rec && font, EP24_E_ARG, "draw24_paint: null pointer");
    hipLaunchKernelGGL(draw24_paint_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 15) / 16)), dim3(256), 0, S_, image, H, W, rec,
                       n, font, fill_alpha, font_scale);
    EP24_LAUNCH_CHECK("ep24_draw24_paint");
    return EP24_OK;
}
