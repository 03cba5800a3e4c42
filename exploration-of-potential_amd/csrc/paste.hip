// ep24 - copy-paste augmentation for 24-point labels (YOLOv5 / v8 `copy_paste`; Ghiasi et al., "Simple Copy-Paste"): a post-pass of
// two launches over the batch that the augmentation's two launches (csrc/augment.hip) produced, with or without mixup.
//
// Every label is a star-shaped 24-gon around its centre, and that polygon IS the object's mask here: no instance masks are
// loaded.  Image i may paste objects of a PARTNER image j of the same batch through a rigid integer transform, so pixels are
// copied, never resampled:
//   point  (X, Y) -> ((flip ? S_w - X : X) + dx, Y + dy)              (double on the fp32 label, rounded once to fp32)
//   pixel  (x, y) reads (xs, ys): xu = x - dx, xs = flip ? S_w - 1 - xu : xu, ys = y - dy
// with the conventions of ep24_augment_u8 / ep24_augment_labels: pixel x covers [x, x + 1), its centre is x + 0.5, labels mirror
// continuously (S_w - X) and pixels by column (S_w - 1 - x).
// Labels (ep24_paste_labels): the candidates are the partner's rows in order; one is pasted iff its select bit is set, its
// transformed centre is min_margin inside the output, its 24 transformed vertices are inside the closed output rectangle, and it hides
// less than ioa_thr of every row already there - inter(cand, q) / area(q) by poly24.h's exact intersection, over the image's own rows
// and the candidates accepted before it.  Acceptance is sequential per image, so the result does not depend on any scheduling.
// Image (ep24_paste_u8): a pixel whose centre is inside a pasted polygon by the crossing rule of raster_rule.h, and whose source
// pixel exists, is the partner's pixel; every other pixel is the image's own.  No arithmetic on pixel values: bit exact.
#include "common.h"
#include "poly24.h"
#include "raster_rule.h"

namespace {

constexpr int PASTE_I = 8;              // int64 words per paste descriptor
constexpr int ROW = 51;                 // floats per label row
constexpr int MAX_ROWS = 256;           // rows per image the two kernels keep in LDS (48 fp32 each)
constexpr int GROUPS = 10;              // rows a candidate is intersected with at a time: 10 x 24 lanes of 256
constexpr int TW = 64, TH = 16;        // pixels per workgroup of the image kernel: 16 lanes x 4 pixels wide, 16 rows

// One workgroup per image.  sPoly holds the vertices of the rows the image has so far (its own, then the accepted candidates).
__global__ __launch_bounds__(256) void paste_labels_kernel(const float* __restrict__ pre_labels, const int* __restrict__ pre_count,
                                                           const long long* __restrict__ paste, int n, int img0, int S_h, int S_w,
                                                           double margin, double thr, float* __restrict__ out_labels,
                                                           int* __restrict__ out_count, int* __restrict__ paste_range,
                                                           int max_labels) {
    extern __shared__ float sPoly[];                                   // [max_labels][48]
    __shared__ float sCand[ROW];
    __shared__ double sPart[GROUPS][24];
    const int i = img0 + blockIdx.x, tid = threadIdx.x;
    const float* own = pre_labels + (long)i * max_labels * ROW;
    float* o = out_labels + (long)i * max_labels * ROW;
    const int pc = pre_count[i];
    const int E = pc < 0 ? 0 : (pc > max_labels ? max_labels : pc);
    for (int e = tid; e < max_labels * ROW; e += 256) {
        const int r = e / ROW, col = e - r * ROW;
        const float v = r < E ? own[e] : 0.f;
        o[e] = v;
        if (r < E && col >= 3) sPoly[r * 48 + (col - 3)] = v;
    }
    const long long* D = paste + (long)i * PASTE_I;
    const long long j = D[1];
    const bool on = D[0] != 0 && j >= 0 && j < n && pc <= max_labels;
    int cur = E;
    if (on) {
        const bool flip = D[2] != 0;
        const double dx = (double)D[3], dy = (double)D[4];
        const unsigned long long select = (unsigned long long)D[5];
        const double W = (double)S_w, H = (double)S_h;
        const float* cand = pre_labels + (long)j * max_labels * ROW;
        const int pj = pre_count[j];
        const int nc = pj < 0 ? 0 : (pj > max_labels ? max_labels : pj);
        __syncthreads();                                               // sPoly is filled
        for (int k = 0; k < nc && cur < max_labels; ++k) {
            if (k >= 64 || !((select >> k) & 1ull)) continue;          // uniform over the workgroup
            bool bad = false;
            if (tid < 25) {                                            // point 0 is the centre, 1..24 the vertices
                const double x = (double)cand[k * ROW + 1 + 2 * tid], y = (double)cand[k * ROW + 2 + 2 * tid];
                const float fx = (float)((flip ? W - x : x) + dx), fy = (float)(y + dy);
                const double tx = (double)fx, ty = (double)fy;
                if (tid == 0) {
                    bad = !(tx >= margin && tx <= W - margin && ty >= margin && ty <= H - margin);
                    sCand[0] = cand[k * ROW];
                    sCand[1] = fx; sCand[2] = fy;
                } else {
                    bad = !(tx >= 0.0 && tx <= W && ty >= 0.0 && ty <= H);
                    const int v = tid - 1, vo = flip ? (36 - v) % 24 : v;      // the mirrored ray of 15 v degrees is 180 - 15 v
                    sCand[3 + 2 * vo] = fx; sCand[4 + 2 * vo] = fy;
                }
            }
            if (__syncthreads_or(bad)) continue;                       // the barrier also publishes sCand
            // the candidate against GROUPS rows at a time: 24 lanes per row, lane e sums the terms of the candidate's edge e against the
            // row's 24 edges (poly24_edge_accumulate), lane 0 adds the 24 sums in edge order and finishes as poly24_inter does
            bool veto = false;
            for (int base = 0; base < cur; base += GROUPS) {
                const int g = tid / 24, e = tid - g * 24, q = base + g;
                const bool live = g < GROUPS && q < cur;
                double yb = 0.0, sa = 0.0, sb = 0.0;
                int kind = POLY24_APART;
                if (live) {
                    kind = poly24_prepare(sCand + 3, sPoly + q * 48, &yb, &sa, &sb);
                    double S = 0.0;
                    if (kind == POLY24_MEET) poly24_edge_accumulate(sCand + 3, sPoly + q * 48, e, yb, S);
                    sPart[g][e] = S;
                }
                __syncthreads();
                if (live && e == 0 && kind == POLY24_MEET) {           // a NaN row or boxes apart: nothing is hidden (thr > 0)
                    double S = 0.0;
                    for (int f = 0; f < 24; ++f) S += sPart[g][f];
                    double ac, aq;
                    const double inter = poly24_finish(S, sa, sb, &ac, &aq);
                    if (aq > 0.0 && inter / aq >= thr) veto = true;
                }
                __syncthreads();                                       // sPart is free for the next rows
            }
            if (__syncthreads_or(veto)) continue;
            if (tid < ROW) o[cur * ROW + tid] = sCand[tid];
            if (tid < 48) sPoly[cur * 48 + tid] = sCand[3 + tid];
            ++cur;
            __syncthreads();                                           // sPoly grew; sCand is free again
        }
    }
    if (tid == 0) {
        out_count[i] = pc + (cur - E);
        paste_range[2 * i] = E;
        paste_range[2 * i + 1] = cur;
    }
}

// 24 fp32 vertices in LDS seen as the doubles raster_point_inside indexes
struct PromotedVertices {
    const float* p;
    __device__ __forceinline__ double operator[](int k) const { return (double)p[k]; }
};

// One workgroup per TW x TH pixels of one image.  The pasted polygons whose vertex box (widened by one pixel: a rounded crossing
// stays within it) meets the tile go to LDS; a tile that none meets is a plain copy.  VEC: S_w % 4 == 0 and 16-byte aligned
// buffers, four pixels per 16-byte access; otherwise the same code pixel by pixel.
template <bool VEC>
__global__ __launch_bounds__(256) void paste_u8_kernel(const float* __restrict__ pre, const float* __restrict__ labels,
                                                       const int* __restrict__ paste_range, const long long* __restrict__ paste,
                                                       int n, int img0, float* __restrict__ out, int S_h, int S_w, int tiles_x,
                                                       int max_labels) {
    extern __shared__ float sV[];                                      // [max_labels][48] vertices, then
    float* sBox = sV + max_labels * 48;                                // [max_labels][4] x_lo, x_hi, y_lo, y_hi of the vertices
    __shared__ int sN;
    const int i = img0 + blockIdx.y, tid = threadIdx.x;
    const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x - (blockIdx.x / tiles_x) * tiles_x) * TW;
    const long long* D = paste + (long)i * PASTE_I;
    const long long j = D[1];
    const bool on = D[0] != 0 && j >= 0 && j < n;
    const bool flip = D[2] != 0;
    const long long dx = D[3], dy = D[4];
    int lo = paste_range[2 * i], hi = paste_range[2 * i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > max_labels ? max_labels : hi;
    // the image's own pixels first: their loads are in flight while the polygons are sorted out below
    const int y = ty0 + (tid >> 4), xb = tx0 + (tid & 15) * 4;
    const bool active = y < S_h && xb < S_w;
    const long plane = (long)S_h * S_w;
    const float* src = pre + (long)i * 3 * plane;
    const float* par = pre + (long)j * 3 * plane;                      // read only where `on`
    float* dst = out + (long)i * 3 * plane;
    const long at = (long)y * S_w + xb;
    float c[3][4] = {};
    if (VEC && active) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + ch * plane + at);
            c[ch][0] = v[0]; c[ch][1] = v[1]; c[ch][2] = v[2]; c[ch][3] = v[3];
        }
    } else if (active) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int p = 0; p < 4; ++p) c[ch][p] = xb + p < S_w ? src[ch * plane + at + p] : 0.f;
    }
    if (tid == 0) sN = 0;
    __syncthreads();
    if (on) {
        for (int r = lo + tid; r < hi; r += 256) {
            const float* v = labels + ((long)i * max_labels + r) * ROW + 3;
            float xl = INFINITY, xh = -INFINITY, yl = INFINITY, yh = -INFINITY;
            bool finite = true;
            for (int k = 0; k < 24; ++k) {
                xl = fminf(xl, v[2 * k]); xh = fmaxf(xh, v[2 * k]);
                yl = fminf(yl, v[2 * k + 1]); yh = fmaxf(yh, v[2 * k + 1]);
                finite = finite && fabsf(v[2 * k]) < INFINITY && fabsf(v[2 * k + 1]) < INFINITY;
            }
            // pixel centres of the tile: [tx0 + 0.5, tx0 + TW - 0.5] x [ty0 + 0.5, ty0 + TH - 0.5].  A row with a NaN or infinite
            // coordinate (ep24_paste_labels never writes one) pastes nothing: the box argument needs a closed finite polygon.
            if (finite && xh + 1.f >= (float)tx0 && xl - 1.f <= (float)(tx0 + TW) && yh >= (float)ty0 && yl <= (float)(ty0 + TH)) {
                const int s = atomicAdd(&sN, 1);                       // the order does not matter: the pixel test is an OR
                for (int k = 0; k < 48; ++k) sV[s * 48 + k] = v[k];
                sBox[4 * s] = xl; sBox[4 * s + 1] = xh; sBox[4 * s + 2] = yl; sBox[4 * s + 3] = yh;
            }
        }
    }
    __syncthreads();
    const int np = sN;
    if (!active) return;
    if (np > 0) {
        const double py = (double)y + 0.5;
        const long long ys = (long long)y - dy;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int x = xb + p;
            const long long xu = (long long)x - dx, xs = flip ? (long long)S_w - 1 - xu : xu;
            if (x >= S_w || xs < 0 || xs >= S_w || ys < 0 || ys >= S_h) continue;
            const double px = (double)x + 0.5;
            bool in = false;
            for (int s = 0; s < np && !in; ++s) {
                // outside the rows [y_lo, y_hi) no edge counts; beyond the widened x range the crossings to the right are none or all
                if (py < (double)sBox[4 * s + 2] || py >= (double)sBox[4 * s + 3] || px < (double)sBox[4 * s] - 1.0 ||
                    px > (double)sBox[4 * s + 1] + 1.0) continue;
                in = raster_point_inside(PromotedVertices{sV + s * 48}, 24, px, py);
            }
            if (in) {
                const long from = (long)ys * S_w + (long)xs;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch][p] = par[ch * plane + from];
            }
        }
    }
    if constexpr (VEC) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            f32x4 v;
            v[0] = c[ch][0]; v[1] = c[ch][1]; v[2] = c[ch][2]; v[3] = c[ch][3];
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + ch * plane + at));
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (xb + p < S_w) dst[ch * plane + at + p] = c[ch][p];
    }
}

}  // namespace

extern "C" int ep24_paste_labels(const float* pre_labels, const int32_t* pre_count, const int64_t* paste, int n, int S_h, int S_w,
                                 double min_margin, double ioa_thr, float* out_labels, int32_t* out_count, int32_t* paste_range,
                                 int max_labels, void* stream) {
    EP24_REQUIRE(n >= 0, EP24_E_ARG, "paste_labels: negative n");
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(pre_labels && pre_count && paste && out_labels && out_count && paste_range && S_h > 0 && S_w > 0 && min_margin >= 0.0,
                 EP24_E_ARG, "paste_labels: bad arguments");
    EP24_REQUIRE(max_labels > 0 && max_labels <= MAX_ROWS, EP24_E_ARG, "paste_labels: max_labels must be 1 .. %d", MAX_ROWS);
    EP24_REQUIRE(ioa_thr > 0.0, EP24_E_ARG, "paste_labels: ioa_thr must be positive (a share of an object's area)");
    EP24_REQUIRE(out_labels != pre_labels, EP24_E_ARG, "paste_labels: pre_labels is a snapshot; out_labels must be another buffer");
    for (int lo = 0; lo < n; lo += 65535) {
        const int cnt = n - lo < 65535 ? n - lo : 65535;
        hipLaunchKernelGGL(paste_labels_kernel, dim3(cnt), dim3(256), (size_t)max_labels * 48 * sizeof(float), (hipStream_t)stream,
                           pre_labels, (const int*)pre_count, (const long long*)paste, n, lo, S_h, S_w, min_margin, ioa_thr,
                           out_labels, (int*)out_count, (int*)paste_range, max_labels);
        EP24_LAUNCH_CHECK("ep24_paste_labels");
    }
    return EP24_OK;
}

extern "C" int ep24_paste_u8(const float* pre_images, const float* out_labels, const int32_t* paste_range, const int64_t* paste,
                             int n, float* out_images, int S_h, int S_w, int max_labels, void* stream) {
    EP24_REQUIRE(n >= 0, EP24_E_ARG, "paste_u8: negative n");
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(pre_images && out_labels && paste_range && paste && out_images && S_h > 0 && S_w > 0, EP24_E_ARG,
                 "paste_u8: bad arguments");
    EP24_REQUIRE(max_labels > 0 && max_labels <= MAX_ROWS, EP24_E_ARG, "paste_u8: max_labels must be 1 .. %d", MAX_ROWS);
    EP24_REQUIRE(out_images != pre_images, EP24_E_ARG, "paste_u8: pre_images is a snapshot; out_images must be another buffer");
    const int tiles_x = ep24_cdiv(S_w, TW), tiles_y = ep24_cdiv(S_h, TH);
    EP24_REQUIRE((long)tiles_x * tiles_y <= 2147483647L, EP24_E_ARG, "paste_u8: image too large");
    const size_t lds = (size_t)max_labels * 52 * sizeof(float);
    const bool vec = S_w % 4 == 0 && (uintptr_t)pre_images % 16 == 0 && (uintptr_t)out_images % 16 == 0;
    for (int lo = 0; lo < n; lo += 65535) {
        const int cnt = n - lo < 65535 ? n - lo : 65535;
        if (vec)
            hipLaunchKernelGGL(paste_u8_kernel<true>, dim3(tiles_x * tiles_y, cnt), dim3(256), lds, (hipStream_t)stream, pre_images,
                               out_labels, (const int*)paste_range, (const long long*)paste, n, lo, out_images, S_h, S_w, tiles_x,
                               max_labels);
        else
            hipLaunchKernelGGL(paste_u8_kernel<false>, dim3(tiles_x * tiles_y, cnt), dim3(256), lds, (hipStream_t)stream, pre_images,
                               out_labels, (const int*)paste_range, (const long long*)paste, n, lo, out_images, S_h, S_w, tiles_x,
                               max_labels);
        EP24_LAUNCH_CHECK("ep24_paste_u8");
    }
    return EP24_OK;
}
