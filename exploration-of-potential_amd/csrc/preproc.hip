// ep24 - input pipeline on the GPU: preproc + TrainTransform of the reference
// (yolox_24p/datasets/data_augment.py:109-174) for a whole batch in two launches.
//
// The reference resizes every image on a CPU worker (cv2.resize INTER_LINEAR to (int(w*r), int(h*r)), r = min(S/h, S/w)),
// pastes it top-left into a 114-filled canvas, transposes to CHW, converts to fp32 and ships 4.9 MB per 640x640 image over
// PCIe.  Here the raw uint8 HWC images travel (0.9 MB for 480x640) and one thread per output pixel does the rest: the
// four source texels of the fixed-point bilinear sample (resize.h), or 114 outside the resized area, written to the three
// fp32 planes of the network input (four pixels of a row per thread, 16-byte streaming stores).  HBM bound: 3 bytes read (L2 serves the neighbours) and 12 written per output pixel.
// Labels: (v * width) * r for x columns, (v * height) * r for y columns in double, rounded to fp32, zero-padded to 50 rows.
//
// Multiscale training (the reference's Exp.preprocess, exp/yolox_base.py:109-118: F.interpolate(bilinear, align_corners=False) of the
// finished fp32 batch + the label columns times tsize / input_size) is the second pair of kernels here: resize_bilinear_kernel and
// scale_labels_kernel.  A streaming kernel (98 MB in, up to 154 MB out at batch 20, 640 -> 800): a lane owns ONE output pixel,
// computes its source indices and weights once - in double, as the other kernels of this file do - and walks planes (blockIdx.y,
// strided): two 8-byte loads and one store per plane, both contiguous across the wave.  The blend is fp32, every operation rounded on
// its own (DESIGN.md section 7 states the rule and the layouts that were measured; tests/resize_oracle.py restates the rule in numpy).
#include "common.h"
#include "resize.h"

namespace {

__global__ __launch_bounds__(256) void preproc_u8_kernel(const uint8_t* images, const long long* desc, const double* scales,
                                                         float* out, int S_h, int S_w) {
    const int n = blockIdx.y;
    const long long* d = desc + (long)n * 6;
    const uint8_t* src = images + d[0];
    const int sh = (int)d[1], sw = (int)d[2], rh = (int)d[4], rw = (int)d[5];
    const long ld = d[3];
    const double scale_x = scales[2 * n], scale_y = scales[2 * n + 1];
    const int plane = S_h * S_w;
    float* o = out + (long)n * 3 * plane;
    // four consecutive pixels of a row per thread: three 16-byte stores (S_w % 4 == 0, checked by the launcher)
    const int quads = plane >> 2;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
        const int i = q << 2;
        const int y = i / S_w, xb = i - y * S_w;
        f32x4 v0 = {114.f, 114.f, 114.f, 114.f}, v1 = v0, v2 = v0;
        if (y < rh && xb < rw) {
            int y0, y1, by0, by1;
            lin_coef(y, scale_y, sh, y0, y1, by0, by1);
            const uint8_t* r0 = src + (long)y0 * ld;
            const uint8_t* r1 = src + (long)y1 * ld;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = xb + j;
                if (x < rw) {
                    int x0, x1, ax0, ax1;
                    lin_coef(x, scale_x, sw, x0, x1, ax0, ax1);
                    v0[j] = (float)lin_mix_u8(r0[x0 * 3 + 0], r0[x1 * 3 + 0], r1[x0 * 3 + 0], r1[x1 * 3 + 0], ax0, ax1, by0, by1);
                    v1[j] = (float)lin_mix_u8(r0[x0 * 3 + 1], r0[x1 * 3 + 1], r1[x0 * 3 + 1], r1[x1 * 3 + 1], ax0, ax1, by0, by1);
                    v2[j] = (float)lin_mix_u8(r0[x0 * 3 + 2], r0[x1 * 3 + 2], r1[x0 * 3 + 2], r1[x1 * 3 + 2], ax0, ax1, by0, by1);
                }
            }
        }
        __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(o + i));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(o + plane + i));
        __builtin_nontemporal_store(v2, reinterpret_cast<f32x4*>(o + 2 * plane + i));
    }
}

__global__ __launch_bounds__(256) void preproc_labels_kernel(const double* rows, const long long* row_off, const double* whr,
                                                             float* out, int max_labels) {
    const int n = blockIdx.x;
    const long lo = row_off[n];
    const int cnt = (int)min((long long)max_labels, row_off[n + 1] - lo);
    const double w = whr[3 * n], h = whr[3 * n + 1], r = whr[3 * n + 2];
    float* o = out + (long)n * max_labels * 51;
    for (int i = threadIdx.x; i < max_labels * 51; i += 256) {
        const int j = i / 51, c = i - j * 51;
        float v = 0.f;
        if (j < cnt) {
            const double t = rows[(lo + j) * 51 + c];
            v = c == 0 ? (float)t : (float)((t * ((c & 1) ? w : h)) * r);     // columns 1,3,5.. are x, 2,4,6.. are y
        }
        o[i] = v;
    }
}

// one axis of the rule: src = max(s * (d + 0.5) - 0.5, 0), i0 = min((int)src, n_in - 1), i1 = min(i0 + 1, n_in - 1), w1 = (float)(src - i0)
__device__ __forceinline__ void bilinear_axis(int d, double s, int n_in, int& i0, int& i1, float& w0, float& w1) {
    const double src = fmax(s * ((double)d + 0.5) - 0.5, 0.0);
    i0 = min((int)src, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    w1 = (float)(src - (double)i0);
    w0 = 1.0f - w1;
}

// PAIR (sw >= 2): the two taps of a row come from ONE 8-byte load of the window [xb, xb + 1], xb = min(x0, sw - 2) - it holds x0 and x1
// also at the right edge, where x1 == x0 == sw - 1.  Half the load instructions: 30.0 against 33.4 us at 640 -> 480, batch 20.
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef f32x2 __attribute__((aligned(4))) f32x2_u;          // a source window starts on any float
template <bool PAIR>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ src, int n, int sh, int sw, float* __restrict__ dst,
                                                              int dh, int dw, double scale_y, double scale_x, int items) {
    const long splane = (long)sh * sw;
    for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
        const int y = it / dw, x = it - y * dw;
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        bilinear_axis(y, scale_y, sh, y0, y1, wy0, wy1);
        bilinear_axis(x, scale_x, sw, x0, x1, wx0, wx1);
        const int r0 = y0 * sw, r1 = y1 * sw;              // < sh * sw <= INT_MAX (checked by the launcher)
        const int xb = min(x0, sw - 2);
        const bool hi0 = x0 != xb, hi1 = x1 != xb;
        for (int p = blockIdx.y; p < n; p += gridDim.y) {
            const float* s0 = src + p * splane + r0;
            const float* s1 = src + p * splane + r1;
            float a, b, c, d;
            if (PAIR) {
                const f32x2 t = *reinterpret_cast<const f32x2_u*>(s0 + xb), u = *reinterpret_cast<const f32x2_u*>(s1 + xb);
                a = hi0 ? t[1] : t[0];
                b = hi1 ? t[1] : t[0];
                c = hi0 ? u[1] : u[0];
                d = hi1 ? u[1] : u[0];
            } else {
                a = s0[x0], b = s0[x1], c = s1[x0], d = s1[x1];
            }
            const float top = a * wx0 + b * wx1;
            const float bot = c * wx0 + d * wx1;
            dst[(long)p * items + it] = top * wy0 + bot * wy1;
        }
    }
}

__global__ __launch_bounds__(256) void scale_labels_kernel(const float* in, float* out, long total, float scale_x, float scale_y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % 51);
        const float v = in[i];
        out[i] = c == 0 ? v : ((c & 1) ? v * scale_x : v * scale_y);      // columns 1,3,5.. are x, 2,4,6.. are y
    }
}

}  // namespace

extern "C" int ep24_resize_bilinear_f32(const float* src, int n, int sh, int sw, float* dst, int dh, int dw, void* stream) {
    EP24_REQUIRE(src && dst, EP24_E_ARG, "resize_bilinear_f32: null pointer");
    EP24_REQUIRE(n > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0, EP24_E_ARG, "resize_bilinear_f32: sizes must be positive (n %d, %d x %d -> %d x %d)",
                 n, sh, sw, dh, dw);
    // a plane is indexed with int (planes with long): source and destination planes below 2^31 elements, the grid stride included
    EP24_REQUIRE((long)sh * sw <= 0x7fffffffL && (long)dh * dw <= 0x7fffffffL - 2048L * 256, EP24_E_ARG,
                 "resize_bilinear_f32: a plane of %d x %d -> %d x %d is beyond the kernel's 31-bit plane index", sh, sw, dh, dw);
    if (sh == dh && sw == dw) {                            // the rule is the identity here: a copy
        if (src != dst) {
            hipError_t e = hipMemcpyAsync(dst, src, (size_t)n * sh * sw * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
            EP24_REQUIRE(e == hipSuccess, EP24_E_LAUNCH, "resize_bilinear_f32: copy failed: %s", hipGetErrorString(e));
        }
        return EP24_OK;
    }
    const int items = dh * dw;
    // grid sized to the chip with a grid stride: x over the pixels of a plane (at most 2048 workgroups), y over the planes, ~8192
    // workgroups in all - a thread's coordinates serve n / grid.y planes
    int bx = ep24_cdiv(items, 256);
    if (bx > 2048) bx = 2048;
    int by = 8192 / bx;
    if (by > n) by = n;
    if (by < 1) by = 1;
    const double scale_y = (double)sh / (double)dh, scale_x = (double)sw / (double)dw;
    if (sw >= 2)
        hipLaunchKernelGGL(resize_bilinear_kernel<true>, dim3(bx, by), dim3(256), 0, (hipStream_t)stream, src, n, sh, sw, dst, dh, dw, scale_y,
                           scale_x, items);
    else
        hipLaunchKernelGGL(resize_bilinear_kernel<false>, dim3(bx, by), dim3(256), 0, (hipStream_t)stream, src, n, sh, sw, dst, dh, dw, scale_y,
                           scale_x, items);
    EP24_LAUNCH_CHECK("ep24_resize_bilinear_f32");
    return EP24_OK;
}

extern "C" int ep24_scale_labels(const float* in, float* out, int64_t rows, float scale_x, float scale_y, void* stream) {
    EP24_REQUIRE(in && out, EP24_E_ARG, "scale_labels: null pointer");
    EP24_REQUIRE(rows > 0 && rows <= ((int64_t)1 << 40), EP24_E_ARG, "scale_labels: rows must be in [1, 2^40], got %lld", (long long)rows);
    const long total = (long)rows * 51;
    long bx = (total + 255) / 256;
    if (bx > 2048) bx = 2048;
    hipLaunchKernelGGL(scale_labels_kernel, dim3((int)bx), dim3(256), 0, (hipStream_t)stream, in, out, total, scale_x, scale_y);
    EP24_LAUNCH_CHECK("ep24_scale_labels");
    return EP24_OK;
}

extern "C" int ep24_preproc_u8(const uint8_t* images, const int64_t* desc, const double* scales, int n, float* out, int S_h,
                               int S_w, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(images && desc && scales && out && n > 0 && n <= 65535 && S_h > 0 && S_w > 0, EP24_E_ARG, "preproc_u8: bad arguments");
    EP24_REQUIRE(S_w % 4 == 0 && (uintptr_t)out % 16 == 0, EP24_E_ARG, "preproc_u8: the network input width must be a multiple of 4 (it is a multiple of 32)");
    int bx = (S_h * S_w / 4 + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(preproc_u8_kernel, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)desc, scales, out,
                       S_h, S_w);
    EP24_LAUNCH_CHECK("ep24_preproc_u8");
    return EP24_OK;
}

extern "C" int ep24_preproc_labels(const double* rows, const int64_t* row_off, const double* whr, int n, float* out,
                                   int max_labels, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(row_off && whr && out && n > 0 && max_labels > 0, EP24_E_ARG, "preproc_labels: bad arguments");
    hipLaunchKernelGGL(preproc_labels_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, rows, (const long long*)row_off, whr, out,
                       max_labels);
    EP24_LAUNCH_CHECK("ep24_preproc_labels");
    return EP24_OK;
}
