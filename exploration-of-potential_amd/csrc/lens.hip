// ep24 - fisheye lens model (Kannala-Brandt, the model of OpenCV's cv2.fisheye): images, points and 24-point labels between a pinhole
// frame and a fisheye frame, by calibration (include/ep24.h and DESIGN.md section 7 state the contract; tests/lens_oracle.py restates it).
//
// A model is 14 doubles: pinhole fx, fy, cx, cy; fisheye fx, fy, cx, cy; k1..k4; theta_max; thetad(theta_max).  All map arithmetic is
// double, every operation rounded on its own (-ffp-contract=off).  Images: one thread per DESTINATION pixel maps its centre into the
// source frame with the other direction's map and takes an integer bilinear sample (1/32 pixel steps, exact) or the fill value.  The
// work per pixel is the map - atan or 12 Newton steps and a tan, in double - against 12 source bytes (L2 serves the neighbours) and 3
// or 12 bytes written: VALU bound, so the launches are plain: grid (min(ceil(pixels / 256), 4096), n) with a grid stride over the pixels
// of the image, 256 threads.  Labels: labelwarp.h with the lens map in place of the sector map.
#include "common.h"
#include "labelwarp.h"
#include "lensmath.h"

namespace {

constexpr int LENS_D = 14;              // doubles per model
constexpr int LENS_IMG_D = 18;          // doubles per image of the image launches: model, direction, dst h, dst w, dst byte offset
constexpr int LENS_GRID_CAP = 4096;

struct Lens {
    double pfx, pfy, pcx, pcy, ffx, ffy, fcx, fcy, k1, k2, k3, k4, tmax, tdmax;
    __host__ __device__ explicit Lens(const double* m)
        : pfx(m[0]), pfy(m[1]), pcx(m[2]), pcy(m[3]), ffx(m[4]), ffy(m[5]), fcx(m[6]), fcy(m[7]), k1(m[8]), k2(m[9]), k3(m[10]),
          k4(m[11]), tmax(m[12]), tdmax(m[13]) {}
};

// pinhole (u, v) -> fisheye (X, Y); `in`: the point lies inside the field (atan r <= theta_max)
__device__ __forceinline__ void lens_to_fisheye(const Lens& L, double u, double v, double& X, double& Y, bool& in) {
    const double a = (u - L.pcx) / L.pfx, b = (v - L.pcy) / L.pfy;
    const double r = hypot(a, b);
    const double t = atan(r);
    in = t <= L.tmax;
    const double th = fmin(t, L.tmax);
    const double td = lens_thetad(th, L.k1, L.k2, L.k3, L.k4);
    const double s = r > 0.0 ? td / r : 1.0;
    X = L.ffx * a * s + L.fcx;
    Y = L.ffy * b * s + L.fcy;
}

// fisheye (X, Y) -> pinhole (u, v); `in`: inside the field (thetad <= thetad(theta_max)).  Newton on th * P(th^2) = thetad from
// th = thetad, a fixed 12 steps, clamped to [0, theta_max] after each (fmin / fmax also swallow a step that is not a number)
__device__ __forceinline__ void lens_to_pinhole(const Lens& L, double X, double Y, double& u, double& v, bool& in) {
    const double x = (X - L.fcx) / L.ffx, y = (Y - L.fcy) / L.ffy;
    const double rd = hypot(x, y);
    in = rd <= L.tdmax;
    const double td = fmin(rd, L.tdmax);
    const double th = lens_newton(td, L.k1, L.k2, L.k3, L.k4, L.tmax);
    const double s = rd > 0.0 ? tan(th) / rd : 1.0;              // rd, not td: a point beyond the field lands on its rim
    u = L.pfx * x * s + L.pcx;
    v = L.pfy * y * s + L.pcy;
}

__global__ __launch_bounds__(256) void lens_points_kernel(const double* __restrict__ pts, int m, Lens L, int direction,
                                                          double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double X, Y;
    bool in;
    if (direction == 0) lens_to_fisheye(L, pts[2 * i], pts[2 * i + 1], X, Y, in);
    else lens_to_pinhole(L, pts[2 * i], pts[2 * i + 1], X, Y, in);
    out[2 * i] = X; out[2 * i + 1] = Y;
}

// One destination pixel (ox, oy) of an image that goes in `direction` (0 distort: the destination is the fisheye frame, 1 undistort:
// it is the pinhole frame) from the sh x sw source.  Sampled iff inside the field and 0 <= sx <= sw - 1 and 0 <= sy <= sh - 1 (a
// comparison with a NaN is false: fill); then qx <= 32 (sw - 1), so xa <= sw - 1 and every read is inside the source.
__device__ __forceinline__ void lens_pixel(const Lens& L, int direction, const uint8_t* __restrict__ src, int sh, int sw, int ox, int oy,
                                           int fill, int c[3]) {
    double sx, sy;
    bool in;
    if (direction == 0) lens_to_pinhole(L, (double)ox, (double)oy, sx, sy, in);
    else lens_to_fisheye(L, (double)ox, (double)oy, sx, sy, in);
    c[0] = c[1] = c[2] = fill;
    if (in && sx >= 0.0 && sx <= (double)(sw - 1) && sy >= 0.0 && sy <= (double)(sh - 1)) {
        const long qx = (long)floor(sx * 32.0 + 0.5), qy = (long)floor(sy * 32.0 + 0.5);
        const int xa = (int)(qx >> 5), ya = (int)(qy >> 5), wx = (int)(qx & 31), wy = (int)(qy & 31);
        const int xb = min(xa + 1, sw - 1), yb = min(ya + 1, sh - 1);
        const uint8_t* r0 = src + (long)ya * sw * 3;
        const uint8_t* r1 = src + (long)yb * sw * 3;
        const int w00 = (32 - wx) * (32 - wy), w01 = wx * (32 - wy), w10 = (32 - wx) * wy, w11 = wx * wy;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = (w00 * r0[xa * 3 + ch] + w01 * r0[xb * 3 + ch] + w10 * r1[xa * 3 + ch] + w11 * r1[xb * 3 + ch] + 512) >> 10;
    }
}

// grid (x, n): the workgroups of column blockIdx.y stride over the pixels of image blockIdx.y, whatever its size
__global__ __launch_bounds__(256) void lens_warp_u8_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ desc,
                                                           const double* __restrict__ tab, uint8_t* __restrict__ out, int fill) {
    const int n = blockIdx.y;
    const long long* d = desc + (long)n * 3;
    const double* T = tab + (long)n * LENS_IMG_D;
    const Lens L(T);
    const int direction = (int)T[14], dh = (int)T[15], dw = (int)T[16];
    const int sh = (int)d[1], sw = (int)d[2];
    const uint8_t* src = images + d[0];
    uint8_t* o = out + (long)T[17];
    const long total = (long)dh * dw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int oy = (int)(i / dw), ox = (int)(i - (long)oy * dw);
        int c[3];
        lens_pixel(L, direction, src, sh, sw, ox, oy, fill, c);
        o[i * 3 + 0] = (uint8_t)c[0]; o[i * 3 + 1] = (uint8_t)c[1]; o[i * 3 + 2] = (uint8_t)c[2];
    }
}

// the same pixel written as the network input: three fp32 planes of S_h x S_w, a lane's stores contiguous across the wave
__global__ __launch_bounds__(256) void lens_preproc_u8_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ desc,
                                                              const double* __restrict__ tab, float* __restrict__ out, int S_h, int S_w,
                                                              int fill) {
    const int n = blockIdx.y;
    const long long* d = desc + (long)n * 3;
    const double* T = tab + (long)n * LENS_IMG_D;
    const Lens L(T);
    const int direction = (int)T[14];
    const int sh = (int)d[1], sw = (int)d[2];
    const uint8_t* src = images + d[0];
    const int plane = S_h * S_w;                              // < 2^31 - grid stride (checked by the launcher)
    float* o = out + (long)n * 3 * plane;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
        const int oy = i / S_w, ox = i - oy * S_w;
        int c[3];
        lens_pixel(L, direction, src, sh, sw, ox, oy, fill, c);
        o[i] = (float)c[0]; o[plane + i] = (float)c[1]; o[2 * plane + i] = (float)c[2];
    }
}

// the lens map as labelwarp.h takes it: the forward map of the image's direction.  Doubles per image: the model, direction, h, w
// (source image), h', w' (destination), scale, first row, rows
struct LensMap {
    static constexpr int GEO_D = 22, I_OH = 17, I_OW = 18, I_SCALE = 19, I_FIRST = 20, I_ROWS = 21;
    Lens L;
    int direction;
    double h, w;
    __device__ explicit LensMap(const double* G) : L(G), direction((int)G[14]), h(G[15]), w(G[16]) {}
    __device__ __forceinline__ void point(double u, double v, double& X, double& Y) const {
        bool in;
        if (direction == 0) lens_to_fisheye(L, u, v, X, Y, in);
        else lens_to_pinhole(L, u, v, X, Y, in);
    }
};

}  // namespace

extern "C" int ep24_lens_points(const double* points, int m, const double* model, int direction, double* out, void* stream) {
    if (m == 0) return EP24_OK;
    EP24_REQUIRE(points && out && model && m > 0 && (direction == 0 || direction == 1), EP24_E_ARG, "lens_points: bad arguments");
    for (int i = 0; i < LENS_D; ++i) EP24_REQUIRE(model[i] == model[i] && model[i] - model[i] == 0.0, EP24_E_ARG, "lens_points: model[%d] is not finite", i);
    const Lens L(model);
    EP24_REQUIRE(L.pfx > 0.0 && L.pfy > 0.0 && L.ffx > 0.0 && L.ffy > 0.0 && L.tmax > 0.0 && L.tmax < 1.5707963267948966 && L.tdmax > 0.0,
                 EP24_E_ARG, "lens_points: focal lengths and thetad(theta_max) must be positive and 0 < theta_max < pi / 2");
    hipLaunchKernelGGL(lens_points_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, m, L, direction, out);
    EP24_LAUNCH_CHECK("ep24_lens_points");
    return EP24_OK;
}

extern "C" int ep24_lens_warp_u8(const uint8_t* images, const int64_t* desc, const double* table, int n, int64_t max_pixels, uint8_t* out,
                                 int fill, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(images && desc && table && out && n > 0 && n <= 65535 && max_pixels > 0 && fill >= 0 && fill <= 255, EP24_E_ARG,
                 "lens_warp_u8: bad arguments");
    long bx = (max_pixels + 255) / 256;
    if (bx > LENS_GRID_CAP) bx = LENS_GRID_CAP;
    hipLaunchKernelGGL(lens_warp_u8_kernel, dim3((unsigned)bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)desc, table, out,
                       fill);
    EP24_LAUNCH_CHECK("ep24_lens_warp_u8");
    return EP24_OK;
}

extern "C" int ep24_lens_preproc_u8(const uint8_t* images, const int64_t* desc, const double* table, int n, float* out, int S_h, int S_w,
                                    int fill, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(images && desc && table && out && n > 0 && n <= 65535 && S_h > 0 && S_w > 0 && fill >= 0 && fill <= 255, EP24_E_ARG,
                 "lens_preproc_u8: bad arguments");
    EP24_REQUIRE((long)S_h * S_w <= 0x7fffffffL - (long)LENS_GRID_CAP * 256, EP24_E_ARG,
                 "lens_preproc_u8: a plane of %d x %d is beyond the kernel's 31-bit plane index", S_h, S_w);
    long bx = ((long)S_h * S_w + 255) / 256;
    if (bx > LENS_GRID_CAP) bx = LENS_GRID_CAP;
    hipLaunchKernelGGL(lens_preproc_u8_kernel, dim3((unsigned)bx, n), dim3(256), 0, (hipStream_t)stream, images, (const long long*)desc, table,
                       out, S_h, S_w, fill);
    EP24_LAUNCH_CHECK("ep24_lens_preproc_u8");
    return EP24_OK;
}

extern "C" int ep24_lens_labels(const double* rows, const double* geo, const double* rot, int n, int max_labels, float* cand, int32_t* keep,
                                float* out, int32_t* out_count, int32_t* out_flags, void* stream) {
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(rows && geo && rot && cand && keep && out && out_count && out_flags && n > 0 && n <= 65535 && max_labels > 0,
                 EP24_E_ARG, "lens_labels: bad arguments");
    hipLaunchKernelGGL(warp_labels_kernel<LensMap>, dim3((unsigned)((max_labels + LW_ROWS_PER_WG - 1) / LW_ROWS_PER_WG), n), dim3(256), 0,
                       (hipStream_t)stream, rows, geo, rot, max_labels, cand, (int*)keep);
    EP24_LAUNCH_CHECK("ep24_lens_labels");
    hipLaunchKernelGGL(warp_compact_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, cand, (const int*)keep, max_labels, out,
                       (int*)out_count, (int*)out_flags);
    EP24_LAUNCH_CHECK("ep24_lens_labels");
    return EP24_OK;
}
