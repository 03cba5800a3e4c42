// ep24 - polygon NMS: greedy suppression of 24-point detections by the exact area IoU of their own polygons (poly24.h), the
// nms_iou = "poly24" path of postprocess and of the evaluator.  Candidates, order and class rule are
// nms_kernel's (infer.hip); only the IoU differs.
//
// nms_kernel walks the sorted list serially, one workgroup per image, and tests a rectangle pair in a dozen fp32 operations.
// A polygon pair costs about 23 k fp64 operations, so the work is split:
//   sort      one workgroup per image: compact + bitonic sort (nms_sort.h), n_cand = min(candidates, K)
//   geometry  one thread per sorted candidate: 24 vertices, their box, the class
//   matrix    one workgroup per (image, 64 rows, 64 columns) at and above the diagonal: bit (i, j) = "i would remove j"
//   scan      one workgroup per image: the greedy pass over the bit matrix
// Determinism: integer atomics only (the compaction offset of a queue whose order does not matter, ORs into a bit word).
#include "nms_sort.h"
#include "poly24.h"

namespace {

constexpr int PN_MAX_K = 65536;      // the scan holds K / 64 words of "removed" bits in LDS
constexpr int PN_NT = 256;

__global__ __launch_bounds__(1024) void polynms_sort_kernel(const float* score, int A, int K, float* skey, int* sidx, int* n_cand,
                                                            int P) {
    __shared__ int n_sh;
    const int b = blockIdx.x;
    const int n = nms_compact_sort<1024>(score + (long)b * A, A, skey + (long)b * P, sidx + (long)b * P, &n_sh);
    if (threadIdx.x == 0) n_cand[b] = n < K ? n : K;
}

// Sorted candidate r of image b: vertices as the evaluator forms a detection's, their fp32 box (x0, y0, x1, y1) and the class.
// A row with a NaN vertex gets a NaN box: every comparison of the matrix kernel's box test is then false, as poly24_iou's NaN
// is never above a threshold.
__global__ __launch_bounds__(PN_NT) void polynms_geometry_kernel(const float* pred, int ncols, const int* cls, const int* sidx,
                                                                 const int* n_cand, int B, int A, int K, int P, const float* cs,
                                                                 float* verts, float* vbox, int* vcls) {
    const long i = (long)blockIdx.x * PN_NT + threadIdx.x;
    if (i >= (long)B * K) return;
    const int b = (int)(i / K), r = (int)(i - (long)b * K);
    if (r >= n_cand[b]) return;
    const int a = sidx[(long)b * P + r];
    float v[48];
    poly24_det_vertices(pred + ((long)b * A + a) * ncols, cs, v);
    float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    bool nan = false;
    for (int k = 0; k < 24; ++k) {
        const float px = v[2 * k], py = v[2 * k + 1];
        nan |= px != px || py != py;
        x0 = fminf(x0, px); x1 = fmaxf(x1, px); y0 = fminf(y0, py); y1 = fmaxf(y1, py);
    }
    if (nan) x0 = y0 = x1 = y1 = __builtin_nanf("");
    float* o = verts + i * 48;
    for (int k = 0; k < 48; ++k) o[k] = v[k];
    vbox[i * 4 + 0] = x0; vbox[i * 4 + 1] = y0; vbox[i * 4 + 2] = x1; vbox[i * 4 + 3] = y1;
    vcls[i] = cls[(long)b * A + a];
}

// first block of row-block bi in the row-major enumeration of the upper triangle of an nb x nb block grid
__device__ __forceinline__ long tri_start(long bi, long nb) { return bi * nb - bi * (bi - 1) / 2; }

// Block (bi, bj), bj >= bi, of image b: rows i = 64 bi + r, columns j = 64 bj + c.  A wave takes a row at a time with lane = column
// and does the cheap tests (j > i, j < n, class, vertex boxes overlap - the test poly24_iou itself starts with, on the same
// values: the fp32 box promoted is the double min / max of the promoted vertices); a few per cent of the pairs survive them.  Run
// in place, poly24_iou would hold a wave at a few live lanes for 576 edge pairs, so the survivors go through an LDS queue (as
// cost_kernel of assign.hip compacts its lens items) and the IoU runs on dense waves, one lane a whole pair with
// a = suppressor, b = candidate: the value eval_iou_kernel gives for the same operands.  The block's 64 words are assembled in LDS
// and every one of them with a row < n is stored, so the scan reads nothing this launch did not write.
__global__ __launch_bounds__(PN_NT) void polynms_matrix_kernel(const float* verts, const float* vbox, const int* vcls,
                                                               const int* n_cand, int K, int nb, double thr, int agnostic,
                                                               unsigned long long* mask) {
    __shared__ unsigned long long words[64];
    __shared__ unsigned short queue[64 * 64];
    __shared__ int nq_sh;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = n_cand[b];
    const long t = blockIdx.x;
    long bi = (long)((2.0 * nb + 1.0 - sqrt((2.0 * nb + 1.0) * (2.0 * nb + 1.0) - 8.0 * (double)t)) * 0.5);
    bi = bi < 0 ? 0 : (bi > nb - 1 ? nb - 1 : bi);
    while (bi + 1 < nb && tri_start(bi + 1, nb) <= t) ++bi;
    while (bi > 0 && tri_start(bi, nb) > t) --bi;
    const int bj = (int)(bi + (t - tri_start(bi, nb)));
    const int i0 = (int)bi * 64, j0 = bj * 64;
    if (i0 >= n || j0 >= n) return;                                // the grid is sized for K: blocks beyond the candidates exit
    const long base = (long)b * K;
    if (tid < 64) words[tid] = 0ull;
    if (tid == 0) nq_sh = 0;
    __syncthreads();
    const int j = j0 + lane;
    float bx0 = 0.f, by0 = 0.f, bx1 = 0.f, by1 = 0.f;
    int bc = 0;
    if (j < n) {
        const float* q = vbox + (base + j) * 4;
        bx0 = q[0]; by0 = q[1]; bx1 = q[2]; by1 = q[3];
        bc = vcls[base + j];
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = w; r < 64; r += 4) {
        const int i = i0 + r;
        if (i >= n) break;
        const float* q = vbox + (base + i) * 4;
        const float ax0 = q[0], ay0 = q[1], ax1 = q[2], ay1 = q[3];
        bool live = j > i && j < n && (agnostic || vcls[base + i] == bc);
        // poly24_iou: boxes that do not overlap with positive width and height give exactly 0.0, which is never > thr >= 0
        live = live && fmin((double)ax1, (double)bx1) - fmax((double)ax0, (double)bx0) > 0.0 &&
               fmin((double)ay1, (double)by1) - fmax((double)ay0, (double)by0) > 0.0;
        const unsigned long long m = __ballot(live);
        if (m) {
            int qb = 0;
            if (lane == 0) qb = atomicAdd(&nq_sh, __popcll(m));
            qb = __shfl(qb, 0, 64);
            if (live) queue[qb + __popcll(m & lt)] = (unsigned short)(r * 64 + lane);
        }
    }
    __syncthreads();
    const int nq = nq_sh;
    for (int q = tid; q < nq; q += PN_NT) {
        const int it = queue[q], r = it >> 6, c = it & 63;
        const float* pa = verts + (base + i0 + r) * 48;
        const float* pb = verts + (base + j0 + c) * 48;
        float va[48], vb[48];
        for (int k = 0; k < 48; ++k) { va[k] = pa[k]; vb[k] = pb[k]; }
        const double iou = poly24_iou(va, vb);
        if (iou > thr) atomicOr(&words[r], 1ull << c);            // false for NaN
    }
    __syncthreads();
    if (tid < 64 && i0 + tid < n) mask[(base + i0 + tid) * nb + bj] = words[tid];
}

// The greedy pass.  For the 64 candidates of word w in turn: wave 0 resolves them against each other (the diagonal words of their
// rows, one per lane, handed round by shuffles) starting from the bits better candidates left in removed[w], appends the kept ones
// to `keep` in order, and all threads then OR the kept rows into the words after w.
__global__ __launch_bounds__(PN_NT) void polynms_scan_kernel(const unsigned long long* mask, const int* sidx, const int* n_cand, int A,
                                                             int K, int nb, int P, int* keep, int* keep_count) {
    __shared__ unsigned long long removed[PN_MAX_K / 64];
    __shared__ unsigned long long kmask_sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_cand[b];
    const int nw = (n + 63) >> 6;
    const unsigned long long* mk = mask + (long)b * K * nb;
    const int* idx = sidx + (long)b * P;
    int* kp = keep + (long)b * A;
    for (int x = tid; x < nw; x += PN_NT) removed[x] = 0ull;
    __syncthreads();
    int kept = 0;
    for (int w = 0; w < nw; ++w) {
        if (tid < 64) {
            const int i = w * 64 + tid;
            const unsigned long long d = i < n ? mk[(long)i * nb + w] : 0ull;
            unsigned long long cur = removed[w], km = 0ull;
            const int top = n - w * 64 < 64 ? n - w * 64 : 64;
            for (int bit = 0; bit < top; ++bit) {
                const unsigned long long db = __shfl(d, bit, 64);
                if (!((cur >> bit) & 1ull)) { km |= 1ull << bit; cur |= db; }
            }
            if ((km >> tid) & 1ull) kp[kept + __popcll(km & ((1ull << tid) - 1ull))] = idx[i];
            if (tid == 0) kmask_sh = km;
        }
        __syncthreads();
        const unsigned long long km = kmask_sh;
        kept += __popcll(km);
        for (int x = w + 1 + tid; x < nw; x += PN_NT) {
            unsigned long long acc = removed[x], m = km;
            while (m) {
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1;
                acc |= mk[(long)(w * 64 + bit) * nb + x];
            }
            removed[x] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) keep_count[b] = kept;
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_post_nms_poly24(const float* pred, int ncols, const float* score, const int32_t* cls, int B, int A, int K,
                                    float nms_thre, int class_agnostic, const float* ray_cs, float* sort_key, int32_t* sort_idx, int P,
                                    int32_t* n_cand, float* verts, float* vbox, int32_t* vcls, uint64_t* mask, int32_t* keep,
                                    int32_t* keep_count, void* stream) {
    EP24_REQUIRE(pred && score && cls && ray_cs && sort_key && sort_idx && n_cand && verts && vbox && vcls && mask && keep && keep_count,
                 EP24_E_ARG, "post_nms_poly24: null pointer");
    EP24_REQUIRE(B > 0 && A > 0 && ncols >= 27, EP24_E_ARG, "post_nms_poly24: B=%d A=%d ncols=%d", B, A, ncols);
    EP24_REQUIRE(K >= 1 && K <= A, EP24_E_ARG, "post_nms_poly24: K=%d candidates per image (1..A=%d)", K, A);
    EP24_REQUIRE(P >= A && (P & (P - 1)) == 0, EP24_E_ARG, "post_nms_poly24: scratch rows P=%d must be a power of two >= A=%d", P, A);
    EP24_REQUIRE(nms_thre >= 0.f, EP24_E_ARG, "post_nms_poly24: nms_thre=%g: the box pre-test is exact for thresholds >= 0 only",
                 (double)nms_thre);
    EP24_REQUIRE(K <= PN_MAX_K, EP24_E_UNSUPPORTED, "post_nms_poly24: K=%d (at most %d candidates per image)", K, PN_MAX_K);
    EP24_REQUIRE(B <= 65535, EP24_E_UNSUPPORTED, "post_nms_poly24: B=%d (at most 65535 images per call)", B);
    const int nb = (K + 63) / 64;
    hipLaunchKernelGGL(polynms_sort_kernel, dim3(B), dim3(1024), 0, S_, score, A, K, sort_key, sort_idx, n_cand, P);
    hipLaunchKernelGGL(polynms_geometry_kernel, dim3((unsigned)(((long)B * K + PN_NT - 1) / PN_NT)), dim3(PN_NT), 0, S_, pred, ncols, cls,
                       sort_idx, n_cand, B, A, K, P, ray_cs, verts, vbox, vcls);
    hipLaunchKernelGGL(polynms_matrix_kernel, dim3((unsigned)((long)nb * (nb + 1) / 2), B), dim3(PN_NT), 0, S_, verts, vbox, vcls, n_cand, K,
                       nb, (double)nms_thre, class_agnostic, (unsigned long long*)mask);
    hipLaunchKernelGGL(polynms_scan_kernel, dim3(B), dim3(PN_NT), 0, S_, (const unsigned long long*)mask, sort_idx, n_cand, A, K, nb, P, keep,
                       keep_count);
    EP24_LAUNCH_CHECK("ep24_post_nms_poly24");
    return EP24_OK;
}
