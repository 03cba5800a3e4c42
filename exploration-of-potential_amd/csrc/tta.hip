// ep24 - test-time augmentation on the postprocess path ("Test-time augmentation"; ep24/tta.py):
//   mirror   a batch of fp32 planes left to right, bit for bit
//   unmap    the decoded prediction rows of one view back into the canonical frame, into their slice of the merged table
//   vote     after ep24_post_nms_poly24: a kept detection becomes the score-weighted consensus of the candidates whose exact
//            area IoU with it (poly24.h, kept row = operand a) is above vote_thre
// Determinism: integer atomics only (the offset of a queue whose order does not matter, ORs into the voter bit mask); every
// floating-point sum has a fixed order.
#include "poly24.h"

namespace {

constexpr int TT_NT = 256;
constexpr int TT_MAX_K = 65536;          // the voter mask holds K / 64 words in LDS (ep24_post_nms_poly24's own limit)
constexpr int TT_TILE = 2048;            // candidates per pre-test tile: the queue holds a tile's survivors and a carried remainder
constexpr int TT_LIST = 1024;            // voters gathered before the ray phase runs on them
constexpr int TT_SLOTS = 10;             // 24 rays x 10 voter slots = 240 of the 256 threads
constexpr int TT_MAX_GX = 256;           // workgroups per image

// ---- mirror --------------------------------------------------------------------------------------------------------------
// Words, not floats: a move of 32 bits keeps every NaN payload.  VEC: W % 4 == 0 and both pointers 16-byte aligned, so every
// row starts aligned; a thread turns one group of four round.
template <bool VEC>
__global__ __launch_bounds__(TT_NT) void mirror_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long rows, int W) {
    const long stride = (long)gridDim.x * TT_NT;
    if constexpr (VEC) {
        const int W4 = W >> 2;
        const long total = rows * W4;
        for (long e = (long)blockIdx.x * TT_NT + threadIdx.x; e < total; e += stride) {
            const long r = e / W4;
            const int q = (int)(e - r * W4);
            const uint4 v = *reinterpret_cast<const uint4*>(in + r * W + (W - 4 - 4 * q));
            *reinterpret_cast<uint4*>(out + r * W + 4 * q) = make_uint4(v.w, v.z, v.y, v.x);
        }
    } else {
        const long total = rows * W;
        for (long e = (long)blockIdx.x * TT_NT + threadIdx.x; e < total; e += stride) {
            const long r = e / W;
            const int x = (int)(e - r * W);
            out[e] = in[r * W + (W - 1 - x)];
        }
    }
}

// ---- unmap ---------------------------------------------------------------------------------------------------------------
// One thread per element of view [B][A_v][ncols].  Every arithmetic result is ONE fp32 operation on fp32 operands (the library
// is built with -ffp-contract=off), columns >= 26 and the identity case move as words.
__global__ __launch_bounds__(TT_NT) void unmap_kernel(const float* __restrict__ view, long total, int A_v, int ncols, float wv, float s,
                                                      int mirror, int identity, float* __restrict__ merged, int A_tot, int off) {
    const long stride = (long)gridDim.x * TT_NT;
    for (long e = (long)blockIdx.x * TT_NT + threadIdx.x; e < total; e += stride) {
        const long row = e / ncols;
        const int col = (int)(e - row * ncols);
        const long b = row / A_v;
        const int a = (int)(row - b * A_v);
        const float* src = view + row * ncols;
        float* dst = merged + ((b * A_tot + off + a) * ncols + col);
        if (identity || col >= 26) {
            *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src + col);
        } else if (col == 0) {
            *dst = mirror ? (wv - src[0]) * s : src[0] * s;
        } else if (col == 1) {
            *dst = src[1] * s;
        } else {
            const int k = col - 2;
            const int ks = mirror ? (36 - k) % 24 : k;             // (12 - k) mod 24
            *dst = src[2 + ks] * s;
        }
    }
}

// ---- vote ----------------------------------------------------------------------------------------------------------------
// (cos, sin)(15 deg * k), k = 0 .. 23, as numpy float64 gives them (np.cos / np.sin of k * (15 * pi / 180)): cos first, then sin
__device__ const double TT_RAY[48] = {
    1.0, 0.9659258262890683, 0.8660254037844387, 0.7071067811865476,
    0.5000000000000001, 0.25881904510252096, 6.123233995736766e-17, -0.25881904510252063,
    -0.4999999999999998, -0.7071067811865475, -0.8660254037844385, -0.9659258262890682,
    -1.0, -0.9659258262890684, -0.8660254037844388, -0.7071067811865479,
    -0.5000000000000004, -0.2588190451025215, -1.8369701987210297e-16, 0.2588190451025203,
    0.49999999999999933, 0.7071067811865474, 0.8660254037844384, 0.9659258262890681,
    0.0, 0.25881904510252074, 0.49999999999999994, 0.7071067811865475,
    0.8660254037844386, 0.9659258262890682, 1.0, 0.9659258262890683,
    0.8660254037844387, 0.7071067811865476, 0.5000000000000003, 0.258819045102521,
    1.2246467991473532e-16, -0.25881904510252035, -0.4999999999999997, -0.7071067811865471,
    -0.8660254037844384, -0.9659258262890681, -1.0, -0.9659258262890684,
    -0.866025403784439, -0.7071067811865477, -0.5000000000000004, -0.25881904510252157,
};

// Nearest crossing t >= 0 of the ray c + t * (dx, dy) with the closed 24-gon v (fp32 vertices, promoted); +inf when there is
// none.  The side-of-line rule of augment_labels_kernel: an edge meets the ray's line iff its ends are on opposite sides of it,
// ends included, and the side of a vertex is ONE number shared by both of its edges.
__device__ __forceinline__ double vote_ray_hit(const float* __restrict__ v, double cx, double cy, double dx, double dy) {
    double best = __longlong_as_double(0x7FF0000000000000LL);
    double px = v[0], py = v[1];
    double sp = dx * (py - cy) - dy * (px - cx);
    for (int j = 0; j < 24; ++j) {
        const int jn = j == 23 ? 0 : j + 1;
        const double qx = v[2 * jn], qy = v[2 * jn + 1];
        const double sq = dx * (qy - cy) - dy * (qx - cx);
        if ((sp <= 0.0 && sq >= 0.0) || (sp >= 0.0 && sq <= 0.0)) {
            if (sp == sq) {                                        // both ends on the line
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
    return best;
}

// Workgroup (x, b) takes the kept entries m = x, x + gridDim.x, ... of image b.  For each:
//   find      the sorted row i of keep[m] by a parallel search of sort_idx
//   voters    tiles of TT_TILE candidates: the fp32 box pre-test of polynms_matrix_kernel, lane = candidate; the survivors go
//             through an LDS queue that carries over from tile to tile, and the exact IoU runs on dense lanes (a = the kept
//             row); voters are ORed into vmask
//   centre    every thread sums the voters of its words (ascending), then a fixed tree over the threads
//   rays      the voters are listed in ascending order, TT_LIST at a time; thread (ray k, slot s) takes the list entries
//             s, s + TT_SLOTS, ... and keeps one partial sum; ray k's thread adds the slots in order
__global__ __launch_bounds__(TT_NT) void vote_kernel(const float* __restrict__ pred, int ncols, const float* __restrict__ score, int A,
                                                     int K, double thr, int agnostic, const int* __restrict__ sidx, int P,
                                                     const int* __restrict__ n_cand,
                                                     const float* __restrict__ verts, const float* __restrict__ vbox,
                                                     const int* __restrict__ vcls, const int* __restrict__ keep,
                                                     const int* __restrict__ keep_count, float* __restrict__ voted,
                                                     int* __restrict__ n_voters) {
    __shared__ unsigned long long vmask[TT_MAX_K / 64];
    __shared__ int queue[TT_TILE + TT_NT];
    __shared__ int list[TT_LIST];
    __shared__ double red[3][TT_NT];
    __shared__ double rsum[2][TT_SLOTS][24];
    __shared__ int wcount[4], lcount[4];
    __shared__ int nq_sh, i_sh;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ep24_post_nms_poly24 leaves 0 <= n <= K and 0 <= kc <= n; other contents must not index past the LDS mask
    const int n = min(max(n_cand[b], 0), K), kc = min(max(keep_count[b], 0), A);
    const int nw = (n + 63) >> 6;
    const long base = (long)b * K;
    const int* idx = sidx + (long)b * P;
    const float* sc = score + (long)b * A;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int m = blockIdx.x; m < kc; m += gridDim.x) {
        const int arow = keep[(long)b * A + m];
        if (tid == 0) { i_sh = -1; nq_sh = 0; }
        for (int x = tid; x < nw; x += TT_NT) vmask[x] = 0ull;
        __syncthreads();
        for (int r = tid; r < n; r += TT_NT)
            if (idx[r] == arow) i_sh = r;                          // a row is listed once
        __syncthreads();
        const int i = i_sh;
        if (i < 0) {                                               // keep[m] is no sorted candidate: not ep24_post_nms_poly24's buffers
            __syncthreads();
            continue;
        }
        const float* krow = pred + ((long)b * A + arow) * ncols;
        float* vo = voted + ((long)b * A + m) * 26;
        const float* bq = vbox + (base + i) * 4;
        const float ax0 = bq[0], ay0 = bq[1], ax1 = bq[2], ay1 = bq[3];
        const int ac = vcls[base + i];
        // ---- voters: the survivors of the pre-test queue up across the tiles, and the IoU runs whenever whole groups of TT_NT of
        // them are waiting (at the last tile: on all that is left), so that its lanes are dense however few a tile yields
        for (int t0 = 0; t0 < n; t0 += TT_TILE) {
            for (int x = 0; x < TT_TILE / TT_NT; ++x) {
                const int j = t0 + x * TT_NT + tid;
                bool live = false;
                if (j < n && j != i) {
                    const float* q = vbox + (base + j) * 4;
                    const float bx0 = q[0], by0 = q[1], bx1 = q[2], by1 = q[3];
                    live = agnostic || vcls[base + j] == ac;
                    // poly24_iou: boxes that do not overlap with positive width and height give exactly 0.0, never > thr >= 0
                    live = live && fmin((double)ax1, (double)bx1) - fmax((double)ax0, (double)bx0) > 0.0 &&
                           fmin((double)ay1, (double)by1) - fmax((double)ay0, (double)by0) > 0.0;
                }
                const unsigned long long mk = __ballot(live);
                if (mk) {
                    int qb = 0;
                    if (lane == 0) qb = atomicAdd(&nq_sh, __popcll(mk));
                    qb = __shfl(qb, 0, 64);
                    if (live) queue[qb + __popcll(mk & lt)] = j;   // at most TT_NT - 1 carried over + TT_TILE new ones
                }
            }
            __syncthreads();
            const int nq = nq_sh;
            const int run = t0 + TT_TILE >= n ? nq : nq / TT_NT * TT_NT;
            for (int q = tid; q < run; q += TT_NT) {
                const int j = queue[q];
                const float* pa = verts + (base + i) * 48;
                const float* pb = verts + (base + j) * 48;
                float va[48], vb[48];
                for (int k = 0; k < 48; ++k) { va[k] = pa[k]; vb[k] = pb[k]; }
                const double iou = poly24_iou(va, vb);
                if (iou > thr) atomicOr(&vmask[j >> 6], 1ull << (j & 63));    // false for NaN
            }
            const int rem = nq - run;                              // < TT_NT: they wait for the next tile, at the queue's front
            const int carry = tid < rem ? queue[run + tid] : 0;
            __syncthreads();
            if (tid < rem) queue[tid] = carry;
            if (tid == 0) nq_sh = rem;
            __syncthreads();
        }
        if (tid == 0) vmask[i >> 6] |= 1ull << (i & 63);           // the kept row always votes, NaN or not
        __syncthreads();
        // ---- centre: sum w, sum w x, sum w y
        double sw = 0.0, sx = 0.0, sy = 0.0;
        int cnt = 0;
        for (int x = tid; x < nw; x += TT_NT) {
            unsigned long long mk = vmask[x];
            cnt += __popcll(mk);
            while (mk) {
                const int j = x * 64 + __ffsll((long long)mk) - 1;
                mk &= mk - 1;
                const int a = idx[j];
                const double w = (double)sc[a];
                const float* pr = pred + ((long)b * A + a) * ncols;
                sw += w;
                sx += w * (double)pr[0];
                sy += w * (double)pr[1];
            }
        }
        red[0][tid] = sw; red[1][tid] = sx; red[2][tid] = sy;
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) wcount[wv] = cnt;
        __syncthreads();
        for (int o = TT_NT / 2; o > 0; o >>= 1) {
            if (tid < o) {
                red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o];
            }
            __syncthreads();
        }
        const int nv = wcount[0] + wcount[1] + wcount[2] + wcount[3];
        const double W = red[0][0];
        if (tid == 0) n_voters[(long)b * A + m] = nv;
        if (nv <= 1 || !(W > 0.0)) {                               // one voter, or no weight to share out: the kept row itself
            if (tid < 26) reinterpret_cast<uint32_t*>(vo)[tid] = reinterpret_cast<const uint32_t*>(krow)[tid];
            __syncthreads();
            continue;
        }
        const double cx = red[1][0] / W, cy = red[2][0] / W;
        // ---- rays
        const int rk = tid % 24, rs = tid / 24;                    // rs < TT_SLOTS for the 240 working threads
        const double dx = TT_RAY[rk], dy = TT_RAY[24 + rk];
        double at = 0.0, aw = 0.0;
        int nl = 0;                                                // voters in the list
        for (int g0 = 0; g0 < nw; g0 += 4) {
            // the 256 candidates of words g0 .. g0 + 3 are appended in ascending order: wave = word, lane = bit
            const int wd = g0 + wv;
            const unsigned long long mk = wd < nw ? vmask[wd] : 0ull;
            if (lane == 0) lcount[wv] = __popcll(mk);
            __syncthreads();
            int pos = nl;
            for (int x = 0; x < wv; ++x) pos += lcount[x];
            if ((mk >> lane) & 1ull) list[pos + __popcll(mk & lt)] = wd * 64 + lane;
            nl += lcount[0] + lcount[1] + lcount[2] + lcount[3];
            __syncthreads();
            if (nl > TT_LIST - TT_NT || g0 + 4 >= nw) {            // no room for another 256, or the last group: the ray phase
                if (rs < TT_SLOTS) {
                    for (int e = rs; e < nl; e += TT_SLOTS) {
                        const int j = list[e];
                        const double t = vote_ray_hit(verts + (base + j) * 48, cx, cy, dx, dy);
                        if (t < __longlong_as_double(0x7FF0000000000000LL)) {    // no crossing: the voter abstains on this ray
                            const double w = (double)sc[idx[j]];
                            at += w * t;
                            aw += w;
                        }
                    }
                }
                nl = 0;
            }
        }
        if (rs < TT_SLOTS) { rsum[0][rs][rk] = at; rsum[1][rs][rk] = aw; }
        __syncthreads();
        if (tid < 24) {
            double t = 0.0, w = 0.0;
            for (int s = 0; s < TT_SLOTS; ++s) { t += rsum[0][s][tid]; w += rsum[1][s][tid]; }
            if (w > 0.0) vo[2 + tid] = (float)(t / w);
            else reinterpret_cast<uint32_t*>(vo)[2 + tid] = reinterpret_cast<const uint32_t*>(krow)[2 + tid];
        } else if (tid == 24) {
            vo[0] = (float)cx;
        } else if (tid == 25) {
            vo[1] = (float)cy;
        }
        __syncthreads();
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_mirror_f32(const float* in, int N, int H, int W, float* out, void* stream) {
    EP24_REQUIRE(in && out, EP24_E_ARG, "mirror_f32: null pointer");
    EP24_REQUIRE(in != out, EP24_E_ARG, "mirror_f32: in == out (the mirror is not done in place)");
    EP24_REQUIRE(N >= 0 && H >= 0 && W >= 0, EP24_E_ARG, "mirror_f32: N=%d H=%d W=%d", N, H, W);
    const long rows = (long)N * H;
    if (rows == 0 || W == 0) return EP24_OK;
    const bool vec = W % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    const long items = vec ? rows * (W / 4) : rows * W;
    long g = (items + TT_NT - 1) / TT_NT;
    if (g > 16384) g = 16384;
    if (vec)
        hipLaunchKernelGGL(mirror_kernel<true>, dim3((unsigned)g), dim3(TT_NT), 0, S_, (const uint32_t*)in, (uint32_t*)out, rows, W);
    else
        hipLaunchKernelGGL(mirror_kernel<false>, dim3((unsigned)g), dim3(TT_NT), 0, S_, (const uint32_t*)in, (uint32_t*)out, rows, W);
    EP24_LAUNCH_CHECK("ep24_mirror_f32");
    return EP24_OK;
}

extern "C" int ep24_tta_unmap(const float* view, int B, int A_v, int ncols, int w_v, float s, int mirror, float* merged, int A_tot,
                              int off, void* stream) {
    EP24_REQUIRE(view && merged, EP24_E_ARG, "tta_unmap: null pointer");
    EP24_REQUIRE(B > 0 && A_v > 0 && A_tot > 0 && w_v > 0, EP24_E_ARG, "tta_unmap: B=%d A_v=%d A_tot=%d w_v=%d", B, A_v, A_tot, w_v);
    EP24_REQUIRE(ncols >= 27, EP24_E_ARG, "tta_unmap: ncols=%d (a decoded row has at least 27 columns)", ncols);
    EP24_REQUIRE(off >= 0 && (long)off + A_v <= A_tot, EP24_E_ARG, "tta_unmap: rows [%d, %d + %d) do not fit A_tot=%d", off, off, A_v,
                 A_tot);
    EP24_REQUIRE(s > 0.f && s <= 3.4028234663852886e38f, EP24_E_ARG, "tta_unmap: scale %g must be finite and positive", (double)s);
    const long total = (long)B * A_v * ncols;
    long g = (total + TT_NT - 1) / TT_NT;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(unmap_kernel, dim3((unsigned)g), dim3(TT_NT), 0, S_, view, total, A_v, ncols, (float)w_v, s, mirror ? 1 : 0,
                       (s == 1.0f && !mirror) ? 1 : 0, merged, A_tot, off);
    EP24_LAUNCH_CHECK("ep24_tta_unmap");
    return EP24_OK;
}

extern "C" int ep24_post_vote_poly24(const float* pred, int ncols, const float* score, int B, int A, int K, float vote_thre,
                                     int class_agnostic, const int32_t* sort_idx, int P, const int32_t* n_cand,
                                     const float* verts, const float* vbox, const int32_t* vcls, const int32_t* keep,
                                     const int32_t* keep_count, float* voted, int32_t* n_voters, void* stream) {
    EP24_REQUIRE(pred && score && sort_idx && n_cand && verts && vbox && vcls && keep && keep_count && voted && n_voters,
                 EP24_E_ARG, "post_vote_poly24: null pointer");
    EP24_REQUIRE(B > 0 && A > 0 && ncols >= 27, EP24_E_ARG, "post_vote_poly24: B=%d A=%d ncols=%d", B, A, ncols);
    EP24_REQUIRE(K >= 1 && K <= A, EP24_E_ARG, "post_vote_poly24: K=%d candidates per image (1..A=%d)", K, A);
    EP24_REQUIRE(P >= A && (P & (P - 1)) == 0, EP24_E_ARG, "post_vote_poly24: scratch rows P=%d must be a power of two >= A=%d", P, A);
    EP24_REQUIRE(vote_thre >= 0.f, EP24_E_ARG, "post_vote_poly24: vote_thre=%g: the box pre-test is exact for thresholds >= 0 only",
                 (double)vote_thre);
    EP24_REQUIRE(K <= TT_MAX_K, EP24_E_UNSUPPORTED, "post_vote_poly24: K=%d (at most %d candidates per image)", K, TT_MAX_K);
    EP24_REQUIRE(B <= 65535, EP24_E_UNSUPPORTED, "post_vote_poly24: B=%d (at most 65535 images per call)", B);
    const int gx = K < TT_MAX_GX ? K : TT_MAX_GX;
    hipLaunchKernelGGL(vote_kernel, dim3(gx, B), dim3(TT_NT), 0, S_, pred, ncols, score, A, K, (double)vote_thre, class_agnostic,
                       sort_idx, P, n_cand, verts, vbox, vcls, keep, keep_count, voted, n_voters);
    EP24_LAUNCH_CHECK("ep24_post_vote_poly24");
    return EP24_OK;
}
