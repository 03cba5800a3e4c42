// ep24 - tracking of 24-point detections across frames (ep24.track; DESIGN.md section 7, "Tracking"): association by the exact
// area IoU of the 24-gons (poly24.h) in two stages (high scores first, then the low ones against the confirmed tracks of the last
// frame: ByteTrack's scheme), a constant-gain filter on the centre, its velocity and the 24 radii, and the slot bookkeeping.  The
// state lives in tables of the caller's on the device; a frame is two launches and no host synchronisation:
//   cost   one workgroup per (stream, 64 slots, 64 rows): geometry of both sides in LDS, the cheap tests with lane = row, the
//          survivors through an LDS queue so that poly24_iou runs on dense waves (polynms_matrix_kernel's pattern); every word
//          of iou [S][T][N] and dscore [S][N] is written
//   step   one workgroup per stream: rounds of mutual best (the same matches as the sorted greedy), filter, bookkeeping, spawns
//          by ordered scans (wave_scan.h), outputs
// Determinism: integer atomics only (the offset of a queue whose order does not matter); every table word has one writer.
#include "poly24.h"
#include "wave_scan.h"

namespace {

constexpr int TK_NT = 256;
constexpr int TK_VS = 49;            // LDS stride of a polygon's 48 floats: odd, so the lanes of the IoU phase spread over the banks
constexpr int TS_NT = 1024;
constexpr int TS_MAX_T = 1024;       // the step handles one slot per thread
constexpr int TS_MAX_N = 4096;       // and four rows per thread in its scans; the row tables are LDS

enum { TK_OK = 1, TK_NAN = 2 };

// Block (bt, bd) of stream s: slots t0 .. t0 + 63 against rows d0 .. d0 + 63.
__global__ __launch_bounds__(TK_NT) void track_cost_kernel(const float* det, int ncols, const int* count, const float* trk_f,
                                                           const int* trk_i, int T, int N, float low_thre, int agnostic,
                                                           const float* cs, double* iou, float* dscore) {
    __shared__ float verts[128 * TK_VS];
    __shared__ float box[128 * 4];
    __shared__ int cls_sh[128];
    __shared__ unsigned char flag_sh[128];
    __shared__ unsigned short queue[64 * 64];
    __shared__ int nq_sh;
    const int s = blockIdx.z, t0 = blockIdx.y * 64, d0 = blockIdx.x * 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) nq_sh = 0;
    if (tid < 128) {
        // threads 0..63: the predicted polygon of slot t0 + tid; threads 64..127: the polygon of row d0 + tid - 64
        float q[26];
        int c = 0;
        bool ok = false;
        if (tid < 64) {
            const long t = (long)s * T + t0 + tid;
            const int* ti = trk_i + t * 8;
            ok = ti[0] != 0;
            if (ok) {
                const float* f = trk_f + t * 32;
                q[0] = f[0] + f[26];
                q[1] = f[1] + f[27];
                for (int k = 2; k < 26; ++k) q[k] = f[k];
                c = ti[1];
            }
        } else {
            const int d = d0 + tid - 64;
            float score = __builtin_nanf("");
            if (d < N && d < count[s]) {
                const float* row = det + ((long)s * N + d) * ncols;
                const float sc = row[26] * row[27];
                ok = sc >= low_thre;                                   // false for NaN
                if (ok) {
                    score = sc;
                    for (int k = 0; k < 26; ++k) q[k] = row[k];
                    c = (int)row[28];
                }
            }
            if (blockIdx.y == 0 && d < N) dscore[(long)s * N + d] = score;
        }
        int fl = 0;
        if (ok) {
            float v[48];
            poly24_det_vertices(q, cs, v);
            float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
            bool nan = false;
            for (int k = 0; k < 24; ++k) {
                const float px = v[2 * k], py = v[2 * k + 1];
                nan |= px != px || py != py;
                x0 = fminf(x0, px); x1 = fmaxf(x1, px); y0 = fminf(y0, py); y1 = fmaxf(y1, py);
            }
            for (int k = 0; k < 48; ++k) verts[tid * TK_VS + k] = v[k];
            box[tid * 4 + 0] = x0; box[tid * 4 + 1] = y0; box[tid * 4 + 2] = x1; box[tid * 4 + 3] = y1;
            fl = TK_OK | (nan ? TK_NAN : 0);
        }
        cls_sh[tid] = c;
        flag_sh[tid] = (unsigned char)fl;
    }
    __syncthreads();
    const int d = d0 + lane;
    const int bf = flag_sh[64 + lane], bc = cls_sh[64 + lane];
    float bx0 = 0.f, by0 = 0.f, bx1 = 0.f, by1 = 0.f;
    if (bf) { bx0 = box[(64 + lane) * 4]; by0 = box[(64 + lane) * 4 + 1]; bx1 = box[(64 + lane) * 4 + 2]; by1 = box[(64 + lane) * 4 + 3]; }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = w; r < 64; r += 4) {
        const int af = flag_sh[r];
        bool live = af && bf && (agnostic || cls_sh[r] == bc);
        if (live && !((af | bf) & TK_NAN)) {
            // poly24_iou: boxes that do not overlap with positive width and height give exactly 0.0; a NaN vertex goes on to it
            const float ax0 = box[r * 4], ay0 = box[r * 4 + 1], ax1 = box[r * 4 + 2], ay1 = box[r * 4 + 3];
            live = fmin((double)ax1, (double)bx1) - fmax((double)ax0, (double)bx0) > 0.0 &&
                   fmin((double)ay1, (double)by1) - fmax((double)ay0, (double)by0) > 0.0;
        }
        if (!live && d < N) iou[((long)s * T + t0 + r) * N + d] = 0.0;
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
    for (int q = tid; q < nq; q += TK_NT) {
        const int it = queue[q], r = it >> 6, c = it & 63;
        float va[48], vb[48];
        for (int k = 0; k < 48; ++k) { va[k] = verts[r * TK_VS + k]; vb[k] = verts[(64 + c) * TK_VS + k]; }
        iou[((long)s * T + t0 + r) * N + d0 + c] = poly24_iou(va, vb);     // a live row has d0 + c < N
    }
}

// exclusive prefix of v over the workgroup's threads in thread order and the total; every thread calls it; wsum: 17 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    const int inc = wave_incl_sum(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    if (tid < 64) {
        const int x = tid < TS_NT / 64 ? wsum[tid] : 0;
        const int xi = wave_incl_sum(x, tid);
        if (tid < TS_NT / 64) wsum[tid] = xi - x;
        if (tid == 63) wsum[TS_NT / 64] = xi;
    }
    __syncthreads();
    const int r = wsum[w] + inc - v;
    *total = wsum[TS_NT / 64];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TS_NT) void track_step_kernel(const float* det, int ncols, const double* iou, const float* dscore,
                                                           float* trk_f, int* trk_i, int* hdr, int T, int N, float high_thre,
                                                           float new_thre, float match_thre, float match_low_thre, float alpha,
                                                           float beta, float gamma, int max_age, int min_hits, int* det_track,
                                                           float* out_f, int* out_i, int* out_count) {
    __shared__ short row_match[TS_MAX_N], row_choice[TS_MAX_N];
    __shared__ unsigned char row_flag[TS_MAX_N];
    __shared__ short slot_match[TS_MAX_T], slot_choice[TS_MAX_T], spawn_row[TS_MAX_T];
    __shared__ int slot_id[TS_MAX_T];
    __shared__ unsigned char slot_flag[TS_MAX_T];
    __shared__ int wsum[TS_NT / 64 + 1];
    __shared__ int any_sh;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* M = iou + (long)s * T * N;
    const float* ds = dscore + (long)s * N;
    const float* dt = det + (long)s * N * ncols;
    float* tf = trk_f + (long)s * T * 32;
    int* ti = trk_i + (long)s * T * 8;
    int* h = hdr + s * 4;
    const int next_id = h[0], frame = h[1] + 1, dropped = h[2];

    // row_flag: 1 = a row of stage 1 (score >= high_thre), 2 = a row of stage 2 (eligible, below it), 0 = not eligible (dscore NaN)
    for (int d = tid; d < N; d += TS_NT) {
        const float sc = ds[d];
        row_flag[d] = sc >= high_thre ? 1 : (sc == sc ? 2 : 0);
        row_match[d] = -1;
    }
    // slot_flag: bit 1 = live (stage 1), bit 2 = confirmed with age 0 (stage 2)
    if (tid < T) {
        const int id = ti[tid * 8], st = ti[tid * 8 + 2], age = ti[tid * 8 + 4];
        slot_id[tid] = id;
        slot_flag[tid] = id != 0 ? (1 | (st == 2 && age == 0 ? 2 : 0)) : 0;
        slot_match[tid] = -1;
    }
    __syncthreads();

    for (int stage = 1; stage <= 2; ++stage) {
        const double thr = stage == 1 ? (double)match_thre : (double)match_low_thre;
        for (;;) {
            for (int d = tid; d < N; d += TS_NT) row_choice[d] = -1;
            if (tid == 0) any_sh = 0;
            __syncthreads();
            // every unmatched slot takes its best admissible unmatched row (ties: the lower row) - a wave per slot, lane = row
            for (int t = w; t < T; t += TS_NT / 64) {
                if (!(slot_flag[t] & stage) || slot_match[t] >= 0) {
                    if (lane == 0) slot_choice[t] = -1;
                    continue;
                }
                double best = -1.0;
                int bd = -1;
                for (int d = lane; d < N; d += 64) {
                    if (row_flag[d] != stage || row_match[d] >= 0) continue;
                    const double x = M[(long)t * N + d];
                    if (x > thr && x > best) { best = x; bd = d; }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o, 64);
                    const int od = __shfl_xor(bd, o, 64);
                    if (od >= 0 && (bd < 0 || ob > best || (ob == best && od < bd))) { best = ob; bd = od; }
                }
                if (lane == 0) {
                    slot_choice[t] = (short)bd;
                    if (bd >= 0) row_choice[bd] = -2;                  // chosen by somebody: the row looks for its best slot
                }
            }
            __syncthreads();
            // every chosen row takes its best slot (ties: the lower slot)
            for (int d = tid; d < N; d += TS_NT) {
                if (row_choice[d] != -2) continue;
                double best = -1.0;
                int bt = -1;
                for (int t = 0; t < T; ++t) {
                    if (!(slot_flag[t] & stage) || slot_match[t] >= 0) continue;
                    const double x = M[(long)t * N + d];
                    if (x > thr && x > best) { best = x; bt = t; }
                }
                row_choice[d] = (short)bt;
            }
            __syncthreads();
            for (int d = tid; d < N; d += TS_NT) {
                const int bt = row_choice[d];
                if (bt >= 0 && slot_choice[bt] == d) {
                    row_match[d] = (short)bt;
                    slot_match[bt] = (short)d;
                    any_sh = 1;
                }
            }
            __syncthreads();
            const int any = any_sh;
            __syncthreads();
            if (!any) break;
        }
    }

    // the slot's new state, in registers until the spawns are known
    float f[32];
    int iw[8];
    float tail[3] = {0.f, 0.f, 0.f};                                   // columns 26..28 of the matched or spawning row
    for (int k = 0; k < 32; ++k) f[k] = 0.f;
    for (int k = 0; k < 8; ++k) iw[k] = 0;
    if (tid < T && slot_id[tid] != 0) {
        for (int k = 0; k < 29; ++k) f[k] = tf[tid * 32 + k];
        for (int k = 0; k < 7; ++k) iw[k] = ti[tid * 8 + k];
        const float px = f[0] + f[26], py = f[1] + f[27];
        const int d = slot_match[tid];
        if (d >= 0) {
            const float* z = dt + (long)d * ncols;
            const float ex = z[0] - px, ey = z[1] - py;
            f[0] = px + alpha * ex;
            f[1] = py + alpha * ey;
            f[26] = f[26] + beta * ex;
            f[27] = f[27] + beta * ey;
            for (int k = 2; k < 26; ++k) f[k] = f[k] + gamma * (z[k] - f[k]);
            f[28] = ds[d];
            tail[0] = z[26]; tail[1] = z[27]; tail[2] = z[28];
            iw[3] += 1;
            iw[4] = 0;
            if (iw[2] == 3 || (iw[2] == 1 && iw[3] >= min_hits)) iw[2] = 2;
            iw[6] = d;
        } else {
            iw[4] += 1;
            if (iw[2] == 1 || iw[4] > max_age) {
                for (int k = 0; k < 32; ++k) f[k] = 0.f;
                for (int k = 0; k < 8; ++k) iw[k] = 0;
            } else {
                iw[2] = 3;
                f[0] = px;
                f[1] = py;
                iw[6] = -1;
            }
        }
    }
    int nfree, nspawn, nout;
    const int frank = block_excl_scan(tid < T && iw[0] == 0 ? 1 : 0, wsum, tid, &nfree);
    // spawning rows in ascending order: the rows of stage 1 left unmatched with score >= new_thre; four rows per thread
    int cand = 0;
    for (int j = 0; j < 4; ++j) {
        const int d = tid * 4 + j;
        if (d < N && row_flag[d] == 1 && row_match[d] < 0 && ds[d] >= new_thre) cand |= 1 << j;
    }
    int k = block_excl_scan(__popc(cand), wsum, tid, &nspawn);
    for (int j = 0; j < 4; ++j) {
        const int d = tid * 4 + j;
        if (d >= N) break;
        int id = 0;
        if (row_match[d] >= 0) id = slot_id[row_match[d]];
        else if ((cand >> j) & 1) {
            if (k < nfree) { spawn_row[k] = (short)d; id = next_id + k; }
            ++k;
        }
        det_track[(long)s * N + d] = id;
    }
    __syncthreads();
    const int born = nspawn < nfree ? nspawn : nfree;
    if (tid < T && iw[0] == 0 && frank < born) {
        const int d = spawn_row[frank];
        const float* z = dt + (long)d * ncols;
        for (int q = 0; q < 26; ++q) f[q] = z[q];
        f[28] = ds[d];
        tail[0] = z[26]; tail[1] = z[27]; tail[2] = z[28];
        iw[0] = next_id + frank;
        iw[1] = (int)z[28];
        iw[2] = min_hits > 1 ? 1 : 2;
        iw[3] = 1;
        iw[5] = frame;
        iw[6] = d;
    }
    if (tid < T) {
        for (int q = 0; q < 32; ++q) tf[tid * 32 + q] = f[q];
        for (int q = 0; q < 8; ++q) ti[tid * 8 + q] = iw[q];
    }
    // the confirmed slots matched or born in this step, in slot order; the rows after them are zeroed
    const bool shown = tid < T && iw[0] != 0 && iw[2] == 2 && iw[4] == 0;
    const int orank = block_excl_scan(shown ? 1 : 0, wsum, tid, &nout);
    if (shown) {
        float* of = out_f + ((long)s * T + orank) * 29;
        int* oi = out_i + ((long)s * T + orank) * 4;
        for (int q = 0; q < 26; ++q) of[q] = f[q];
        of[26] = tail[0]; of[27] = tail[1]; of[28] = tail[2];
        oi[0] = iw[0]; oi[1] = iw[6]; oi[2] = iw[3]; oi[3] = tid;
    }
    if (tid < T && tid >= nout) {
        float* of = out_f + ((long)s * T + tid) * 29;
        int* oi = out_i + ((long)s * T + tid) * 4;
        for (int q = 0; q < 29; ++q) of[q] = 0.f;
        for (int q = 0; q < 4; ++q) oi[q] = 0;
    }
    if (tid == 0) {
        h[0] = next_id + born;
        h[1] = frame;
        h[2] = dropped + (nspawn - born);
        h[3] = T - nfree + born;
        out_count[s] = nout;
    }
}

bool finite_f(float v) { return v - v == 0.f; }

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_track_cost(const float* det, int ncols, const int32_t* count, const float* trk_f, const int32_t* trk_i, int S,
                               int T, int N, float low_thre, int class_agnostic, const float* ray_cs, double* iou, float* dscore,
                               void* stream) {
    EP24_REQUIRE(det && count && trk_f && trk_i && ray_cs && iou && dscore, EP24_E_ARG, "track_cost: null pointer");
    EP24_REQUIRE(S > 0 && T > 0 && N > 0 && ncols >= 29, EP24_E_ARG, "track_cost: S=%d T=%d N=%d ncols=%d", S, T, N, ncols);
    EP24_REQUIRE(finite_f(low_thre), EP24_E_ARG, "track_cost: low_thre=%g is not finite", (double)low_thre);
    EP24_REQUIRE(T % 64 == 0 && T <= TS_MAX_T, EP24_E_UNSUPPORTED, "track_cost: T=%d (a multiple of 64 in 64..%d)", T, TS_MAX_T);
    EP24_REQUIRE(N <= TS_MAX_N, EP24_E_UNSUPPORTED, "track_cost: N=%d (1..%d rows per stream)", N, TS_MAX_N);
    EP24_REQUIRE(S <= 65535, EP24_E_UNSUPPORTED, "track_cost: S=%d (at most 65535 streams per call)", S);
    hipLaunchKernelGGL(track_cost_kernel, dim3((N + 63) / 64, T / 64, S), dim3(TK_NT), 0, S_, det, ncols, count, trk_f, trk_i, T, N,
                       low_thre, class_agnostic, ray_cs, iou, dscore);
    EP24_LAUNCH_CHECK("ep24_track_cost");
    return EP24_OK;
}

extern "C" int ep24_track_step(const float* det, int ncols, const double* iou, const float* dscore, float* trk_f, int32_t* trk_i,
                               int32_t* hdr, int S, int T, int N, float high_thre, float new_thre, float match_thre,
                               float match_low_thre, float alpha, float beta, float gamma, int max_age, int min_hits,
                               int32_t* det_track, float* out_f, int32_t* out_i, int32_t* out_count, void* stream) {
    EP24_REQUIRE(det && iou && dscore && trk_f && trk_i && hdr && det_track && out_f && out_i && out_count, EP24_E_ARG,
                 "track_step: null pointer");
    EP24_REQUIRE(S > 0 && T > 0 && N > 0 && ncols >= 29, EP24_E_ARG, "track_step: S=%d T=%d N=%d ncols=%d", S, T, N, ncols);
    EP24_REQUIRE(finite_f(high_thre) && finite_f(new_thre) && finite_f(match_thre) && finite_f(match_low_thre), EP24_E_ARG,
                 "track_step: thresholds high=%g new=%g match=%g match_low=%g must be finite", (double)high_thre, (double)new_thre,
                 (double)match_thre, (double)match_low_thre);
    EP24_REQUIRE(match_thre >= 0.f && match_low_thre >= 0.f, EP24_E_ARG,
                 "track_step: match_thre=%g match_low_thre=%g: the box pre-test of the IoU matrix is exact for thresholds >= 0 only",
                 (double)match_thre, (double)match_low_thre);
    EP24_REQUIRE(alpha >= 0.f && alpha <= 1.f && beta >= 0.f && beta <= 1.f && gamma >= 0.f && gamma <= 1.f, EP24_E_ARG,
                 "track_step: gains alpha=%g beta=%g gamma=%g outside [0, 1]", (double)alpha, (double)beta, (double)gamma);
    EP24_REQUIRE(min_hits >= 1 && max_age >= 0, EP24_E_ARG, "track_step: min_hits=%d (>= 1) max_age=%d (>= 0)", min_hits, max_age);
    EP24_REQUIRE(T % 64 == 0 && T <= TS_MAX_T, EP24_E_UNSUPPORTED, "track_step: T=%d (a multiple of 64 in 64..%d)", T, TS_MAX_T);
    EP24_REQUIRE(N <= TS_MAX_N, EP24_E_UNSUPPORTED, "track_step: N=%d (1..%d rows per stream)", N, TS_MAX_N);
    hipLaunchKernelGGL(track_step_kernel, dim3(S), dim3(TS_NT), 0, S_, det, ncols, iou, dscore, trk_f, trk_i, hdr, T, N, high_thre,
                       new_thre, match_thre, match_low_thre, alpha, beta, gamma, max_age, min_hits, det_track, out_f, out_i, out_count);
    EP24_LAUNCH_CHECK("ep24_track_step");
    return EP24_OK;
}
