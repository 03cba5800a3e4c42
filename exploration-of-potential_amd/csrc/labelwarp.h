// ep24 - 24-point labels under a continuous point map: outline -> centre -> rays -> row, and the ordered
// compaction.  Shared by the sector warp (sector.hip, ep24_sector_labels) and the lens model (lens.hip, ep24_lens_labels): the text is
// the same, only the map differs.  A map is a struct
//     static constexpr int GEO_D, I_OH, I_OW, I_SCALE, I_FIRST, I_ROWS;   doubles per image in the parameter table and where the size of
//                                                                          the mapped image, the output scale, the index of the image's
//                                                                          first row and its row count stand in it
//     __device__ explicit Map(const double* G);                            from the image's entry of the table
//     double h, w;                                                         the source image: rows are normalised by them
//     __device__ void point(double u, double v, double& X, double& Y) const;
// All double; no floating-point atomics; results do not depend on the order in which anything ran.
#pragma once
#include "common.h"

namespace {

constexpr int LW_SUB = 8;                  // pieces per polygon edge
constexpr int LW_NPT = 24 * LW_SUB;        // outline points per label: 3 per lane of one wave
constexpr int LW_ROWS_PER_WG = 4;          // one wave per label row

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (ceil(max_labels / 4), n), 256 threads: wave wv of workgroup bx handles label row 4*bx + wv of image blockIdx.y.  Every row slot
// j < max_labels gets its keep word (bit 0 keep, bit 1 centre fell back) and, when kept, its candidate row; warp_compact_kernel
// packs them.  The barriers are outside every divergent branch: a wave without a row runs through them with `active` false.
template <class Map>
__global__ __launch_bounds__(256) void warp_labels_kernel(const double* __restrict__ rows, const double* __restrict__ geo,
                                                          const double* __restrict__ rot, int max_labels,
                                                          float* __restrict__ cand, int* __restrict__ keep) {
    constexpr int SUB = LW_SUB, NPT = LW_NPT, ROWS_PER_WG = LW_ROWS_PER_WG;
    __shared__ double sO[ROWS_PER_WG][NPT][2];
    const int n = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * ROWS_PER_WG + wv;
    const double* G = geo + (long)n * Map::GEO_D;
    long cnt = (long)G[Map::I_ROWS];
    cnt = cnt < 0 ? 0 : (cnt > max_labels ? max_labels : cnt);
    const bool active = j < cnt;
    const Map g(G);
    const double oh = G[Map::I_OH], ow = G[Map::I_OW], lb = G[Map::I_SCALE];
    const double* row = rows + ((long)G[Map::I_FIRST] + (active ? j : 0)) * 51;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    double x1 = inf, y1 = inf, x2 = -inf, y2 = -inf;
    if (active) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = lane * 3 + i, k = idx / SUB, s = idx - k * SUB, kn = k == 23 ? 0 : k + 1;
            const double px = row[3 + 2 * k] * g.w, py = row[4 + 2 * k] * g.h;
            const double qx = row[3 + 2 * kn] * g.w, qy = row[4 + 2 * kn] * g.h;
            const double f = (double)s / (double)SUB;
            double X, Y;
            g.point(px + f * (qx - px), py + f * (qy - py), X, Y);
            sO[wv][idx][0] = X; sO[wv][idx][1] = Y;
            x1 = fmin(x1, X); x2 = fmax(x2, X); y1 = fmin(y1, Y); y2 = fmax(y2, Y);
        }
    }
    __syncthreads();
    if (!active) {
        if (lane == 0 && j < max_labels) keep[(long)n * max_labels + j] = 0;
        return;                                                     // no barrier below this line
    }
    x1 = wave_min(x1); y1 = wave_min(y1); x2 = wave_max(x2); y2 = wave_max(y2);
    double cx = (x1 + x2) / 2.0, cy = (y1 + y2) / 2.0;
    // even-odd rule: three edges per lane, the parity of the wave's crossings
    int crossings = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int idx = lane * 3 + i, nx = idx == NPT - 1 ? 0 : idx + 1;
        const double px = sO[wv][idx][0], py = sO[wv][idx][1], qx = sO[wv][nx][0], qy = sO[wv][nx][1];
        if ((py > cy) != (qy > cy)) {
            const double xc = px + (cy - py) * (qx - px) / (qy - py);
            crossings += xc > cx ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) crossings += __shfl_xor(crossings, o, 64);
    const int fell_back = (crossings & 1) ? 0 : 1;
    if (fell_back) g.point(row[1] * g.w, row[2] * g.h, cx, cy);
    // ray k on lane k < 24 against the closed outline (augment_labels_kernel's rule: one side value per vertex, ends included)
    double nx_ = 0.0, ny_ = 0.0;
    if (lane < 24) {
        const double dx = rot[2 * lane], dy = rot[2 * lane + 1];
        double best = inf;
        double px = sO[wv][0][0], py = sO[wv][0][1];
        double sp = dx * (py - cy) - dy * (px - cx);
        for (int e = 0; e < NPT; ++e) {
            const int en = e == NPT - 1 ? 0 : e + 1;
            const double qx = sO[wv][en][0], qy = sO[wv][en][1];
            const double sq = dx * (qy - cy) - dy * (qx - cx);
            if ((sp <= 0.0 && sq >= 0.0) || (sp >= 0.0 && sq <= 0.0)) {
                if (sp == sq) {                                    // both ends on the line
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
        if (best == inf) best = 0.0;                               // a ray that meets no edge stays at the centre
        nx_ = fmin(fmax(cx + best * dx, 0.0), ow) * lb;
        ny_ = fmin(fmax(cy + best * dy, 0.0), oh) * lb;
    }
    const bool ray = lane < 24;
    const double ex1 = wave_min(ray ? nx_ : inf), ex2 = wave_max(ray ? nx_ : -inf);
    const double ey1 = wave_min(ray ? ny_ : inf), ey2 = wave_max(ray ? ny_ : -inf);
    const bool kept = fmin(ex2 - ex1, ey2 - ey1) > 1.0;           // TrainTransform's filter: min(width, height) > 1
    // column c of the candidate row on lane c: class, centre, then vertex (c - 3) / 2 from the lane that cast it
    const int col = lane < 51 ? lane : 50;
    const int src = col >= 3 ? (col - 3) >> 1 : 0;
    const double vx = __shfl(nx_, src, 64), vy = __shfl(ny_, src, 64);
    if (kept && lane < 51) {
        const double v = col == 0 ? row[0] : (col == 1 ? cx * lb : (col == 2 ? cy * lb : (((col - 3) & 1) ? vy : vx)));
        cand[((long)n * max_labels + j) * 51 + col] = (float)v;
    }
    if (lane == 0) keep[(long)n * max_labels + j] = (kept ? 1 : 0) | (fell_back << 1);
}

// One workgroup per image: the kept candidates in row order, the rest of the table zero.  256 row slots per pass, their output slots
// from a ballot prefix, so nothing depends on the order in which anything ran.
__global__ __launch_bounds__(256) void warp_compact_kernel(const float* __restrict__ cand, const int* __restrict__ keep,
                                                           int max_labels, float* __restrict__ out, int* __restrict__ out_count,
                                                           int* __restrict__ out_flags) {
    __shared__ int sSlot[256];
    __shared__ int sWave[4];
    const int n = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const float* C = cand + (long)n * max_labels * 51;
    const int* K = keep + (long)n * max_labels;
    float* O = out + (long)n * max_labels * 51;
    int* Fl = out_flags + (long)n * max_labels;
    int kept0 = 0;
    for (int base = 0; base < max_labels; base += 256) {
        const int jj = base + tid;
        const int kw = jj < max_labels ? K[jj] : 0;
        const unsigned long long b = __ballot(kw & 1);
        if (lane == 0) sWave[wv] = __popcll(b);
        __syncthreads();
        int slot = kept0 + __popcll(b & ((1ULL << lane) - 1ULL));
        for (int w = 0; w < wv; ++w) slot += sWave[w];
        sSlot[tid] = (kw & 1) ? slot : -1;
        if (kw & 1) Fl[slot] = kw >> 1;
        const int total = sWave[0] + sWave[1] + sWave[2] + sWave[3];
        __syncthreads();
        const int in_pass = min(256, max_labels - base);
        for (int e = tid; e < in_pass * 51; e += 256) {
            const int c = e / 51, col = e - c * 51;
            const int s = sSlot[c];
            if (s >= 0) O[(long)s * 51 + col] = C[(long)(base + c) * 51 + col];
        }
        kept0 += total;
        __syncthreads();
    }
    for (int e = kept0 * 51 + tid; e < max_labels * 51; e += 256) O[e] = 0.f;
    for (int e = kept0 + tid; e < max_labels; e += 256) Fl[e] = 0;
    if (tid == 0) out_count[n] = kept0;
}

}  // namespace
