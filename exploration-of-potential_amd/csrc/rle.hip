// ep24 - bit-packed instance masks -> COCO run lengths on the GPU: pycocotools' rleEncode without a byte per pixel and without a
// host loop.
//
// rleEncode walks a mask column-major (p = x * H + y) from a previous value of 0; every change of value closes a run and the end
// of the mask closes the last one.  So the positions p with bit(p) != bit(p - 1), bit(-1) = 0, in ascending order and followed by
// H * W, are the inclusive prefix sums ("ends") of the counts.  The pixel before (x, 0) is (x - 1, H - 1).
//   pack_bytes  byte masks of different sizes (the buffer and desc table of ep24_ray24) -> packed rows, one wave per (mask, row);
//               the run kernels then have one input form
//   count       one wave per (mask, 32-column word): strips of 64 rows, one lane per row, each lane loads its row's word once;
//               t = word ^ (the row above's word, by a lane shift; the column before's last row for row 0) has one bit per
//               transition, __ballot of bit b is column b's 64-row segment and __popcll counts it; lane b keeps column b's count
//   scan        one wave per mask turns its W column counts into their exclusive prefix and leaves runs = transitions + 1; one
//               workgroup then scans the N run counts in index order into offsets[N + 1].  No atomics: a position is a sum
//   emit        count's traversal again: a transition of column x at row y goes to offsets[n] + prefix[x] + (the column's
//               transitions in earlier strips) + (the set bits below its lane in the ballot)
//   counts      ends -> run lengths: one thread per run takes the difference to the end before it; a mask's last run ends at H * W
// Integer work only: no floating point, no atomics.  Every mask word is read once by count and once by emit (plus one or two words per
// (mask, word column) for the row-0 carry).
#include "wave_scan.h"

namespace {

// mask n of a batch: uniform (tab == NULL: N masks of H x W behind each other, column counts at n * W) or by table
// tab[n][4] int64 = {first word in bits, H, W, first entry in the column table}
struct MaskRef {
    long word0, col0;
    int H, W;
    bool ok;
};

__device__ __forceinline__ MaskRef mask_ref(const long long* tab, long n, int H, int W) {
    MaskRef m;
    if (tab) {
        const long long* t = tab + n * 4;
        const long long h = t[1], w = t[2];
        m.ok = h > 0 && w > 0 && h <= 0x7FFFFFFFLL && w <= 0x7FFFFFFFLL && h * w <= 0x7FFFFFFFLL && t[0] >= 0 && t[3] >= 0;
        m.word0 = t[0];
        m.col0 = t[3];
        m.H = (int)h;
        m.W = (int)w;
    } else {
        m.ok = true;
        m.word0 = n * H * ((W + 31) >> 5);
        m.col0 = n * W;
        m.H = H;
        m.W = W;
    }
    return m;
}

// the transitions of rows y0 .. y0 + 63 (this lane: row y0 + lane) in the 32 columns of word column xw: bit b set iff pixel
// (32 xw + b, y) differs from the pixel before it.  carry = the word "above row y0"; it leaves as the word of row y0 + 63.
__device__ __forceinline__ uint32_t strip_transitions(const uint32_t* col, int WW, int H, int y0, int lane, uint32_t valid,
                                                      uint32_t& carry) {
    const int y = y0 + lane;
    const uint32_t cur = y < H ? col[(long)y * WW] : 0u;
    uint32_t prev = __shfl_up(cur, 1, 64);
    if (lane == 0) prev = carry;
    carry = __shfl(cur, 63, 64);
    return y < H ? (cur ^ prev) & valid : 0u;
}

// the word above row 0: the last row shifted by one column, with the last row's bit 31 of the word column before
__device__ __forceinline__ uint32_t first_carry(const uint32_t* col, int WW, int H, int xw) {
    const uint32_t* last = col + (long)(H - 1) * WW;
    return (last[0] << 1) | (xw > 0 ? last[-1] >> 31 : 0u);
}

__device__ __forceinline__ uint32_t valid_columns(int W, int xw) {
    const int k = W - 32 * xw;
    return k >= 32 ? 0xFFFFFFFFu : (1u << k) - 1u;
}

__global__ __launch_bounds__(256) void rle_pack_bytes_kernel(const uint8_t* masks, long total, const long long* desc,
                                                             const long long* tab, long n0, uint32_t* bits) {
    const int lane = threadIdx.x & 63;
    const long n = n0 + blockIdx.y;
    const MaskRef m = mask_ref(tab, n, 0, 0);
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!m.ok || y >= m.H) return;                             // whole waves leave together
    const long long* d = desc + n * 6;
    const long off = d[0], ld = d[5];
    if (off < 0 || ld < m.W || off + (long)(m.H - 1) * ld + m.W > total) return;
    const uint8_t* s = masks + off + (long)y * ld;
    const int WW = (m.W + 31) >> 5;
    uint32_t* row = bits + m.word0 + (long)y * WW;
    for (int x0 = 0; x0 < m.W; x0 += 64) {
        const int x = x0 + lane;
        const unsigned long long b = __ballot(x < m.W && s[x] != 0);
        const int w = (x0 >> 5) + lane;                       // lanes 0 and 1 store the two words
        if (lane < 2 && w < WW) row[w] = (uint32_t)(b >> (32 * lane));
    }
}

// grid (ceil(max WW / 4), masks of this launch): one wave per (mask, word column)
__global__ __launch_bounds__(256) void rle_count_kernel(const uint32_t* bits, const long long* tab, long n0, int H, int W,
                                                        int32_t* colcnt) {
    const int lane = threadIdx.x & 63;
    const MaskRef m = mask_ref(tab, n0 + blockIdx.y, H, W);
    const int xw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int WW = (m.W + 31) >> 5;
    if (!m.ok || xw >= WW) return;
    const uint32_t* col = bits + m.word0 + xw;
    const uint32_t valid = valid_columns(m.W, xw);
    uint32_t carry = first_carry(col, WW, m.H, xw);
    int cnt = 0;                                              // lane b: the transitions of column 32 xw + b
    for (int y0 = 0; y0 < m.H; y0 += 64) {
        const uint32_t t = strip_transitions(col, WW, m.H, y0, lane, valid, carry);
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const int c = __popcll(__ballot((t >> b) & 1u));
            if (lane == b) cnt += c;
        }
    }
    const int x = 32 * xw + lane;
    if (lane < 32 && x < m.W) colcnt[m.col0 + x] = cnt;
}

// one wave per mask: column counts -> their exclusive prefix, in place; offsets[n + 1] = the mask's number of runs
__global__ __launch_bounds__(256) void rle_colscan_kernel(int32_t* colcnt, const long long* tab, long N, int H, int W,
                                                          long long* offsets) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const MaskRef m = mask_ref(tab, n, H, W);
    int carry = 0;
    if (m.ok) {
        int32_t* c = colcnt + m.col0;
        for (int x0 = 0; x0 < m.W; x0 += 64) {
            const int x = x0 + lane;
            const int v = x < m.W ? c[x] : 0;
            const int inc = wave_incl_sum(v, lane);
            if (x < m.W) c[x] = carry + inc - v;
            carry += __shfl(inc, 63, 64);
        }
    }
    if (lane == 0) offsets[n + 1] = (long long)carry + 1;
}

// one workgroup: offsets[0] = 0, offsets[1 .. N] -> their inclusive prefix in index order
__global__ __launch_bounds__(1024) void rle_offsets_kernel(long long* offsets, long N) {
    __shared__ long long wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) offsets[0] = 0;
    long long carry = 0;
    for (long i0 = 0; i0 < N; i0 += 1024) {
        const long i = i0 + tid;
        const long long inc = wave_incl_sum(i < N ? offsets[1 + i] : 0LL, lane);
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        long long before = 0, all = 0;
        for (int k = 0; k < 16; ++k) {
            if (k < wv) before += wsum[k];
            all += wsum[k];
        }
        if (i < N) offsets[1 + i] = carry + before + inc;
        carry += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rle_emit_kernel(const uint32_t* bits, const long long* tab, long n0, int H, int W,
                                                       const int32_t* colprefix, const long long* offsets, int32_t* ends, long cap) {
    const int lane = threadIdx.x & 63;
    const long n = n0 + blockIdx.y;
    const MaskRef m = mask_ref(tab, n, H, W);
    const int xw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int WW = (m.W + 31) >> 5;
    if (!m.ok || xw >= WW) return;
    const uint32_t* col = bits + m.word0 + xw;
    const uint32_t valid = valid_columns(m.W, xw);
    uint32_t carry = first_carry(col, WW, m.H, xw);
    const long lo = offsets[n];
    long hi = offsets[n + 1] - 1;                             // the mask's transitions live in [lo, hi); hi holds its last run
    if (hi > cap) hi = cap;
    const int x = 32 * xw + lane;
    long base = 0;                                            // lane b: where column 32 xw + b's next transition goes
    if (lane < 32 && x < m.W) base = lo + colprefix[m.col0 + x];
    for (int y0 = 0; y0 < m.H; y0 += 64) {
        const uint32_t t = strip_transitions(col, WW, m.H, y0, lane, valid, carry);
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const unsigned long long seg = __ballot((t >> b) & 1u);
            if (!seg) continue;                               // the same for the whole wave
            const long at = __shfl(base, b, 64) + __popcll(seg & ((1ull << lane) - 1ull));
            if (((t >> b) & 1u) && at >= lo && at < hi) ends[at] = (32 * xw + b) * m.H + y0 + lane;
            if (lane == b) base += __popcll(seg);
        }
    }
}

__global__ __launch_bounds__(256) void rle_counts_kernel(const int32_t* ends, const long long* offsets, const long long* tab, long N,
                                                         int H, int W, long total, int32_t* counts) {
    const long end_all = offsets[N] < total ? offsets[N] : total;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < end_all; i += (long)gridDim.x * 256) {
        long lo = 0, hi = N - 1;                              // the last mask with offsets[n] <= i (every mask has a run)
        while (lo < hi) {
            const long mid = (lo + hi + 1) >> 1;
            if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const MaskRef m = mask_ref(tab, lo, H, W);
        const long first = offsets[lo], last = offsets[lo + 1] - 1;
        const int end = i < last ? ends[i] : (m.ok ? m.H * m.W : 0);       // a skipped table row: one run of 0
        const int before = i > first ? ends[i - 1] : 0;
        counts[i] = end - before;
    }
}

}  // namespace

#define S_ (hipStream_t) stream

// tab == NULL: H and W are every mask's; otherwise they are the largest H and W of the table (they size the grids)
static bool rle_shape_ok(int N, int H, int W) { return N >= 0 && H > 0 && W > 0 && (long)H * W <= 0x7FFFFFFFL; }

extern "C" int ep24_rle_pack_bytes(const uint8_t* masks, int64_t total, const int64_t* desc, const int64_t* tab, int N, int max_h,
                                   uint32_t* bits, void* stream) {
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(N > 0 && max_h > 0 && total > 0, EP24_E_UNSUPPORTED, "rle_pack_bytes: N=%d max_h=%d total=%ld", N, max_h, (long)total);
    EP24_REQUIRE(masks && desc && tab && bits, EP24_E_ARG, "rle_pack_bytes: null pointer");
    for (long n0 = 0; n0 < N; n0 += 65535) {
        const unsigned ny = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
        hipLaunchKernelGGL(rle_pack_bytes_kernel, dim3((max_h + 3) / 4, ny), dim3(256), 0, S_, masks, (long)total, (const long long*)desc,
                           (const long long*)tab, n0, bits);
    }
    EP24_LAUNCH_CHECK("ep24_rle_pack_bytes");
    return EP24_OK;
}

extern "C" int ep24_rle_count(const uint32_t* bits, const int64_t* tab, int N, int H, int W, int32_t* colcnt, void* stream) {
    EP24_REQUIRE(rle_shape_ok(N, H, W), EP24_E_UNSUPPORTED, "rle_count: N=%d H=%d W=%d (N >= 0, H, W > 0, H * W < 2^31)", N, H, W);
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(bits && colcnt, EP24_E_ARG, "rle_count: null pointer");
    const int WW = (W + 31) / 32;
    for (long n0 = 0; n0 < N; n0 += 65535) {
        const unsigned ny = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
        hipLaunchKernelGGL(rle_count_kernel, dim3((WW + 3) / 4, ny), dim3(256), 0, S_, bits, (const long long*)tab, n0, H, W, colcnt);
    }
    EP24_LAUNCH_CHECK("ep24_rle_count");
    return EP24_OK;
}

extern "C" int ep24_rle_scan(int32_t* colcnt, const int64_t* tab, int N, int H, int W, int64_t* offsets, void* stream) {
    EP24_REQUIRE(rle_shape_ok(N, H, W), EP24_E_UNSUPPORTED, "rle_scan: N=%d H=%d W=%d (N >= 0, H, W > 0, H * W < 2^31)", N, H, W);
    EP24_REQUIRE(offsets && (colcnt || N == 0), EP24_E_ARG, "rle_scan: null pointer");
    if (N > 0)
        hipLaunchKernelGGL(rle_colscan_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, S_, colcnt, (const long long*)tab, (long)N, H, W,
                           (long long*)offsets);
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(1024), 0, S_, (long long*)offsets, (long)N);
    EP24_LAUNCH_CHECK("ep24_rle_scan");
    return EP24_OK;
}

extern "C" int ep24_rle_emit(const uint32_t* bits, const int64_t* tab, int N, int H, int W, const int32_t* colprefix,
                             const int64_t* offsets, int32_t* ends, int64_t cap, void* stream) {
    EP24_REQUIRE(rle_shape_ok(N, H, W) && cap >= 0, EP24_E_UNSUPPORTED, "rle_emit: N=%d H=%d W=%d (N >= 0, H, W > 0, H * W < 2^31)", N, H,
                 W);
    if (N == 0 || cap == 0) return EP24_OK;
    EP24_REQUIRE(bits && colprefix && offsets && ends, EP24_E_ARG, "rle_emit: null pointer");
    const int WW = (W + 31) / 32;
    for (long n0 = 0; n0 < N; n0 += 65535) {
        const unsigned ny = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
        hipLaunchKernelGGL(rle_emit_kernel, dim3((WW + 3) / 4, ny), dim3(256), 0, S_, bits, (const long long*)tab, n0, H, W, colprefix,
                           (const long long*)offsets, ends, (long)cap);
    }
    EP24_LAUNCH_CHECK("ep24_rle_emit");
    return EP24_OK;
}

extern "C" int ep24_rle_counts(const int32_t* ends, const int64_t* offsets, const int64_t* tab, int N, int H, int W, int64_t total,
                               int32_t* counts, void* stream) {
    EP24_REQUIRE(rle_shape_ok(N, H, W) && total >= 0, EP24_E_UNSUPPORTED, "rle_counts: N=%d H=%d W=%d (N >= 0, H, W > 0, H * W < 2^31)", N,
                 H, W);
    if (N == 0 || total == 0) return EP24_OK;
    EP24_REQUIRE(ends && offsets && counts, EP24_E_ARG, "rle_counts: null pointer");
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(rle_counts_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, S_, ends,
                       (const long long*)offsets, (const long long*)tab, (long)N, H, W, (long)total, counts);
    EP24_LAUNCH_CHECK("ep24_rle_counts");
    return EP24_OK;
}
