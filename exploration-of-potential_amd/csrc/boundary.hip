// ep24 - boundary bands of packed instance masks for Boundary IoU (include/ep24.h section E7; DESIGN.md section 7;
// ep24.masks.boundary, ep24.segmeval.SegmEvaluator(iou_type="boundary")).
//
//   boundary(M, d) = M & ~erode(M, d), erode = the (2d + 1) x (2d + 1) square minimum with everything outside the image not set.
//
//   mask_boundary     a workgroup takes one mask and work items = (band of rows, tile of word columns) of it.  Per item:
//                       1. the band's words are loaded into registers, 16 loads per thread in flight together, and kept there for step
//                          3 (a band without a set bit is written as zeros and done); with dv rows above and below they also go to
//                          LDS (a tile of a row too wide for that reads its neighbours from global memory instead: the same cache
//                          lines).  Then every word of those rows is eroded HORIZONTALLY in registers and stored to a second LDS
//                          array.  The window of 2 dh + 1 bits is a run of dh + 1 bits to the right AND one to the left; a run of
//                          k <= 32 bits over two neighbouring words is a 64-bit value ANDed with itself shifted by 1, 2, 4, ...
//                          (doubling) and by the rest, five shifts without a branch; a radius of 32 or more walks whole words
//                          (32-bit runs) first.  Words beyond the row are zero; an empty word is done at once.
//                       2. van Herk / Gil-Werman over the rows in LDS: rows in blocks of 2 dv + 1, a running AND from each block's
//                          first row down (prefix, over the copy of step 1) and from its last row up (suffix, in place), sixteen
//                          rows per step so that a thread's LDS reads are in flight together.
//                       3. the vertical window of output row o is suffix[o] & prefix[o + 2 dv]; out = the word of step 1 & ~that.
//                     Nine LDS word accesses per staged word and its neighbours' reads, whatever d is.  dh = min(d, W) and
//                     dv = min(d, H): a window that long always leaves the image.  Rows above and below the image count as zero.
//                     Two LDS arrays of BD_CAP words = 64 KiB: two workgroups per CU.  The band is as tall as the arrays allow; a row
//                     too wide for 2 dv + 1 rows of it is cut into tiles of word columns (a tile needs no halo in LDS: the horizontal
//                     pass reads its neighbours from global memory).  2 dv + 1 > BD_CAP (an image more than 8 192 rows tall with a
//                     radius to match) takes the direct form: every output word walks its own 2 dv + 1 rows.
//   segm_iou_min      iou[i] = min(iou[i], other[i])
//
// Integer work only, no atomics; every output word is written exactly once.
#include "common.h"

namespace {

constexpr int BD_CAP = 8192;          // words per LDS array
constexpr int BD_NT = 512;            // threads of a workgroup (measured: 256 and 1 024 threads, and 4 096-word arrays, were slower)
constexpr int BD_CH = 16;             // rows per step of the running ANDs
constexpr int BD_RG = BD_CAP / BD_NT;   // words of a band per thread

// i / n for 0 <= i < 2^13 and 1 <= n <= 2^13 by one multiplication: with m = ceil(2^32 / n), m * n - 2^32 < n and i * n < 2^32
struct BdDiv {
    uint32_t m;
    int n;
};
__host__ __device__ inline BdDiv bd_div(int n) { return BdDiv{0xFFFFFFFFu / (uint32_t)n + 1u, n}; }      // n == 1: unused
__host__ __device__ inline int bd_quot(int i, const BdDiv& d) {
    return d.n == 1 ? i : (int)(((unsigned long long)(uint32_t)i * d.m) >> 32);
}

struct BdPlan {
    int R, CW, nb, nct;               // rows per band (0: the direct form), word columns per tile, bands, tiles
};

// The split of one mask into work items; the host sizes the grid with the same function.  32-bit unsigned arithmetic throughout:
// every wave of the kernel computes it, and a 64-bit division is hundreds of instructions.
__host__ __device__ inline BdPlan bd_plan(int H, int WW, int dv) {
    BdPlan p;
    const uint32_t h = (uint32_t)H, ww = (uint32_t)WW, halo = 2u * (uint32_t)dv, cap = (uint32_t)BD_CAP;
    if (halo + 1 > cap) {
        p.R = 0; p.CW = WW; p.nb = (int)(((unsigned long long)h * ww + 4095) / 4096); p.nct = 1;
        return p;
    }
    // a tile as wide as leaves room for a band at least as tall as its halo (or the image)
    const uint32_t tall = halo > 16 ? halo : 16, want = halo + (h < tall ? h : tall);
    uint32_t cw = cap / want;
    cw = cw < 1 ? 1 : (cw > ww ? ww : cw);
    const uint32_t nct = (ww + cw - 1) / cw;
    p.nct = (int)nct;
    p.CW = (int)((ww + nct - 1) / nct);
    const uint32_t cap_rows = cap / (uint32_t)p.CW - halo;    // >= 1: CW * (halo + 1) <= BD_CAP
    const uint32_t rmax = cap_rows < h ? cap_rows : h;
    const uint32_t nb = (h - 1) / rmax + 1;
    p.nb = (int)nb;
    p.R = (int)((h - 1) / nb + 1);
    return p;
}

// A run of k <= 32 bits by doubling without a branch: five shifts s_i = min(length so far, k - length so far) grow a window of 1 bit
// to min(32, k) bits (1, 2, 4, 8, 16 for k = 32; zeros once k is reached).
struct BdSteps {
    int s[5];
};
__device__ __forceinline__ BdSteps bd_steps(int k) {
    BdSteps t;
    int len = 1;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        t.s[i] = min(len, k - len);
        len += t.s[i];
    }
    return t;
}
// bit x (0 .. 31) = bits x .. x + k - 1 of the 64-bit value (b : a) are all set
__device__ __forceinline__ uint32_t run_up(uint32_t a, uint32_t b, const BdSteps& st) {
    unsigned long long t = (unsigned long long)a | ((unsigned long long)b << 32);
#pragma unroll
    for (int i = 0; i < 5; ++i) t &= t >> st.s[i];
    return (uint32_t)t;
}
// bit x of a = bits x - k + 1 .. x all set, the bits below a's bit 0 being those of prev
__device__ __forceinline__ uint32_t run_down(uint32_t prev, uint32_t a, const BdSteps& st) {
    unsigned long long t = (unsigned long long)prev | ((unsigned long long)a << 32);
#pragma unroll
    for (int i = 0; i < 5; ++i) t &= t << st.s[i];
    return (uint32_t)(t >> 32);
}

// word w of the row p[0 .. WW) eroded by dh = 32 q + r bits to either side; s32 and sr are the steps of 32 and of r + 1 bits.  The
// word and its two neighbours are read together; an empty word is done (whole waves skip the rest over empty rows).
__device__ __forceinline__ uint32_t erode_row_word(const uint32_t* p, int WW, int w, int q, const BdSteps& s32, const BdSteps& sr) {
    const uint32_t cur = p[w], next = w + 1 < WW ? p[w + 1] : 0u, prev = w >= 1 ? p[w - 1] : 0u;
    if (cur == 0) return 0;
    uint32_t acc = cur & run_up(cur, next, q ? s32 : sr) & run_down(prev, cur, q ? s32 : sr);
    uint32_t lo = next;                                       // further words to the right: (lo, hi) = (w + j, w + j + 1)
    for (int j = 1; j <= q && acc; ++j) {
        const uint32_t hi = w + j + 1 < WW ? p[w + j + 1] : 0u;
        acc &= run_up(lo, hi, j < q ? s32 : sr);
        lo = hi;
    }
    uint32_t hi = prev;                                       // and to the left: (lo, hi) = (w - j - 1, w - j)
    for (int j = 1; j <= q && acc; ++j) {
        lo = w - j - 1 >= 0 ? p[w - j - 1] : 0u;
        acc &= run_down(lo, hi, j < q ? s32 : sr);
        hi = lo;
    }
    return acc;
}

// grid (work items per mask, masks of this launch)
__global__ __launch_bounds__(BD_NT) void mask_boundary_kernel(const uint32_t* bits, const long long* tab, long n0, int uH, int uW, int ud,
                                                            uint32_t* out) {
    __shared__ uint32_t suf[BD_CAP];
    __shared__ uint32_t pre[BD_CAP];
    const long n = n0 + blockIdx.y;
    long long word0, H64, W64, d64;
    if (tab) {
        const long long* t = tab + n * 4;
        word0 = t[0]; H64 = t[1]; W64 = t[2]; d64 = t[3];
    } else {
        H64 = uH; W64 = uW; d64 = ud;
        word0 = n * (long long)uH * ((uW + 31) >> 5);
    }
    if (word0 < 0 || H64 <= 0 || W64 <= 0 || H64 * W64 >= (1LL << 31) || d64 < 1) return;      // the whole workgroup leaves
    const int H = (int)H64, W = (int)W64, WW = (W + 31) >> 5;
    const int dh = (int)(d64 < W ? d64 : W), dv = (int)(d64 < H ? d64 : H);
    const uint32_t* src = bits + word0;
    uint32_t* dst = out + word0;
    const int tid = threadIdx.x;
    const BdPlan pl = bd_plan(H, WW, dv);
    const int q = dh >> 5;
    const BdSteps s32 = bd_steps(32), sr = bd_steps((dh & 31) + 1);
    if (pl.R == 0) {                                          // the direct form
        const long cells = (long)H * WW;
        for (long i = (long)blockIdx.x * BD_NT + tid; i < cells; i += (long)gridDim.x * BD_NT) {
            const int y = (int)(i / WW), w = (int)(i - (long)y * WW);
            const uint32_t m = src[i];
            uint32_t e = (y - dv < 0 || y + dv >= H) ? 0u : m;
            for (int yy = y - dv; yy <= y + dv && e; ++yy) e &= erode_row_word(src + (long)yy * WW, WW, w, q, s32, sr);
            dst[i] = m & ~e;
        }
        return;
    }
    const int B = 2 * dv + 1;
    const BdDiv divB = bd_div(B);
    for (int item = blockIdx.x; item < pl.nb * pl.nct; item += gridDim.x) {      // the trip count is the workgroup's
        const int band = item / pl.nct, tile = item - band * pl.nct;
        const int y0 = band * pl.R, R = min(pl.R, H - y0);
        const int c0 = tile * pl.CW, CW = min(pl.CW, WW - c0);
        if (R <= 0 || CW <= 0) continue;                      // uniform: bands and tiles are rounded up
        const bool whole = pl.nct == 1;                       // then CW == WW, c0 == 0
        const BdDiv divC = bd_div(CW);
        const int nst = (R + 2 * dv) * CW, nband = R * CW, off = dv * CW;        // staged words (<= BD_CAP), the band's, the band's first
        // 1. the band's own words: BD_RG loads per thread in flight together, kept in registers for step 4 (lanes beyond the band
        //    repeat its last word); whole rows go to LDS with the halo rows, for the neighbours' reads of step 2
        uint32_t rawv[BD_RG];
#pragma unroll
        for (int m = 0; m < BD_RG; ++m) {
            const int i = min(tid + BD_NT * m, nband - 1);
            const int o = bd_quot(i, divC);
            rawv[m] = src[(long)(y0 + o) * WW + c0 + (i - o * CW)];
        }
        uint32_t any = 0u;                                    // an empty band has an empty boundary, whatever lies above and below
#pragma unroll
        for (int m = 0; m < BD_RG; ++m) any |= rawv[m];
        if (!__syncthreads_or(any != 0u)) {                   // (also the barrier between the last item's reads of LDS and this one's writes)
#pragma unroll
            for (int m = 0; m < BD_RG; ++m) {
                const int i = tid + BD_NT * m;
                if (i < nband) {
                    const int o = bd_quot(i, divC);
                    dst[(long)(y0 + o) * WW + c0 + (i - o * CW)] = 0u;
                }
            }
            continue;
        }
        if (whole) {
#pragma unroll
            for (int m = 0; m < BD_RG; ++m)
                if (tid + BD_NT * m < nband) pre[off + tid + BD_NT * m] = rawv[m];
            const long first = (long)(y0 - dv) * WW, cells = (long)H * WW;       // staged word j is word first + j of the mask
#pragma unroll 4
            for (int h = tid; h < 2 * off; h += BD_NT) {
                const int j = h < off ? h : h + nband;
                const long g = first + j;
                const bool in = g >= 0 && g < cells;
                const uint32_t v = src[in ? g : 0];
                pre[j] = in ? v : 0u;
            }
            __syncthreads();
        }
        // 2. horizontal
        for (int j = tid; j < nst; j += BD_NT) {
            const int r = bd_quot(j, divC), c = j - r * CW, y = y0 - dv + r;
            uint32_t v = 0u;
            if (y >= 0 && y < H) v = whole ? erode_row_word(pre + r * WW, WW, c, q, s32, sr) : erode_row_word(src + (long)y * WW, WW, c0 + c, q, s32, sr);
            suf[j] = v;
        }
        __syncthreads();
        // 3. running ANDs over the blocks of B rows
        const int nblk = ((R + 2 * dv) + B - 1) / B;
        for (int i = tid; i < nblk * CW; i += BD_NT) {
            const int blk = bd_quot(i, divC), c = i - blk * CW;
            const int r0 = blk * B, r1 = min(r0 + B, R + 2 * dv);
            uint32_t v[BD_CH], acc = ~0u;                    // BD_CH rows at a time: their reads are in flight together
            for (int r = r0; r < r1; r += BD_CH) {
#pragma unroll
                for (int k = 0; k < BD_CH; ++k) v[k] = r + k < r1 ? suf[(r + k) * CW + c] : ~0u;
#pragma unroll
                for (int k = 0; k < BD_CH; ++k) {
                    acc &= v[k];
                    if (r + k < r1) pre[(r + k) * CW + c] = acc;
                }
            }
            acc = ~0u;
            for (int r = r1 - 1; r >= r0; r -= BD_CH) {
#pragma unroll
                for (int k = 0; k < BD_CH; ++k) v[k] = r - k >= r0 ? suf[(r - k) * CW + c] : ~0u;
#pragma unroll
                for (int k = 0; k < BD_CH; ++k) {
                    acc &= v[k];
                    if (r - k >= r0) suf[(r - k) * CW + c] = acc;
                }
            }
        }
        __syncthreads();
        // 4. the vertical window of output row o and the band
#pragma unroll
        for (int m = 0; m < BD_RG; ++m) {
            const int i = tid + BD_NT * m;
            if (i < nband) {
                const int o = bd_quot(i, divC), c = i - o * CW;
                uint32_t e = suf[i];                          // rows o .. the end of o's block
                if (o - bd_quot(o, divB) * B) e &= pre[(o + B - 1) * CW + c];    // the next block's first rows, down to o + 2 dv
                dst[(long)(y0 + o) * WW + c0 + c] = rawv[m] & ~e;
            }
        }
    }
}

__global__ __launch_bounds__(256) void segm_iou_min_kernel(double* iou, const double* other, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double a = iou[i], b = other[i];
        iou[i] = b < a ? b : a;
    }
}

}  // namespace

#define S_ (hipStream_t) stream

extern "C" int ep24_mask_boundary(const uint32_t* bits, const int64_t* tab, int N, int H, int W, int d, uint32_t* out, void* stream) {
    EP24_REQUIRE(N >= 0, EP24_E_UNSUPPORTED, "mask_boundary: N=%d", N);
    if (N == 0) return EP24_OK;
    EP24_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1LL << 31), EP24_E_UNSUPPORTED, "mask_boundary: H=%d W=%d (H, W > 0, H * W < 2^31)", H,
                 W);
    EP24_REQUIRE(tab || d >= 1, EP24_E_UNSUPPORTED, "mask_boundary: d=%d (d >= 1)", d);
    EP24_REQUIRE(bits && out, EP24_E_ARG, "mask_boundary: null pointer");
    EP24_REQUIRE(out != bits, EP24_E_ARG, "mask_boundary: out == bits (the kernel reads its neighbours' words)");
    const int WW = (W + 31) / 32;
    // One radius for all: the exact number of work items.  A table: its radii are on the device; half as many again as a mask of the
    // largest size has at no halo (a workgroup walks the items beyond the grid).
    BdPlan pl = bd_plan(H, WW, tab ? 0 : (d < H ? d : H));
    long gx = (long)pl.nb * pl.nct;
    if (tab) gx += gx / 2;
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    for (long n0 = 0; n0 < N; n0 += 65535) {
        const unsigned ny = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
        hipLaunchKernelGGL(mask_boundary_kernel, dim3((unsigned)gx, ny), dim3(BD_NT), 0, S_, bits, (const long long*)tab, n0, H, W, d, out);
    }
    EP24_LAUNCH_CHECK("ep24_mask_boundary");
    return EP24_OK;
}

extern "C" int ep24_segm_iou_min(double* iou, const double* other, int64_t n, void* stream) {
    EP24_REQUIRE(n >= 0, EP24_E_UNSUPPORTED, "segm_iou_min: n=%lld", (long long)n);
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(iou && other, EP24_E_ARG, "segm_iou_min: null pointer");
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(segm_iou_min_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, S_, iou, other, (long long)n);
    EP24_LAUNCH_CHECK("ep24_segm_iou_min");
    return EP24_OK;
}
