// ep24 - the Huffman stage of the baseline JPEG decoder on the GPU ("JPEG decode: Huffman stage on the GPU"): the scan
// bytes of a batch of files -> int16 coefficients in ep24_jpeg_idct's layout, by self-synchronising subsequence decoders
// (Weissenberger & Schmidt).  The state machine is csrc/jpeg_huff_core.h, the text the host emulation runs too.
//
//   jpeg_huff_kernel   ONE WORKGROUP PER IMAGE - no workgroup ever waits for another.  The image's restart segments are cut into
//                      subsequences of S bytes; the workgroup walks them in tiles of one subsequence per thread:
//                        setup    the six Huffman tables of the image built in LDS from the file's specifications: the lengths by one
//                                 thread per table, the 6 x 512 look-ahead entries by the whole workgroup
//                        round 0  every thread decodes its subsequence from its start: known for a segment's first subsequence and for
//                                 thread 0 (the verified end of the tile in front), speculative (byte boundary, k = 0, block 0) otherwise
//                        round r  a thread whose predecessor's end state differs from the start it used decodes again from that state
//                        stop     after a round in which no end state changed (__syncthreads_or), at the latest after as many rounds
//                                 as the tile has threads: from the anchored first thread, by induction, that is the serial decode
//                        write    exclusive scan of the blocks begun (restarted per segment, carried across tiles), then every thread
//                                 decodes once more from its verified start and stores the coefficients, the DC as its DIFFERENCE
//                      Speculation is never an error: an invalid code costs the guessing thread one bit and it goes on (why it does
//                      not stop there: jpeg_huff_core.h, ep24huff_run).  Errors come from the write pass: one int32 status word per
//                      image, written once by thread 0.
//   jpeg_dc_kernel     one workgroup per (image, component): DC differences -> values, a prefix sum in scan order in int32 that starts
//                      from zero at every restart segment; a value outside int16 sets the image's status word.
//
// No floating point, no atomics, vector stores only.  A store that a descriptor would send outside the image's coefficients is dropped
// (ep24huff_where); a descriptor that does not fit its buffers ends the workgroup with status EP24_E_ARG before anything is read.
#include "common.h"
#include "jpeg_huff_core.h"
#include "wave_scan.h"

namespace {

#define HUFF_MAX_TILE 1024
#define HUFF_DESC 16          // int64 per image descriptor row
#define HUFF_SEG 6            // int32 per segment row
#define HUFF_SPEC 276         // bytes per table specification: 16 counts, 256 symbols, int32 count of symbols
#define HUFF_E_DATA (-4)      // EP24JPEG_E_DATA of include/ep24_jpeg.h

// v of this thread and of every thread below it in the workgroup; ws: one int per wave
__device__ __forceinline__ int block_incl_sum(int v, int* ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_incl_sum(v, lane);
    if (lane == 63) ws[w] = v;
    __syncthreads();
    int add = 0;
    for (int i = 0; i < w; ++i) add += ws[i];
    __syncthreads();
    return v + add;
}

struct HuffDesc {
    long long scan_off, scan_len, seg_first, nseg, nsub, coef_off, ncoef;
    int ncomp, h0, v0, mcus_x, mcus_y, ri;
};

// false: the row does not fit the buffers (nothing of it may be used)
__device__ __forceinline__ bool load_desc(const long long* __restrict__ row, long long nbytes, long long nseg_total, long long ncoef_total,
                                          HuffDesc& D) {
    D.scan_off = row[0], D.scan_len = row[1], D.seg_first = row[2], D.nseg = row[3], D.nsub = row[4], D.coef_off = row[5], D.ncoef = row[6];
    D.ncomp = (int)row[7], D.h0 = (int)row[8], D.v0 = (int)row[9], D.mcus_x = (int)row[10], D.mcus_y = (int)row[11], D.ri = (int)row[12];
    if (D.scan_off < 0 || D.scan_len < 0 || D.scan_len >= (1LL << 28) || D.scan_off + D.scan_len > nbytes) return false;
    if (D.seg_first < 0 || D.nseg < 1 || D.seg_first + D.nseg > nseg_total) return false;
    if (D.coef_off < 0 || D.ncoef < 0 || D.coef_off + D.ncoef > ncoef_total) return false;
    if ((D.ncomp != 1 && D.ncomp != 3) || D.h0 < 1 || D.h0 > 2 || D.v0 < 1 || D.v0 > 2 || D.mcus_x < 1 || D.mcus_y < 1 || D.mcus_x > 1024 ||
        D.mcus_y > 1024 || D.ri < 0 || D.nsub < 0 || D.nsub > (1LL << 30))
        return false;
    return true;
}

__global__ __launch_bounds__(HUFF_MAX_TILE) void jpeg_huff_kernel(const uint8_t* __restrict__ bytes, long long nbytes,
                                                                  const long long* __restrict__ desc, const int* __restrict__ segs,
                                                                  long long nseg_total, const uint8_t* __restrict__ specs, int S,
                                                                  short* __restrict__ coef, long long ncoef_total, int* __restrict__ status) {
    __shared__ ep24huff_table tabs[6];
    __shared__ uint32_t end_pos[HUFF_MAX_TILE], end_kj[HUFF_MAX_TILE];
    __shared__ int excl_s[HUFF_MAX_TILE];
    __shared__ int wsum[HUFF_MAX_TILE / 64];
    __shared__ uint32_t carry_pos, carry_kj;
    __shared__ int carry_blocks;
    const int img = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    HuffDesc D;
    if (!load_desc(desc + (long long)img * HUFF_DESC, nbytes, nseg_total, ncoef_total, D)) {       // uniform: the whole workgroup leaves
        if (tid == 0) status[img] = EP24_E_ARG;
        return;
    }
    if (tid < 6) {
        const uint8_t* sp = specs + ((long long)img * 6 + tid) * HUFF_SPEC;
        const int nsym = (int)sp[272] | ((int)sp[273] << 8) | ((int)sp[274] << 16) | ((int)sp[275] << 24);
        ep24huff_build_lengths(tabs[tid], sp, sp + 16, nsym);
    }
    __syncthreads();
    for (int i = tid; i < 6 << EP24HUFF_LOOK; i += T)     // the 6 x 512 look-ahead entries, spread over the workgroup
        tabs[i >> EP24HUFF_LOOK].look[i & ((1 << EP24HUFF_LOOK) - 1)] = ep24huff_look_entry(tabs[i >> EP24HUFF_LOOK], i & ((1 << EP24HUFF_LOOK) - 1));
    if (tid == 0) carry_pos = 0, carry_kj = 0, carry_blocks = 0;
    ep24huff_image im;
    im.d = bytes + D.scan_off;
    im.tabs = tabs;
    im.ncomp = D.ncomp, im.h0 = D.h0, im.v0 = D.v0, im.mcus_x = D.mcus_x;
    im.bpm = D.ncomp == 1 ? 1 : D.h0 * D.v0 + 2;
    if (D.ncomp == 1) im.h0 = im.v0 = 1;
    const long long mcus = (long long)D.mcus_x * D.mcus_y;
    im.off1 = 64 * mcus * im.h0 * im.v0;
    im.off2 = im.off1 + 64 * mcus;
    im.ncoef = D.ncoef;
    short* out = coef + D.coef_off;
    const int* sg_rows = segs + D.seg_first * HUFF_SEG;
    const int nseg = (int)D.nseg;
    int err = 0;
    __syncthreads();

    for (long long t0 = 0; t0 < D.nsub; t0 += T) {
        const long long g = t0 + tid;
        const bool active = g < D.nsub;
        ep24huff_segment sg = {0, 0, 0, 0};
        ep24huff_state start = {EP24HUFF_PARKED, 0}, e = {EP24HUFF_PARKED, 0};
        uint32_t bound = 0;
        long long seg_sub0 = 0;
        bool anchored = true, last = false;
        int nb = 0;
        if (active) {
            int lo = 0, hi = nseg - 1;                    // the last segment whose first subsequence is at or below g
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((long long)(uint32_t)sg_rows[mid * HUFF_SEG + 4] <= g) lo = mid;
                else hi = mid - 1;
            }
            const int* r = sg_rows + lo * HUFF_SEG;
            long long off = (uint32_t)r[0], len = (uint32_t)r[1];
            if (off > D.scan_len) off = D.scan_len;       // a row that lies cannot send a read outside the scan
            if (off + len > D.scan_len) len = D.scan_len - off;
            sg.off = (uint32_t)off, sg.end = (uint32_t)(off + len);
            sg.first_mcu = r[2] < 0 ? 0 : r[2];
            const long long expect = (long long)(r[3] < 0 ? 0 : r[3]) * im.bpm;
            sg.expect = (int32_t)(expect > 0x7fffffffLL ? 0x7fffffffLL : expect);
            seg_sub0 = (uint32_t)r[4];
            long long li = g - seg_sub0;
            const long long nsub = max((len + S - 1) / S, 1LL);
            if (li < 0) li = 0;
            if (li >= nsub) li = nsub - 1;
            anchored = li == 0;
            last = li + 1 == nsub;
            const long long b = off + (li + 1) * S;
            bound = (uint32_t)(b < sg.end ? b : sg.end);
            if (anchored) start = ep24huff_state{sg.off * 8u, 0};
            else if (tid == 0) start = ep24huff_state{carry_pos, carry_kj};
            else start = ep24huff_state{ep24huff_spec_start(im.d, sg.off, sg.off + (uint32_t)(li * S)), 0};
            ep24huff_run<false>(im, sg, start, bound, &e, &nb, nullptr, 0, false);
        }
        end_pos[tid] = e.pos, end_kj[tid] = e.kj;
        __syncthreads();
        for (int r = 1; r <= T; ++r) {                    // bounded by the tile; leaves after a round that changed no end state
            const bool follows = active && tid > 0 && !anchored;
            ep24huff_state want = start;
            if (follows) want = ep24huff_state{end_pos[tid - 1], end_kj[tid - 1]};
            __syncthreads();                              // every read of this round in front of every write
            int changed = 0;
            if (follows && (want.pos != start.pos || want.kj != start.kj)) {
                start = want;
                const ep24huff_state was = e;
                ep24huff_run<false>(im, sg, start, bound, &e, &nb, nullptr, 0, false);
                changed = e.pos != was.pos || e.kj != was.kj;
                end_pos[tid] = e.pos, end_kj[tid] = e.kj;
            }
            if (!__syncthreads_or(changed)) break;
        }
        // the blocks begun in front of this subsequence within its segment
        const int incl = block_incl_sum(active ? nb : 0, wsum);
        excl_s[tid] = incl - nb;
        __syncthreads();
        int excl = 0;
        if (active) {
            const long long fs = seg_sub0 > t0 ? seg_sub0 : t0;         // in [t0, g] unless the segment rows lie: clamped
            excl = excl_s[tid] - excl_s[(int)min(fs - t0, (long long)tid)] + (seg_sub0 < t0 ? carry_blocks : 0);
            if (ep24huff_run<true>(im, sg, start, bound, nullptr, nullptr, (int16_t*)out, excl, last)) err = 1;
        }
        __syncthreads();                                  // carry_* are read above
        if (active && (g + 1 == D.nsub || tid == T - 1)) carry_pos = e.pos, carry_kj = e.kj, carry_blocks = excl + nb;
        __syncthreads();
    }
    const int any = __syncthreads_or(err);
    if (tid == 0) status[img] = any ? HUFF_E_DATA : 0;
}

__global__ __launch_bounds__(HUFF_MAX_TILE) void jpeg_dc_kernel(const long long* __restrict__ desc, short* __restrict__ coef,
                                                                long long ncoef_total, int* __restrict__ status) {
    __shared__ int excl_s[HUFF_MAX_TILE];
    __shared__ int wsum[HUFF_MAX_TILE / 64];
    __shared__ int carry;
    const int img = blockIdx.x / 3, c = blockIdx.x % 3, tid = threadIdx.x, T = blockDim.x;
    HuffDesc D;
    // the Huffman launch has said so in the status word where the row does not fit; the scan's bytes are not read here
    if (!load_desc(desc + (long long)img * HUFF_DESC, 1LL << 62, 1LL << 62, ncoef_total, D) || c >= D.ncomp) return;
    const int hc = (c == 0 && D.ncomp == 3) ? D.h0 : 1, vc = (c == 0 && D.ncomp == 3) ? D.v0 : 1, hv = hc * vc;
    const long long mcus = (long long)D.mcus_x * D.mcus_y;
    const long long lum = D.ncomp == 3 ? (long long)D.h0 * D.v0 : 1;
    const long long comp_off = c == 0 ? 0 : 64 * mcus * lum + (c == 2 ? 64 * mcus : 0);
    const long long nq = mcus * hv, bw = (long long)D.mcus_x * hc;
    short* out = coef + D.coef_off;
    if (tid == 0) carry = 0;
    int bad = 0;
    __syncthreads();
    for (long long t0 = 0; t0 < nq; t0 += T) {
        const long long q = t0 + tid;
        const bool active = q < nq;
        long long at = -1, head = 0;
        int d = 0;
        if (active) {
            const long long m = q / hv;
            const int r = (int)(q - m * hv);
            const long long my = m / D.mcus_x, mx = m - my * D.mcus_x;
            const int by = r / hc, bx = r - by * hc;
            at = comp_off + ((my * vc + by) * bw + (mx * hc + bx)) * 64;
            if (at < 0 || at >= D.ncoef) at = -1;
            if (at >= 0) d = out[at];
            head = D.ri ? (m / D.ri) * D.ri * hv : 0;      // the first block of this block's restart segment, in scan order
        }
        const int incl = block_incl_sum(d, wsum);
        excl_s[tid] = incl - d;
        __syncthreads();
        int v = 0;
        if (active) {
            v = head >= t0 ? incl - excl_s[(int)(head - t0)] : (int)((unsigned)carry + (unsigned)incl);      // wraps on garbage, defined
            if (v < -32768 || v > 32767) bad = 1;
            if (at >= 0) out[at] = (short)v;
        }
        __syncthreads();                                  // carry is read above
        if (tid == T - 1) carry = v;
        __syncthreads();
    }
    const int any = __syncthreads_or(bad);
    if (tid == 0 && any) status[img] = HUFF_E_DATA;       // only ever sets it: the Huffman launch wrote the word first
}

}  // namespace

extern "C" int ep24_jpeg_huffman(const uint8_t* bytes, int64_t nbytes, const int64_t* image_desc, int n, const int32_t* segments,
                                 int64_t nseg, const uint8_t* table_specs, int subseq_bytes, int tile, void* coef, int64_t ncoef,
                                 int32_t* status, void* stream) {
    EP24_REQUIRE(n >= 0 && nbytes >= 0 && nseg >= 0 && ncoef >= 0, EP24_E_ARG, "jpeg_huffman: negative count");
    const int S = subseq_bytes;
    EP24_REQUIRE(S == 16 || S == 32 || S == 64 || S == 128 || S == 256, EP24_E_ARG, "jpeg_huffman: subsequences of %d bytes (16, 32, 64, 128 or 256)", S);
    EP24_REQUIRE(tile >= 64 && tile <= HUFF_MAX_TILE && tile % 64 == 0, EP24_E_ARG, "jpeg_huffman: a tile of %d threads (a multiple of 64 up to %d)",
                 tile, HUFF_MAX_TILE);
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(bytes && image_desc && segments && table_specs && coef && status, EP24_E_ARG, "jpeg_huffman: null pointer");
    EP24_REQUIRE((uintptr_t)image_desc % 8 == 0 && (uintptr_t)segments % 4 == 0 && (uintptr_t)coef % 2 == 0 && (uintptr_t)status % 4 == 0, EP24_E_ARG,
                 "jpeg_huffman: misaligned descriptors, segment rows, coefficients or status words");
    hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)n), dim3((unsigned)tile), 0, (hipStream_t)stream, bytes, (long long)nbytes,
                       (const long long*)image_desc, (const int*)segments, (long long)nseg, table_specs, S, (short*)coef, (long long)ncoef, (int*)status);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffman");
    return EP24_OK;
}

extern "C" int ep24_jpeg_dc(const int64_t* image_desc, int n, void* coef, int64_t ncoef, int32_t* status, void* stream) {
    EP24_REQUIRE(n >= 0 && ncoef >= 0, EP24_E_ARG, "jpeg_dc: negative count");
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(n <= 0x7fffffff / 3, EP24_E_UNSUPPORTED, "jpeg_dc: %d images are beyond one launch", n);
    EP24_REQUIRE(image_desc && coef && status, EP24_E_ARG, "jpeg_dc: null pointer");
    EP24_REQUIRE((uintptr_t)image_desc % 8 == 0 && (uintptr_t)coef % 2 == 0 && (uintptr_t)status % 4 == 0, EP24_E_ARG,
                 "jpeg_dc: misaligned descriptors, coefficients or status words");
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3u * (unsigned)n), dim3(HUFF_MAX_TILE), 0, (hipStream_t)stream, (const long long*)image_desc, (short*)coef,
                       (long long)ncoef, (int*)status);
    EP24_LAUNCH_CHECK("ep24_jpeg_dc");
    return EP24_OK;
}
