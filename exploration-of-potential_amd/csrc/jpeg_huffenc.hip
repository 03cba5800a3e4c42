// ep24 - the Huffman stage of the baseline JPEG encoder on the GPU ("JPEG encode: Huffman stage on the GPU"): the int16
// coefficients ep24_jpeg_fdct leaves on the device -> the entropy-coded bytes of every image, restart markers included, back to back
// in one compact buffer.  The block walk, the bit emitter and the byte stuffing are csrc/jpeg_huffenc_core.h, the text the host
// emulation (ep24jpeg_encode_emulate) runs too.
//
//   ep24_jpeg_huffenc_count
//     jpeg_huffenc_count_kernel   one thread per block in SCAN order (MCU by MCU, Y's h x v blocks, Cb, Cr) over the whole batch: the
//                                 workgroup's 256 blocks are fetched into LDS in 16-byte rows, a thread walks its block there in
//                                 zig-zag order and stores its bit count; the DC predictor is read from the coefficients, so blocks are
//                                 independent.  Out-of-range input ORs a bit into the image's status word.
//     jpeg_huffenc_scan_kernel    one workgroup per image: the counts become inclusive sums in place (wave shuffles, a sum across the 16
//                                 waves, a carry across rounds of 1 024), then one thread per restart segment takes the segment's bits
//                                 as a difference of two sums and the words in front of it by the same scan: every segment starts on a
//                                 fresh 32-bit word.
//     jpeg_huffenc_base_kernel    one workgroup: the exclusive sum of the images' word counts, n + 1 values - what the host reads to
//                                 size the word buffer
//   ep24_jpeg_huffenc_emit
//     jpeg_huffenc_emit_kernel    the count kernel's shape; a thread shifts its block's codes into big-endian words from its position
//                                 on.  A word it fills entirely is a plain store; its first and last word may be shared with the
//                                 neighbours and are ORed into the zeroed buffer (atomicOr: order-independent).  The last block of a
//                                 segment fills the segment's last byte with ones.
//     jpeg_huffenc_bytes_kernel   one workgroup per image, an item per 16 words: the bytes the image's scan takes with FF 00 stuffing and
//                                 RSTn markers, summed
//     jpeg_huffenc_base_kernel    their exclusive sum: offsets[n + 1]
//     jpeg_huffenc_stuff_kernel   one workgroup per image: counts per item again, their exclusive sum with a carry across rounds, and
//                                 every item writes its bytes at its offset
//
// Integers only.  Every index made from a descriptor is checked against the buffers before anything is read (ep24huffenc_load); a
// descriptor that does not fit sets the image's status to EP24_E_ARG and nothing of the image is read or written.  A word or byte
// index at or beyond the capacity is dropped and sets EP24HUFFENC_BAD_STORE.
#include "common.h"
#include "jpeg_huffenc_core.h"
#include "wave_scan.h"

namespace {

#define ENC_TILE 256          // blocks per workgroup of the count and the emit kernel
#define ENC_BLK_I16 66        // int16 between two blocks in LDS: 33 dwords, so the 64 lanes of a wave read 64 different banks
#define ENC_SCAN 1024         // threads of the per-image kernels

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// v of this thread and of every thread below it in the workgroup; ws: one value per wave
__device__ __forceinline__ long long block_incl_sum(long long v, long long* ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_incl_sum(v, lane);
    if (lane == 63) ws[w] = v;
    __syncthreads();
    long long add = 0;
    for (int i = 0; i < w; ++i) add += ws[i];
    __syncthreads();
    return v + add;
}

// the image of block g of the batch: the largest i in [0, n) with desc[i][0] <= g
__device__ __forceinline__ int find_image(const int64_t* desc, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long)mid * EP24HUFFENC_DESC] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// what the count and the emit kernel do first: the tables in LDS, the thread's block found, the workgroup's blocks fetched.
// -> the thread has a block (its image's descriptor fits).  Ends behind a barrier.
__device__ __forceinline__ bool enc_prologue(const short* __restrict__ coef, int64_t ncoef, const int64_t* __restrict__ desc, int n,
                                             int64_t total_blocks, int64_t nseg_total, uint32_t* tab, int16_t* blk, int64_t* at_s, int& img,
                                             ep24huffenc_image& I, ep24huffenc_where& W, int64_t& q) {
    const int tid = threadIdx.x;
    for (int i = tid; i < EP24HUFFENC_TABLE; i += ENC_TILE) tab[i] = 0;
    __syncthreads();
    for (int i = tid; i < EP24HUFFENC_ENTRIES; i += ENC_TILE) ep24huffenc_fill(tab, i);       // every symbol has its own entry
    const int64_t g = (int64_t)blockIdx.x * ENC_TILE + tid;
    bool on = g < total_blocks;
    img = 0, q = 0;
    if (on) {
        img = find_image(desc, n, g);
        on = ep24huffenc_load(desc + (long)img * EP24HUFFENC_DESC, total_blocks, nseg_total, ncoef, I);
        q = g - I.first_block;
        on = on && q >= 0 && q < I.nblocks;
        if (on) W = ep24huffenc_locate(I, q);
    }
    at_s[tid] = on ? W.at : -1;
    __syncthreads();
    for (int i = tid; i < ENC_TILE * 8; i += ENC_TILE) {      // 8 lanes fetch the 8 rows of a block
        const int b = i >> 3, r = i & 7;
        const int64_t at = at_s[b];
        if (at < 0) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(coef + at + 8 * r);
        uint32_t* d = reinterpret_cast<uint32_t*>(blk + b * ENC_BLK_I16) + 4 * r;
        d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
    }
    __syncthreads();
    return on;
}

__global__ __launch_bounds__(ENC_TILE) void jpeg_huffenc_count_kernel(const short* __restrict__ coef, int64_t ncoef,
                                                                      const int64_t* __restrict__ desc, int n, int64_t total_blocks,
                                                                      int64_t nseg_total, int64_t* __restrict__ pos, int* __restrict__ status) {
    __shared__ uint32_t tab[EP24HUFFENC_TABLE];
    __shared__ int16_t blk[ENC_TILE * ENC_BLK_I16];
    __shared__ int64_t at_s[ENC_TILE];
    int img;
    int64_t q;
    ep24huffenc_image I;
    ep24huffenc_where W;
    const bool on = enc_prologue(coef, ncoef, desc, n, total_blocks, nseg_total, tab, blk, at_s, img, I, W, q);
    const int64_t g = (int64_t)blockIdx.x * ENC_TILE + threadIdx.x;
    if (g >= total_blocks) return;
    ep24huffenc_counter cnt = {0};
    if (on) {
        const int pred = W.pred_at < 0 ? 0 : coef[W.pred_at];
        const int bad = ep24huffenc_block(blk + threadIdx.x * ENC_BLK_I16, pred, tab + EP24HUFFENC_DC(W.chroma), tab + EP24HUFFENC_AC(W.chroma), cnt);
        if (bad) atomicOr(status + img, bad);
    }
    pos[g] = cnt.bits;
}

__global__ __launch_bounds__(ENC_SCAN) void jpeg_huffenc_scan_kernel(const int64_t* __restrict__ desc, int64_t total_blocks, int64_t nseg_total,
                                                                     int64_t ncoef, int64_t* pos, int64_t* __restrict__ seg,
                                                                     int64_t* __restrict__ image_words, int* __restrict__ status) {
    __shared__ long long ws[ENC_SCAN / 64];
    __shared__ long long carry;
    const int img = blockIdx.x, tid = threadIdx.x;
    ep24huffenc_image I;
    if (!ep24huffenc_load(desc + (long)img * EP24HUFFENC_DESC, total_blocks, nseg_total, ncoef, I)) {      // uniform: the whole workgroup leaves
        if (tid == 0) status[img] = EP24_E_ARG, image_words[img] = 0;
        return;
    }
    int64_t* p = pos + I.first_block;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t t0 = 0; t0 < I.nblocks; t0 += ENC_SCAN) {
        const int64_t q = t0 + tid;
        const long long v = q < I.nblocks ? p[q] : 0;
        const long long incl = block_incl_sum(v, ws) + carry;
        if (q < I.nblocks) p[q] = incl;
        __syncthreads();                                  // carry is read above
        if (tid == ENC_SCAN - 1) carry = incl;
        __syncthreads();
    }
    // the sums are in memory for the whole workgroup behind the barrier; a segment's bits are a difference of two of them
    if (tid == 0) carry = 0;
    __syncthreads();
    const int64_t per = (int64_t)I.ri * I.bpm;
    for (int64_t s0 = 0; s0 < I.nseg; s0 += ENC_SCAN) {
        const int64_t s = s0 + tid;
        long long bits = 0, w = 0;
        if (s < I.nseg) {
            const int64_t b = s * per, e = (per && (s + 1) * per < I.nblocks) ? (s + 1) * per : I.nblocks;
            bits = p[e - 1] - (b ? p[b - 1] : 0);
            w = (bits + 31) >> 5;
        }
        const long long incl = block_incl_sum(w, ws) + carry;
        if (s < I.nseg) {
            seg[2 * (I.first_seg + s)] = incl - w;
            seg[2 * (I.first_seg + s) + 1] = bits;
        }
        __syncthreads();
        if (tid == ENC_SCAN - 1) carry = incl;
        __syncthreads();
    }
    if (tid == 0) image_words[img] = carry;
}

// out[i] = in[0] + .. + in[i - 1] for i in 0 .. n: one workgroup
__global__ __launch_bounds__(ENC_SCAN) void jpeg_huffenc_base_kernel(const int64_t* __restrict__ in, int n, int64_t* __restrict__ out) {
    __shared__ long long ws[ENC_SCAN / 64];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += ENC_SCAN) {
        const int i = t0 + tid;
        const long long v = i < n ? in[i] : 0;
        const long long incl = block_incl_sum(v, ws) + carry;
        if (i < n) out[i] = incl - v;
        __syncthreads();
        if (tid == ENC_SCAN - 1) carry = incl;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}

struct WordStore {
    uint32_t* words;
    int64_t cap;
    int dropped;
    __device__ __forceinline__ void operator()(int64_t w, uint32_t v, bool owned) {
        if (w < 0 || w >= cap) {
            dropped = 1;
            return;
        }
        if (owned) words[w] = v;
        else if (v) atomicOr(words + w, v);
    }
};

__global__ __launch_bounds__(ENC_TILE) void jpeg_huffenc_emit_kernel(const short* __restrict__ coef, int64_t ncoef,
                                                                     const int64_t* __restrict__ desc, int n, int64_t total_blocks,
                                                                     int64_t nseg_total, const int64_t* __restrict__ pos,
                                                                     const int64_t* __restrict__ seg, const int64_t* __restrict__ word_base,
                                                                     uint32_t* __restrict__ words, int64_t nwords, int* __restrict__ status) {
    __shared__ uint32_t tab[EP24HUFFENC_TABLE];
    __shared__ int16_t blk[ENC_TILE * ENC_BLK_I16];
    __shared__ int64_t at_s[ENC_TILE];
    int img;
    int64_t q;
    ep24huffenc_image I;
    ep24huffenc_where W;
    if (!enc_prologue(coef, ncoef, desc, n, total_blocks, nseg_total, tab, blk, at_s, img, I, W, q)) return;
    const int64_t* p = pos + I.first_block;
    const int64_t in_seg = (q ? p[q - 1] : 0) - (W.seg_block ? p[W.seg_block - 1] : 0);
    const int64_t first_word = word_base[img] + seg[2 * (I.first_seg + W.seg)];
    WordStore st = {words, nwords, 0};
    if (in_seg < 0 || first_word < 0 || first_word > nwords) {      // sums that are not the count kernel's: nothing is written
        atomicOr(status + img, EP24HUFFENC_BAD_STORE);
        return;
    }
    ep24huffenc_emitter<WordStore> em;
    em.begin(32 * first_word + in_seg, &st);
    const int pred = W.pred_at < 0 ? 0 : coef[W.pred_at];
    ep24huffenc_block(blk + threadIdx.x * ENC_BLK_I16, pred, tab + EP24HUFFENC_DC(W.chroma), tab + EP24HUFFENC_AC(W.chroma), em);
    if (W.seg_last) em.pad();
    em.finish();
    if (st.dropped) atomicOr(status + img, EP24HUFFENC_BAD_STORE);
}

// the image's words and segment rows; false: the descriptor or the word range does not fit (nothing of the image is read)
__device__ __forceinline__ bool stuff_image(const int64_t* __restrict__ desc, int img, int64_t total_blocks, int64_t nseg_total, int64_t ncoef,
                                            const int64_t* __restrict__ word_base, int64_t nwords, ep24huffenc_image& I, int64_t& w_first,
                                            int64_t& nw) {
    if (!ep24huffenc_load(desc + (long)img * EP24HUFFENC_DESC, total_blocks, nseg_total, ncoef, I)) return false;
    w_first = word_base[img];
    nw = word_base[img + 1] - w_first;
    return w_first >= 0 && nw >= 0 && w_first + nw <= nwords;
}

__device__ __forceinline__ long long chunk_bytes(const uint32_t* words, const int64_t* seg, int64_t nseg, int64_t c, int64_t nw) {
    ep24huffenc_byte_counter bc = {0};
    const int64_t w0 = c * EP24HUFFENC_CHUNK_WORDS, w1 = w0 + EP24HUFFENC_CHUNK_WORDS;
    ep24huffenc_chunk(words, seg, nseg, w0, w1 < nw ? w1 : nw, bc);
    return bc.n;
}

__global__ __launch_bounds__(ENC_SCAN) void jpeg_huffenc_bytes_kernel(const int64_t* __restrict__ desc, int64_t total_blocks, int64_t nseg_total,
                                                                      int64_t ncoef, const int64_t* __restrict__ seg,
                                                                      const int64_t* __restrict__ word_base, const uint32_t* __restrict__ words,
                                                                      int64_t nwords, int64_t* __restrict__ image_bytes) {
    __shared__ long long ws[ENC_SCAN / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    ep24huffenc_image I;
    int64_t w_first, nw;
    if (!stuff_image(desc, img, total_blocks, nseg_total, ncoef, word_base, nwords, I, w_first, nw)) {      // uniform
        if (tid == 0) image_bytes[img] = 0;
        return;
    }
    const int64_t nchunks = (nw + EP24HUFFENC_CHUNK_WORDS - 1) / EP24HUFFENC_CHUNK_WORDS;
    long long mine = 0;
    for (int64_t c = tid; c < nchunks; c += ENC_SCAN) mine += chunk_bytes(words + w_first, seg + 2 * I.first_seg, I.nseg, c, nw);
    const long long incl = block_incl_sum(mine, ws);
    if (tid == ENC_SCAN - 1) image_bytes[img] = incl;
}

__global__ __launch_bounds__(ENC_SCAN) void jpeg_huffenc_stuff_kernel(const int64_t* __restrict__ desc, int64_t total_blocks, int64_t nseg_total,
                                                                      int64_t ncoef, const int64_t* __restrict__ seg,
                                                                      const int64_t* __restrict__ word_base, const uint32_t* __restrict__ words,
                                                                      int64_t nwords, const int64_t* __restrict__ offsets,
                                                                      uint8_t* __restrict__ out, int64_t out_bytes, int* __restrict__ status) {
    __shared__ long long ws[ENC_SCAN / 64];
    __shared__ long long carry;
    const int img = blockIdx.x, tid = threadIdx.x;
    ep24huffenc_image I;
    int64_t w_first, nw;
    if (!stuff_image(desc, img, total_blocks, nseg_total, ncoef, word_base, nwords, I, w_first, nw)) return;      // uniform
    const int64_t nchunks = (nw + EP24HUFFENC_CHUNK_WORDS - 1) / EP24HUFFENC_CHUNK_WORDS;
    const uint32_t* wd = words + w_first;
    const int64_t* sg = seg + 2 * I.first_seg;
    // the image's bytes end where the next image's begin: a count that disagrees with the bytes kernel's cannot reach into them
    const int64_t lo = offsets[img], hi = offsets[img + 1] < out_bytes ? offsets[img + 1] : out_bytes;
    if (tid == 0) carry = 0;
    __syncthreads();
    int dropped = 0;
    for (int64_t c0 = 0; c0 < nchunks; c0 += ENC_SCAN) {
        const int64_t c = c0 + tid;
        const long long mine = c < nchunks ? chunk_bytes(wd, sg, I.nseg, c, nw) : 0;
        const long long incl = block_incl_sum(mine, ws) + carry;
        if (c < nchunks && lo >= 0) {
            ep24huffenc_byte_writer bw = {out, lo + (incl - mine), hi, 0};
            const int64_t w0 = c * EP24HUFFENC_CHUNK_WORDS, w1 = w0 + EP24HUFFENC_CHUNK_WORDS;
            ep24huffenc_chunk(wd, sg, I.nseg, w0, w1 < nw ? w1 : nw, bw);
            dropped |= bw.dropped;
        }
        __syncthreads();                                  // carry is read above
        if (tid == ENC_SCAN - 1) carry = incl;
        __syncthreads();
    }
    if (dropped || lo < 0) atomicOr(status + img, EP24HUFFENC_BAD_STORE);
}

}  // namespace

extern "C" int ep24_jpeg_huffenc_count(const void* coef, int64_t ncoef, const int64_t* image_desc, int n, int64_t total_blocks,
                                       int64_t total_segments, int64_t* positions, int64_t* segments, int64_t* image_words, int64_t* word_base,
                                       int32_t* status, void* stream) {
    EP24_REQUIRE(n >= 0 && ncoef >= 0 && total_blocks >= 0 && total_segments >= 0, EP24_E_ARG, "jpeg_huffenc_count: negative count");
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(coef && image_desc && positions && segments && image_words && word_base && status, EP24_E_ARG, "jpeg_huffenc_count: null pointer");
    EP24_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)image_desc % 8 == 0 && (uintptr_t)positions % 8 == 0 && (uintptr_t)segments % 8 == 0 &&
                     (uintptr_t)image_words % 8 == 0 && (uintptr_t)word_base % 8 == 0 && (uintptr_t)status % 4 == 0,
                 EP24_E_ARG, "jpeg_huffenc_count: coefficients must be 16-byte aligned, descriptors and sums 8-byte, status words 4-byte");
    EP24_REQUIRE(total_blocks <= (int64_t)ENC_TILE * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_huffenc_count: %lld blocks are beyond one launch",
                 (long long)total_blocks);
    hipStream_t s = (hipStream_t)stream;
    if (total_blocks > 0) {
        const unsigned groups = (unsigned)((total_blocks + ENC_TILE - 1) / ENC_TILE);
        hipLaunchKernelGGL(jpeg_huffenc_count_kernel, dim3(groups), dim3(ENC_TILE), 0, s, (const short*)coef, ncoef, image_desc, n, total_blocks,
                           total_segments, positions, (int*)status);
        EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_count");
    }
    hipLaunchKernelGGL(jpeg_huffenc_scan_kernel, dim3((unsigned)n), dim3(ENC_SCAN), 0, s, image_desc, total_blocks, total_segments, ncoef, positions,
                       segments, image_words, (int*)status);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_count (scan)");
    hipLaunchKernelGGL(jpeg_huffenc_base_kernel, dim3(1), dim3(ENC_SCAN), 0, s, (const int64_t*)image_words, n, word_base);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_count (base)");
    return EP24_OK;
}

extern "C" int ep24_jpeg_huffenc_emit(const void* coef, int64_t ncoef, const int64_t* image_desc, int n, int64_t total_blocks,
                                      int64_t total_segments, const int64_t* positions, const int64_t* segments, const int64_t* word_base,
                                      uint32_t* words, int64_t nwords, int64_t* image_bytes, int64_t* offsets, uint8_t* out, int64_t out_bytes,
                                      int32_t* status, void* stream) {
    EP24_REQUIRE(n >= 0 && ncoef >= 0 && total_blocks >= 0 && total_segments >= 0 && nwords >= 0 && out_bytes >= 0, EP24_E_ARG,
                 "jpeg_huffenc_emit: negative count");
    if (n == 0) return EP24_OK;
    EP24_REQUIRE(coef && image_desc && positions && segments && word_base && words && image_bytes && offsets && out && status, EP24_E_ARG,
                 "jpeg_huffenc_emit: null pointer");
    EP24_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)image_desc % 8 == 0 && (uintptr_t)positions % 8 == 0 && (uintptr_t)segments % 8 == 0 &&
                     (uintptr_t)word_base % 8 == 0 && (uintptr_t)image_bytes % 8 == 0 && (uintptr_t)offsets % 8 == 0 && (uintptr_t)words % 4 == 0 &&
                     (uintptr_t)status % 4 == 0,
                 EP24_E_ARG, "jpeg_huffenc_emit: coefficients must be 16-byte aligned, descriptors and sums 8-byte, words and status words 4-byte");
    EP24_REQUIRE(total_blocks <= (int64_t)ENC_TILE * 0x7fffffff, EP24_E_UNSUPPORTED, "jpeg_huffenc_emit: %lld blocks are beyond one launch",
                 (long long)total_blocks);
    hipStream_t s = (hipStream_t)stream;
    if (total_blocks > 0) {
        const unsigned groups = (unsigned)((total_blocks + ENC_TILE - 1) / ENC_TILE);
        hipLaunchKernelGGL(jpeg_huffenc_emit_kernel, dim3(groups), dim3(ENC_TILE), 0, s, (const short*)coef, ncoef, image_desc, n, total_blocks,
                           total_segments, positions, segments, word_base, words, nwords, (int*)status);
        EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_emit");
    }
    hipLaunchKernelGGL(jpeg_huffenc_bytes_kernel, dim3((unsigned)n), dim3(ENC_SCAN), 0, s, image_desc, total_blocks, total_segments, ncoef, segments,
                       word_base, (const uint32_t*)words, nwords, image_bytes);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_emit (bytes)");
    hipLaunchKernelGGL(jpeg_huffenc_base_kernel, dim3(1), dim3(ENC_SCAN), 0, s, (const int64_t*)image_bytes, n, offsets);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_emit (base)");
    hipLaunchKernelGGL(jpeg_huffenc_stuff_kernel, dim3((unsigned)n), dim3(ENC_SCAN), 0, s, image_desc, total_blocks, total_segments, ncoef, segments,
                       word_base, (const uint32_t*)words, nwords, (const int64_t*)offsets, out, out_bytes, (int*)status);
    EP24_LAUNCH_CHECK("ep24_jpeg_huffenc_emit (stuff)");
    return EP24_OK;
}
