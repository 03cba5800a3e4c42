// ep24 - the baseline JPEG Huffman ENCODER, shared by the host (jpeg_host.cpp: ep24jpeg_entropy_encode's tables and
// ep24jpeg_encode_emulate, with threads as loops) and the device (jpeg_huffenc.hip).  One text, so that what the sanitizer build of
// jpeg_huffenc_check.cpp walks through is what the kernels run.  Plain C++ and integers only; every function is EP24_HD.
//
// The device encoder has no serial bit writer: every block's codes are COUNTED, the counts are summed into bit positions, and every
// block then EMITS its codes at its position into a zeroed buffer of 32-bit big-endian words, in any order.  The count and the emit
// pass call ONE routine (ep24huffenc_block) with different sinks, so their bit counts cannot disagree.  A restart segment starts on
// a fresh word; the unstuffed words are then turned into the file's bytes (FF 00 stuffing, RSTn markers) chunk by chunk by
// ep24huffenc_chunk, again one routine for the counting and the writing pass.
#pragma once
#include <stdint.h>

#include "jpeg_huff_core.h"       // EP24_HD, ep24huff_zigzag

// the routines that fill a struct through a reference: inlined into the kernel, so that the struct lives in registers
#if defined(__HIPCC__)
#define EP24_HDF __host__ __device__ __forceinline__
#else
#define EP24_HDF inline
#endif

// ---- the typical Huffman tables of Annex K.3: code counts per length 1 .. 16 and the symbols; t = 0 luminance, 1 chrominance ----

EP24_HD int ep24huffenc_dc_bits(int t, int i) {
    const uint8_t b[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    return b[t & 1][i & 15];
}

EP24_HD int ep24huffenc_dc_val(int, int k) { return k; }        // 0 .. 11 in both tables
#define EP24HUFFENC_DC_VALS 12

EP24_HD int ep24huffenc_ac_bits(int t, int i) {
    const uint8_t b[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    return b[t & 1][i & 15];
}

#define EP24HUFFENC_AC_VALS 162
EP24_HD int ep24huffenc_ac_val(int t, int k) {
    const uint8_t v[2][EP24HUFFENC_AC_VALS] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
    return v[t & 1][k < EP24HUFFENC_AC_VALS ? k : 0];
}

// ---- the code tables: one uint32 per symbol, code | length << 16 (0: the symbol has no code) ----

// [0, 16) DC luminance, [16, 32) DC chrominance, [32, 288) AC luminance, [288, 544) AC chrominance: 2 176 bytes
#define EP24HUFFENC_TABLE 544
#define EP24HUFFENC_DC(t) (16 * (t))
#define EP24HUFFENC_AC(t) (32 + 256 * (t))

// the k-th symbol of a table (in the order of its DHT segment) and its canonical code, on its own: any thread can make any entry.
// ac: 0 / 1; t: 0 luminance, 1 chrominance.  -> code | length << 16, *sym the symbol; 0 when the table has no k-th symbol
EP24_HD uint32_t ep24huffenc_entry(int ac, int t, int k, int* sym) {
    uint32_t code = 0;
    int cum = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = ac ? ep24huffenc_ac_bits(t, l - 1) : ep24huffenc_dc_bits(t, l - 1);
        if (k < cum + cnt) {
            *sym = ac ? ep24huffenc_ac_val(t, k) : ep24huffenc_dc_val(t, k);
            return (code + (uint32_t)(k - cum)) | ((uint32_t)l << 16);
        }
        code = (code + (uint32_t)cnt) << 1;
        cum += cnt;
    }
    *sym = 0;
    return 0;
}

// entry i of the 2 x 12 + 2 x 162 = 348 that a table holds -> where it goes in tab (the caller has zeroed tab)
#define EP24HUFFENC_ENTRIES (2 * EP24HUFFENC_DC_VALS + 2 * EP24HUFFENC_AC_VALS)
EP24_HD void ep24huffenc_fill(uint32_t* tab, int i) {
    int sym;
    if (i < 2 * EP24HUFFENC_DC_VALS) {
        const int t = i / EP24HUFFENC_DC_VALS;
        const uint32_t e = ep24huffenc_entry(0, t, i - t * EP24HUFFENC_DC_VALS, &sym);
        tab[EP24HUFFENC_DC(t) + sym] = e;
    } else if (i < EP24HUFFENC_ENTRIES) {
        i -= 2 * EP24HUFFENC_DC_VALS;
        const int t = i / EP24HUFFENC_AC_VALS;
        const uint32_t e = ep24huffenc_entry(1, t, i - t * EP24HUFFENC_AC_VALS, &sym);
        tab[EP24HUFFENC_AC(t) + sym] = e;
    }
}

// ---- one block ----

#define EP24HUFFENC_BAD_DC 1      // status bits: a DC difference outside +-2047,
#define EP24HUFFENC_BAD_AC 2      // an AC coefficient outside +-1023,
#define EP24HUFFENC_BAD_STORE 4   // a store outside the word or the byte buffer was dropped

EP24_HD int ep24huffenc_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }      // bits of a >= 0

// Hands every (code, length) pair of a block to sink.put, in the order of ep24jpeg_entropy_encode's inner loop: the DC size code with
// the value bits behind it in ONE pair (at most 9 + 11 bits), ZRL while a run is above 15, the run/size code with its value bits in one
// pair (at most 16 + 10), EOB only when a run is pending at the end.  A negative value is coded as v - 1, masked to its size.  blk: 64
// coefficients in natural order; pred: the DC of the previous block of the component in scan order (0 at the start of a restart
// segment); dct / act: the component's 16 DC and 256 AC entries.  -> 0, or EP24HUFFENC_BAD_DC / _AC: nothing further of the block is
// coded, in either pass.  A pair is at most 27 bits; a block at most 20 + 63 * 26 = 1 658.
template <class Sink>
EP24_HD int ep24huffenc_block(const int16_t* blk, int pred, const uint32_t* dct, const uint32_t* act, Sink& sink) {
    const int diff = (int)blk[0] - pred;
    if (diff < -2047 || diff > 2047) return EP24HUFFENC_BAD_DC;
    int s = ep24huffenc_size(diff < 0 ? -diff : diff);
    uint32_t e = dct[s];
    sink.put(((e & 0xFFFFu) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), (int)(e >> 16) + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[ep24huff_zigzag(k)];
        if (v == 0) {
            ++run;
            continue;
        }
        if (v < -1023 || v > 1023) return EP24HUFFENC_BAD_AC;
        while (run > 15) {
            e = act[0xF0];
            sink.put(e & 0xFFFFu, (int)(e >> 16));
            run -= 16;
        }
        s = ep24huffenc_size(v < 0 ? -v : v);
        e = act[(run << 4) | s];
        sink.put(((e & 0xFFFFu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), (int)(e >> 16) + s);
        run = 0;
    }
    if (run) {
        e = act[0];
        sink.put(e & 0xFFFFu, (int)(e >> 16));
    }
    return 0;
}

struct ep24huffenc_counter {
    int bits;
    EP24_HD void put(uint32_t, int len) { bits += len; }
};

// Shifts pairs into 32-bit big-endian words from bit position `pos` of the word buffer on.  store(word index, value, owned): owned =
// the block wrote all 32 bits of the word (a plain store); otherwise the word may be shared with the neighbours and the value is ORed
// into the zeroed buffer - integer OR is order-independent.  finish() hands out the last, partial word.
template <class Store>
struct ep24huffenc_emitter {
    uint64_t acc;
    int n;              // bits held in acc (below 32 between calls), the `pos & 31` leading zeros of the first word included
    int64_t w;          // index of the word acc fills
    bool shared;        // the word acc fills began in front of this block
    Store* store;
    EP24_HD void begin(int64_t pos, Store* st) {
        acc = 0, n = (int)(pos & 31), w = pos >> 5, shared = n != 0, store = st;
    }
    EP24_HD void put(uint32_t code, int len) {      // len <= 27
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            (*store)(w, (uint32_t)(acc >> (n - 32)), !shared);
            shared = false;
            ++w;
            n -= 32;
        }
    }
    // behind the last block of a restart segment: its last byte is filled with ones (a segment starts on a word, so n & 7 is the bit
    // within the byte)
    EP24_HD void pad() {
        const int p = (8 - (n & 7)) & 7;
        if (p) put((1u << p) - 1, p);
    }
    EP24_HD void finish() {
        if (n > 0) (*store)(w, (uint32_t)(acc << (32 - n)), false);
    }
};

// ---- where a block lies ----

// An image as the kernels see it: row i and row i + 1 of image_desc[n + 1][16] int64 = {0 first block of the image in scan order
// (cumulative over the batch, image 0: 0), 1 first restart segment of the image (cumulative), 2 components (1 or 3), 3 / 4 luma
// sampling h / v (1 or 2; chroma is 1 x 1), 5 / 6 MCUs per row / MCU rows, 7 restart interval in MCUs (0: none), 8 .. 10 first block of
// each component's plane in the coefficient buffer (ep24_jpeg_fdct's cumulative block index), 11 .. 15 0}; row n = {total blocks,
// total segments}.
#define EP24HUFFENC_DESC 16

struct ep24huffenc_image {
    int64_t first_block, first_seg, nblocks, nseg, mcus;
    int64_t plane0, plane1, plane2;      // first coefficient of each component (no array: nothing indexes it at run time)
    int32_t ncomp, h0, v0, mcus_x, mcus_y, ri, bpm, lum;
};

// false: the rows do not fit each other or the buffers - nothing of the image may be read or written.  After true, every index the
// routines below make from I lies inside [0, ncoef_total), the image's blocks and its segments.
EP24_HDF bool ep24huffenc_load(const int64_t* row, int64_t total_blocks, int64_t nseg_total, int64_t ncoef_total, ep24huffenc_image& I) {
    const int64_t* next = row + EP24HUFFENC_DESC;
    I.first_block = row[0], I.first_seg = row[1];
    I.nblocks = next[0] - row[0], I.nseg = next[1] - row[1];
    const int64_t ncomp = row[2], h0 = row[3], v0 = row[4], mx = row[5], my = row[6], ri = row[7];
    if ((ncomp != 1 && ncomp != 3) || h0 < 1 || h0 > 2 || v0 < 1 || v0 > 2 || (v0 == 2 && h0 == 1) || (ncomp == 1 && h0 * v0 != 1)) return false;
    if (mx < 1 || mx > 1024 || my < 1 || my > 1024 || ri < 0 || ri > 65535) return false;
    I.ncomp = (int32_t)ncomp, I.h0 = (int32_t)h0, I.v0 = (int32_t)v0, I.mcus_x = (int32_t)mx, I.mcus_y = (int32_t)my, I.ri = (int32_t)ri;
    I.lum = I.h0 * I.v0;
    I.bpm = ncomp == 1 ? 1 : I.lum + 2;
    I.mcus = mx * my;
    if (I.first_block < 0 || I.nblocks != I.mcus * I.bpm || I.first_block + I.nblocks > total_blocks) return false;
    if (I.first_seg < 0 || I.nseg != (ri ? (I.mcus + ri - 1) / ri : 1) || I.first_seg + I.nseg > nseg_total) return false;
    int64_t plane[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        if (c >= I.ncomp) break;
        const int64_t nb = I.mcus * (c ? 1 : I.lum);
        if (row[8 + c] < 0 || row[8 + c] > (int64_t)1 << 40 || 64 * (row[8 + c] + nb) > ncoef_total) return false;
        plane[c] = 64 * row[8 + c];
    }
    I.plane0 = plane[0], I.plane1 = plane[1], I.plane2 = plane[2];
    return true;
}

struct ep24huffenc_where {
    int64_t at;          // first coefficient of the block
    int64_t pred_at;     // the coefficient that holds the DC predictor, -1: the predictor is 0
    int64_t seg;         // restart segment of the block within the image
    int64_t seg_block;   // first block of that segment, in the image's scan order
    int32_t chroma;      // 0 / 1: which pair of tables
    bool seg_last;       // the segment ends behind this block
};

// block q of the image in SCAN order: MCU by MCU, component 0's h x v blocks row by row, then Cb, then Cr
EP24_HDF ep24huffenc_where ep24huffenc_locate(const ep24huffenc_image& I, int64_t q) {
    ep24huffenc_where W;
    const int64_t m = q / I.bpm;
    const int j = (int)(q - m * I.bpm);
    const int c = j < I.lum ? 0 : j - I.lum + 1;
    const int hc = c ? 1 : I.h0, vc = c ? 1 : I.v0;
    const int jj = c ? 0 : j;
    const int64_t my = m / I.mcus_x, mx = m - my * I.mcus_x, bw = (int64_t)I.mcus_x * hc;
    // sums, not a choice between the three fields: a choice of one of three loads is turned into a load from a chosen address, which
    // puts the whole struct into scratch memory on the device
    const int64_t plane = I.plane0 + (c >= 1 ? I.plane1 - I.plane0 : 0) + (c == 2 ? I.plane2 - I.plane1 : 0);
    W.at = plane + ((my * vc + jj / hc) * bw + (mx * hc + jj % hc)) * 64;
    W.chroma = c ? 1 : 0;
    W.seg = I.ri ? m / I.ri : 0;
    W.seg_block = W.seg * I.ri * I.bpm;
    W.seg_last = j == I.bpm - 1 && (m + 1 == I.mcus || (I.ri && (m + 1) % I.ri == 0));
    if (jj > 0) {                                         // the block in front of it in the same MCU
        W.pred_at = I.plane0 + ((my * vc + (jj - 1) / hc) * bw + (mx * hc + (jj - 1) % hc)) * 64;
    } else if (I.ri ? m % I.ri == 0 : m == 0) {
        W.pred_at = -1;
    } else {                                              // the component's last block of the MCU in front
        const int64_t py = (m - 1) / I.mcus_x, px = (m - 1) - py * I.mcus_x;
        W.pred_at = plane + ((py * vc + (vc - 1)) * bw + (px * hc + (hc - 1))) * 64;
    }
    return W;
}

// ---- unstuffed words -> the file's bytes ----

#define EP24HUFFENC_CHUNK_WORDS 16      // one work item of the stuff passes: 64 unstuffed bytes

// Words [w0, w1) of an image's word buffer through sink: in front of the first word of segment j >= 1 the marker FF D0+((j-1) & 7) as
// sink.raw(byte), then the bytes the segment really holds (ceil(bits / 8); the rest of its last word is not data) as sink.data(byte).
// seg[nseg][2] int64 = {first word of the segment relative to the image's first, its bits - the 1-padding not counted}.
template <class Sink>
EP24_HD void ep24huffenc_chunk(const uint32_t* words, const int64_t* seg, int64_t nseg, int64_t w0, int64_t w1, Sink& sink) {
    int64_t lo = 0, hi = nseg - 1;                        // the last segment that starts at or in front of w0
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (seg[2 * mid] <= w0) lo = mid;
        else hi = mid - 1;
    }
    int64_t s = lo;
    for (int64_t w = w0; w < w1; ++w) {
        while (s + 1 < nseg && seg[2 * (s + 1)] <= w) ++s;
        const int64_t in = w - seg[2 * s];
        if (in == 0 && s >= 1) {
            sink.raw(0xFF);
            sink.raw(0xD0 + (unsigned)((s - 1) & 7));
        }
        const int64_t left = ((seg[2 * s + 1] + 7) >> 3) - 4 * in;
        const uint32_t v = words[w];
        for (int b = 0; b < 4 && b < left; ++b) sink.data((v >> (24 - 8 * b)) & 255u);
    }
}

struct ep24huffenc_byte_counter {
    int64_t n;
    EP24_HD void raw(unsigned) { ++n; }
    EP24_HD void data(unsigned b) { n += b == 0xFF ? 2 : 1; }
};

// writes below `cap` only; `dropped` counts what was not written
struct ep24huffenc_byte_writer {
    uint8_t* out;
    int64_t p, cap;
    int dropped;
    EP24_HD void raw(unsigned b) {
        if (p >= 0 && p < cap) out[p] = (uint8_t)b;
        else ++dropped;
        ++p;
    }
    EP24_HD void data(unsigned b) {
        raw(b);
        if (b == 0xFF) raw(0);
    }
};
