// ep24 - the baseline JPEG Huffman state machine, shared by the host (jpeg_host.cpp: ep24jpeg_selfsync_emulate, with threads as
// loops) and the device (jpeg_huff.hip: jpeg_huff_kernel).  One text, so that what the sanitizer build of jpeg_device_check.cpp walks
// through is what the kernel runs.  Plain C++ and integers only; every function is EP24_HD: __host__ __device__ under hipcc, plain
// inline for the host compiler.
//
// A restart segment is a run of raw bytes [seg_off, seg_end) of the image's scan in which every FF is followed by its stuffed 00.
// A POSITION is the raw bit index (8 * byte + bit, relative to the scan's first byte) of the next unread bit; it never points into a
// stuffed 00.  A STATE is (position, zig-zag index k of the next symbol, block-in-MCU j); position EP24HUFF_PARKED is "no state":
// what a thread without a subsequence holds.
//
// ep24huff_run decodes every symbol that STARTS in front of raw byte `bound` (the end of a subsequence) and returns the state behind
// the last one and the number of blocks begun (DC symbols started).  Loops: a block loop step consumes at least one bit (no code has
// length 0) and the bits in front of `bound` are finite; a code search is 7 steps, a refill at most 8.
#pragma once
#include <stdint.h>

#ifndef EP24_HD
#if defined(__HIPCC__)
#define EP24_HD __host__ __device__ inline
#else
#define EP24_HD inline
#endif
#endif

#define EP24HUFF_LOOK 9
#define EP24HUFF_PARKED 0xFFFFFFFFu

struct ep24huff_table {
    uint16_t look[1 << EP24HUFF_LOOK];   // (length << 8) | symbol for codes of at most 9 bits, 0 otherwise
    int32_t maxcode[17];                 // largest code of each length, -1: none
    int32_t valoff[17];                  // vals index = code + valoff[length]
    int32_t nvals;
    uint8_t vals[256];
};

struct ep24huff_state {
    uint32_t pos;                        // raw bit position, or EP24HUFF_PARKED
    uint32_t kj;                         // k | j << 8
};

// what the decode of one image needs besides the segment: the component geometry of ep24_jpeg_idct's coefficient layout
struct ep24huff_image {
    const uint8_t* d;                    // the scan's bytes
    const ep24huff_table* tabs;          // six: DC of component 0 .. 2, then AC of component 0 .. 2
    int32_t ncomp, h0, v0, mcus_x;       // chroma is 1 x 1
    int32_t bpm;                         // blocks per MCU: h0 * v0 (+ 2)
    int64_t off1, off2;                  // first coefficient of components 1 and 2, relative to the image's first (component 0: 0)
    int64_t ncoef;                       // the image's coefficient count: no store at or behind it
};

struct ep24huff_segment {
    uint32_t off, end;                   // raw byte range in the scan
    int32_t first_mcu;                   // of the image
    int32_t expect;                      // blocks the segment must hold
};

struct ep24huff_bits {
    const uint8_t* d;
    uint32_t p;                          // raw index of the next byte to load (virtual behind seg end)
    uint32_t end;                        // the segment's end
    uint32_t bound;                      // the subsequence's end
    uint64_t acc;
    int n;                               // unread bits in acc
    int over;                            // of the loaded bits, those from bytes at or behind bound (made-up ones included)
    int pad;                             // of the loaded bits, zero bits made up behind the segment's end
};

EP24_HD int ep24huff_zigzag(int k) {
    const uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// build_huff of jpeg_host.cpp in two steps, so that a workgroup can share the second: the 16 lengths (one thread per table), then the
// 512 look-ahead entries, each on its own (any thread).
// Step 1: maxcode / valoff per length and the symbols.  false: more codes of a length than fit, or more codes than symbols (the table
// is then empty: every code is invalid)
EP24_HD bool ep24huff_build_lengths(ep24huff_table& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    if (nvals < 0) nvals = 0;
    if (nvals > 256) nvals = 256;
    h.nvals = nvals;
    for (int i = 0; i < 256; ++i) h.vals[i] = i < nvals ? vals[i] : (uint8_t)0;
    int32_t code = 0;
    int k = 0;
    bool ok = true;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        const int cnt = counts[l - 1];
        if (code + cnt > (1 << l) || k + cnt > nvals) {
            ok = false;
            break;
        }
        code += cnt;
        k += cnt;
        h.maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[0] = -1;
    h.valoff[0] = 0;
    if (!ok) {
        for (int l = 0; l <= 16; ++l) h.maxcode[l] = -1, h.valoff[l] = 0;
        h.nvals = 0;
    }
    return ok;
}

// Step 2: look-ahead entry w (the next 9 bits): (length << 8) | symbol of the code of at most 9 bits that w starts with, 0 if none.
// In a canonical code the l-bit prefix of w is a code of length l exactly when it is the first prefix at or below maxcode[l].
EP24_HD uint16_t ep24huff_look_entry(const ep24huff_table& h, int w) {
    for (int l = 1; l <= EP24HUFF_LOOK; ++l) {
        const int32_t code = w >> (EP24HUFF_LOOK - l);
        if (code <= h.maxcode[l]) {
            const int idx = code + h.valoff[l];
            if (idx < 0 || idx >= h.nvals) return 0;
            return (uint16_t)((l << 8) | h.vals[idx]);
        }
    }
    return 0;
}

EP24_HD bool ep24huff_build(ep24huff_table& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    const bool ok = ep24huff_build_lengths(h, counts, vals, nvals);
    for (int w = 0; w < (1 << EP24HUFF_LOOK); ++w) h.look[w] = ep24huff_look_entry(h, w);
    return ok;
}

// the bit reader: FF 00 un-stuffing, zero bits behind the segment's end
EP24_HD void ep24huff_fill(ep24huff_bits& b) {
    while (b.n <= 56) {
        uint32_t v = 0;
        const uint32_t at = b.p;
        if (at < b.end) {
            v = b.d[at];
            b.p = at + 1;
            if (v == 0xFF && b.p < b.end && b.d[b.p] == 0) ++b.p;
        } else {
            b.p = at + 1;
            b.pad += 8;
        }
        if (at >= b.bound) b.over += 8;
        b.acc = (b.acc << 8) | v;
        b.n += 8;
    }
}

EP24_HD void ep24huff_open(ep24huff_bits& b, const uint8_t* d, uint32_t seg_end, uint32_t bound, uint32_t pos) {
    b.d = d;
    b.p = pos >> 3;
    b.end = seg_end;
    b.bound = bound;
    b.acc = 0;
    b.n = b.over = b.pad = 0;
    ep24huff_fill(b);
    b.n -= (int)(pos & 7);
}

// the raw bit position of the next unread bit: the ceil(n / 8) bytes that hold unread bits, walked back from p over stuffed bytes
EP24_HD uint32_t ep24huff_tell(const ep24huff_bits& b, uint32_t seg_off) {
    const int c = (b.n + 7) >> 3;
    uint32_t j = b.p;
    for (int i = 0; i < c; ++i) {
        --j;
        if (j < b.end && j > seg_off && b.d[j] == 0 && b.d[j - 1] == 0xFF) --j;
    }
    return j * 8u + (uint32_t)(8 * c - b.n);
}

// a code (at most 16 bits) and the value behind it (at most 15) are read after ONE refill: the caller keeps 32 bits in the buffer
EP24_HD int ep24huff_symbol(ep24huff_bits& b, const ep24huff_table& h) {
    const uint32_t w = (uint32_t)(b.acc >> (b.n - 16)) & 0xFFFFu;
    const uint16_t e = h.look[w >> (16 - EP24HUFF_LOOK)];
    if (e) {
        b.n -= e >> 8;
        return e & 255;
    }
    for (int l = EP24HUFF_LOOK + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(w >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int idx = code + h.valoff[l];
            if (idx < 0 || idx >= h.nvals) return -1;
            b.n -= l;
            return h.vals[idx];
        }
    }
    return -1;
}

// s bits (1 .. 15) as a signed value: EXTEND(v, s) = v if v >= 2^(s-1) else v - 2^s + 1
EP24_HD int ep24huff_receive_extend(ep24huff_bits& b, int s) {
    const int v = (int)((b.acc >> (b.n - s)) & ((1u << s) - 1));
    b.n -= s;
    const int below = (v - (1 << (s - 1))) >> 31;
    return v + (below & (1 - (1 << s)));
}

// the first position of subsequence i (> 0) of a segment: its byte boundary, one byte later where that is the 00 of an FF 00 pair
EP24_HD uint32_t ep24huff_spec_start(const uint8_t* d, uint32_t seg_off, uint32_t at) {
    if (at > seg_off && d[at] == 0 && d[at - 1] == 0xFF) ++at;
    return at * 8u;
}

// Where coefficient `nat` (natural order) of block `blk` of the segment lies; -1: outside the image (dropped)
EP24_HD int64_t ep24huff_where(const ep24huff_image& im, const ep24huff_segment& sg, int blk, int nat) {
    const int m = sg.first_mcu + blk / im.bpm, j = blk % im.bpm;
    const int my = m / im.mcus_x, mx = m - my * im.mcus_x;
    const int nl = im.h0 * im.v0;
    int c, by = 0, bx = 0, h = 1, v = 1;
    if (j < nl) {
        c = 0, h = im.h0, v = im.v0;
        by = j / h, bx = j - by * h;
    } else {
        c = j - nl + 1;
    }
    if (c >= im.ncomp) return -1;
    const int64_t bw = (int64_t)im.mcus_x * h;
    const int64_t at = (c == 0 ? 0 : c == 1 ? im.off1 : im.off2) + (((int64_t)my * v + by) * bw + ((int64_t)mx * h + bx)) * 64 + nat;
    return (at >= 0 && at < im.ncoef) ? at : -1;
}

EP24_HD int ep24huff_comp(const ep24huff_image& im, int j) {
    const int nl = im.h0 * im.v0;
    const int c = j < nl ? 0 : j - nl + 1;
    return c < im.ncomp ? c : im.ncomp - 1;
}

// Decode from `in` every symbol that starts in front of raw byte `bound` (<= sg.end).
//   WRITE false (the synchronisation rounds): *out the state behind them, *begun the blocks begun.  Speculation is never an error,
//     and it does not stop either: an invalid code costs one bit and the decode goes on, a run past coefficient 63 ends the block.
//     (A thread that stopped there - "parked" until its start state changes - hands "no state" to its successor, which then cannot
//     synchronise before the correction reaches it: in the host emulation the photo fixture then needs 1 023 rounds of a tile of
//     1 024 where this needs 12; DESIGN.md has the figures.  They are the emulation's: that form was never run on the device.)  What such a decode returns is a guess like any other: only a start state that equals the
//     predecessor's end state, in a chain from an anchored thread, is ever written from.
//   WRITE true (the write pass, from a verified state): excl = blocks of the segment begun in front of this subsequence.  Stores the
//     coefficients (the DC as its DIFFERENCE) of every block below sg.expect, drops the others; last: this is the segment's last
//     subsequence.  Returns true on an error inside a block the segment must hold: an invalid code, a run past coefficient 63,
//     made-up bits consumed, or (last) fewer complete blocks than sg.expect.  Up to the first such error the rounds and the write
//     pass read the same symbols; behind it the image's status is set and its coefficients are unspecified (but in bounds).
template <bool WRITE>
EP24_HD bool ep24huff_run(const ep24huff_image& im, const ep24huff_segment& sg, ep24huff_state in, uint32_t bound, ep24huff_state* out,
                          int* begun, int16_t* coef, int excl, bool last) {
    if (in.pos == EP24HUFF_PARKED) {                      // "no state": a thread without a subsequence
        if (!WRITE) *out = in, *begun = 0;
        return false;
    }
    ep24huff_bits b;
    ep24huff_open(b, im.d, sg.end, bound, in.pos);
    int k = (int)(in.kj & 255u), j = (int)(in.kj >> 8);
    if (k > 63) k = 0;
    if (j >= im.bpm) j = 0;
    int nb = 0;
    int cur = k ? excl - 1 : excl;                        // the block in progress, or the next one to begin
    for (;;) {
        if (b.n < 32) ep24huff_fill(b);
        if (b.n <= b.over) break;                         // the next symbol starts at or behind bound
        const int c = ep24huff_comp(im, j);
        if (k == 0) {
            const int t = ep24huff_symbol(b, im.tabs[c]);
            if (t < 0 || t > 11) {
                if (WRITE) return cur < sg.expect;
                if (t < 0) b.n -= 1;                      // a code of more than 11 value bits has been consumed: at least one bit either way
                continue;
            }
            ++nb;
            const int diff = t ? ep24huff_receive_extend(b, t) : 0;
            if (WRITE && cur < sg.expect) {
                if (b.pad > b.n) return true;
                const int64_t at = ep24huff_where(im, sg, cur, 0);
                if (at >= 0) coef[at] = (int16_t)diff;
            }
            k = 1;
        } else {
            const int rs = ep24huff_symbol(b, im.tabs[3 + c]);
            if (rs < 0) {
                if (WRITE) return cur < sg.expect;
                b.n -= 1;
                continue;
            }
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                k = (r == 15) ? k + 16 : 64;              // ZRL, or end of block
            } else {
                k += r;
                if (k > 63) {
                    if (WRITE) return cur < sg.expect;
                    k = 63;                               // the value bits are read, the block ends
                }
                const int v = ep24huff_receive_extend(b, s);
                if (WRITE && cur < sg.expect) {
                    const int64_t at = ep24huff_where(im, sg, cur, ep24huff_zigzag(k));
                    if (at >= 0) coef[at] = (int16_t)v;
                }
                ++k;
            }
            if (WRITE && cur < sg.expect && b.pad > b.n) return true;
        }
        if (k >= 64) {
            k = 0;
            j = j + 1 == im.bpm ? 0 : j + 1;
            ++cur;
        }
    }
    if (WRITE) return last && cur < sg.expect;
    *begun = nb;
    out->pos = ep24huff_tell(b, sg.off);
    out->kj = (uint32_t)k | ((uint32_t)j << 8);
    return false;
}
