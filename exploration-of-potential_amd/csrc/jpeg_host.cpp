// ep24 - host entropy stage of the JPEG decoder (include/ep24_jpeg.h): marker parser and table-driven baseline Huffman decoder.
// Host compiler only: no HIP, no device code - the loader processes load this library without opening the GPU.
//
// Every read of the file goes through a position that is checked against n; every write goes to coef_out below ncoef (<= capacity)
// or into the header; a block decodes in at most 64 steps whatever the bits say, so corrupt input ends in EP24JPEG_E_DATA.
//
// The writer (ep24jpeg_entropy_encode, below the decoder's helpers) is its mirror: markers, the Annex K Huffman tables and the
// interleaved scan from a header and coefficients in the decoder's layout.  Every byte goes through put_byte, which checks the capacity.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/ep24_jpeg.h"
#include "jpeg_huff_core.h"
#include "jpeg_huffenc_core.h"

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

enum { LOOK = 9 };

struct Huff {
    bool defined;
    int nvals;
    uint8_t bits[16];              // codes per length 1 .. 16, as the file gives them
    uint8_t vals[256];
    uint16_t look[1 << LOOK];      // (length << 8) | symbol for codes of at most LOOK bits, 0 otherwise
    int32_t maxcode[17];           // largest code of each length, -1: none
    int32_t valoff[17];            // vals index = code + valoff[length]
};

struct Parsed {
    ep24jpeg_header hd;
    int tq[3], td[3], ta[3], id[3];
    int mcus_x, mcus_y;
    int64_t scan_pos;
    Huff dc[4], ac[4];
};

int build_huff(Huff& h, const uint8_t* bits, const uint8_t* vals, int nvals) {
    h.defined = true;
    h.nvals = nvals;
    memcpy(h.bits, bits, 16);
    memcpy(h.vals, vals, (size_t)nvals);
    memset(h.look, 0, sizeof(h.look));
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        const int cnt = bits[l - 1];
        if (code + cnt > (1 << l)) return fail(EP24JPEG_E_DATA, "jpeg: a Huffman table has more codes of length %d than fit", l);
        if (l <= LOOK)
            for (int i = 0; i < cnt; ++i) {
                const int lo = (code + i) << (LOOK - l);
                for (int j = 0; j < (1 << (LOOK - l)); ++j) h.look[lo + j] = (uint16_t)((l << 8) | vals[k + i]);
            }
        code += cnt;
        k += cnt;
        h.maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    return EP24JPEG_OK;
}

inline int u16(const uint8_t* d, int64_t p) { return (d[p] << 8) | d[p + 1]; }

int parse(const uint8_t* d, int64_t n, Parsed& P) {
    memset(&P.hd, 0, sizeof(P.hd));
    for (int i = 0; i < 4; ++i) P.dc[i].defined = P.ac[i].defined = false;
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(EP24JPEG_E_DATA, "jpeg: not a JPEG file (no SOI marker)");
    uint16_t qt[4][64];
    bool qt_def[4] = {false, false, false, false}, have_frame = false;
    int64_t p = 2;
    for (;;) {
        if (p + 2 > n) return fail(EP24JPEG_E_DATA, "jpeg: the file ends before the scan (offset %lld)", (long long)p);
        if (d[p] != 0xFF) return fail(EP24JPEG_E_DATA, "jpeg: marker expected at offset %lld", (long long)p);
        while (p < n && d[p] == 0xFF) ++p;             // fill bytes
        if (p >= n) return fail(EP24JPEG_E_DATA, "jpeg: the file ends inside a marker");
        const int m = d[p++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;       // no parameters
        if (m == 0xD9) return fail(EP24JPEG_E_DATA, "jpeg: EOI before any scan");
        if (m == 0x00) return fail(EP24JPEG_E_DATA, "jpeg: stuffed byte outside a scan");
        if (p + 2 > n) return fail(EP24JPEG_E_DATA, "jpeg: the file ends inside a segment header");
        const int L = u16(d, p);
        if (L < 2 || p + L > n) return fail(EP24JPEG_E_DATA, "jpeg: segment FF%02X of length %d runs past the end of the file", m, L);
        const uint8_t* s = d + p + 2;
        const int sl = L - 2;
        const int64_t end = p + L;
        if (m == 0xDB) {
            int q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, t = s[q] & 15;
                const int need = pq ? 129 : 65;
                if (pq > 1 || t > 3 || q + need > sl) return fail(EP24JPEG_E_DATA, "jpeg: bad quantisation table segment");
                for (int k = 0; k < 64; ++k) qt[t][ep24huff_zigzag(k)] = (uint16_t)(pq ? u16(s, q + 1 + 2 * k) : s[q + 1 + k]);
                qt_def[t] = true;
                q += need;
            }
        } else if (m == 0xC4) {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) return fail(EP24JPEG_E_DATA, "jpeg: bad Huffman table segment");
                const int tc = s[q] >> 4, th = s[q] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += s[q + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || q + 17 + cnt > sl) return fail(EP24JPEG_E_DATA, "jpeg: bad Huffman table segment");
                const int rc = build_huff(tc ? P.ac[th] : P.dc[th], s + q + 1, s + q + 17, cnt);
                if (rc) return rc;
                q += 17 + cnt;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_frame) return fail(EP24JPEG_E_DATA, "jpeg: a second frame header");
            if (sl < 6) return fail(EP24JPEG_E_DATA, "jpeg: short frame header");
            if (s[0] != 8) return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: %d-bit sample precision is not supported (8-bit only)", s[0]);
            ep24jpeg_header& h = P.hd;
            h.height = u16(s, 1);
            h.width = u16(s, 3);
            h.ncomp = s[5];
            if (h.ncomp != 1 && h.ncomp != 3)
                return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: %d components are not supported (1 or 3; CMYK / YCCK files have 4)", h.ncomp);
            if (sl < 6 + 3 * h.ncomp) return fail(EP24JPEG_E_DATA, "jpeg: short frame header");
            if (h.width < 1 || h.height < 1) return fail(EP24JPEG_E_DATA, "jpeg: empty image (%d x %d)", h.width, h.height);
            if (h.width > EP24JPEG_MAX_SIDE || h.height > EP24JPEG_MAX_SIDE)
                return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: %d x %d is above the supported side of %d", h.width, h.height, EP24JPEG_MAX_SIDE);
            for (int i = 0; i < h.ncomp; ++i) {
                P.id[i] = s[6 + 3 * i];
                h.h[i] = s[7 + 3 * i] >> 4;
                h.v[i] = s[7 + 3 * i] & 15;
                P.tq[i] = s[8 + 3 * i];
                if (P.tq[i] > 3 || h.h[i] < 1 || h.v[i] < 1) return fail(EP24JPEG_E_DATA, "jpeg: bad component %d in the frame header", i);
            }
            if (h.ncomp == 1) {
                h.h[0] = h.v[0] = 1;                   // a one-component scan is not interleaved: its MCU is one block
            } else {
                const bool luma = (h.h[0] == 1 && h.v[0] == 1) || (h.h[0] == 2 && h.v[0] == 1) || (h.h[0] == 2 && h.v[0] == 2);
                if (!luma || h.h[1] != 1 || h.v[1] != 1 || h.h[2] != 1 || h.v[2] != 1)
                    return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: sampling %dx%d,%dx%d,%dx%d is not supported (luma 1x1, 2x1 or 2x2 with chroma 1x1)",
                                h.h[0], h.v[0], h.h[1], h.v[1], h.h[2], h.v[2]);
            }
            have_frame = true;
        } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
            return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: progressive files (SOF%d) are not supported (baseline only)", m - 0xC0);
        } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
            return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: arithmetic coding (SOF%d) is not supported", m - 0xC0);
        } else if (m == 0xCC) {
            return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: arithmetic coding (DAC segment) is not supported");
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC7) {
            return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: lossless / hierarchical files (SOF%d) are not supported", m - 0xC0);
        } else if (m == 0xDD) {
            if (sl < 2) return fail(EP24JPEG_E_DATA, "jpeg: short DRI segment");
            P.hd.restart_interval = u16(s, 0);
        } else if (m == 0xDA) {
            if (!have_frame) return fail(EP24JPEG_E_DATA, "jpeg: a scan before the frame header");
            ep24jpeg_header& h = P.hd;
            if (sl < 1) return fail(EP24JPEG_E_DATA, "jpeg: short scan header");
            const int ns = s[0];
            if (ns != h.ncomp)
                return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: more than one scan (the first holds %d of %d components) is not supported", ns, h.ncomp);
            if (sl < 1 + 2 * ns + 3) return fail(EP24JPEG_E_DATA, "jpeg: short scan header");
            for (int i = 0; i < ns; ++i) {
                if (s[1 + 2 * i] != P.id[i]) return fail(EP24JPEG_E_DATA, "jpeg: scan component %d does not follow the frame's order", i);
                P.td[i] = s[2 + 2 * i] >> 4;
                P.ta[i] = s[2 + 2 * i] & 15;
                if (P.td[i] > 3 || P.ta[i] > 3 || !P.dc[P.td[i]].defined || !P.ac[P.ta[i]].defined)
                    return fail(EP24JPEG_E_DATA, "jpeg: component %d uses a Huffman table that was not defined", i);
                if (!qt_def[P.tq[i]]) return fail(EP24JPEG_E_DATA, "jpeg: component %d uses a quantisation table that was not defined", i);
                memcpy(h.qt[i], qt[P.tq[i]], sizeof(h.qt[i]));
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: a scan with spectral selection / successive approximation is not supported");
            int hmax = 1, vmax = 1;
            for (int i = 0; i < h.ncomp; ++i) {
                if (h.h[i] > hmax) hmax = h.h[i];
                if (h.v[i] > vmax) vmax = h.v[i];
            }
            P.mcus_x = (h.width + 8 * hmax - 1) / (8 * hmax);
            P.mcus_y = (h.height + 8 * vmax - 1) / (8 * vmax);
            h.ncoef = 0;
            for (int i = 0; i < h.ncomp; ++i) {
                h.blocks_w[i] = P.mcus_x * h.h[i];
                h.blocks_h[i] = P.mcus_y * h.v[i];
                h.nblocks[i] = (int64_t)h.blocks_w[i] * h.blocks_h[i];
                h.ncoef += 64 * h.nblocks[i];
            }
            P.scan_pos = end;
            return EP24JPEG_OK;
        }                                                 // APPn, COM and everything else with a length: skipped
        p = end;
    }
}

struct Bits {
    const uint8_t* d;
    int64_t p, end;
    uint64_t acc;
    int n;          // unread bits in acc
    int pad;        // of them (at the low end), zero bits made up after the data ended; pad > n: made-up bits were consumed
    bool stop;      // a marker (or the end of the file) was reached
};

inline void fill(Bits& b) {
    // four bytes at once while none of them is 0xFF (no stuffing, no marker) and the file has them
    if (b.n <= 32 && !b.stop && b.p + 4 <= b.end) {
        uint32_t w;
        memcpy(&w, b.d + b.p, 4);
        const uint32_t inv = ~w;                          // a 0xFF byte of w is a zero byte of inv
        if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
            b.acc = (b.acc << 32) | __builtin_bswap32(w);
            b.n += 32;
            b.p += 4;
            return;
        }
    }
    while (b.n <= 56) {
        unsigned v = 0;
        if (!b.stop && b.p < b.end) {
            v = b.d[b.p];
            if (v == 0xFF) {
                if (b.p + 1 < b.end && b.d[b.p + 1] == 0) {
                    b.p += 2;
                } else {
                    b.stop = true;
                    v = 0;
                    b.pad += 8;
                }
            } else {
                ++b.p;
            }
        } else {
            b.stop = true;
            b.pad += 8;
        }
        b.acc = (b.acc << 8) | v;
        b.n += 8;
    }
}

// a code (at most 16 bits) and the value behind it (at most 15) are read after ONE refill: the caller keeps 32 bits in the buffer
inline int decode_symbol(Bits& b, const Huff& h) {
    const uint32_t w = (uint32_t)(b.acc >> (b.n - 16)) & 0xFFFFu;
    const uint16_t e = h.look[w >> (16 - LOOK)];
    if (e) {
        b.n -= e >> 8;
        return e & 255;
    }
    for (int l = LOOK + 1; l <= 16; ++l) {
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
inline int receive_extend(Bits& b, int s) {
    const int v = (int)((b.acc >> (b.n - s)) & ((1u << s) - 1));
    b.n -= s;
    // without a branch (the sign of a coefficient is a coin toss): all ones when v is below 2^(s-1)
    const int below = (v - (1 << (s - 1))) >> 31;
    return v + (below & (1 - (1 << s)));
}

// ---- the encoder's side: Annex K's tables, a bit writer that never leaves its buffer ----

const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// what ep24.jpeg._check refuses, and what the marker segments cannot say
int check_header(const ep24jpeg_header& h, int& mcus_x, int& mcus_y) {
    mcus_x = mcus_y = 0;
    if ((h.ncomp != 1 && h.ncomp != 3) || h.width < 1 || h.height < 1 || h.width > EP24JPEG_MAX_SIDE || h.height > EP24JPEG_MAX_SIDE)
        return fail(EP24JPEG_E_ARG, "jpeg encode: inconsistent header (%d components, %d x %d)", h.ncomp, h.width, h.height);
    if (h.restart_interval < 0 || h.restart_interval > 65535)
        return fail(EP24JPEG_E_ARG, "jpeg encode: restart interval %d outside 0 .. 65535", h.restart_interval);
    if (h.ncomp == 1) {
        if (h.h[0] != 1 || h.v[0] != 1) return fail(EP24JPEG_E_ARG, "jpeg encode: a one-component image is sampled 1x1");
    } else {
        const bool luma = (h.h[0] == 1 && h.v[0] == 1) || (h.h[0] == 2 && h.v[0] == 1) || (h.h[0] == 2 && h.v[0] == 2);
        if (!luma || h.h[1] != 1 || h.v[1] != 1 || h.h[2] != 1 || h.v[2] != 1)
            return fail(EP24JPEG_E_ARG, "jpeg encode: sampling %dx%d,%dx%d,%dx%d (luma 1x1, 2x1 or 2x2 with chroma 1x1)", h.h[0], h.v[0], h.h[1],
                        h.v[1], h.h[2], h.v[2]);
    }
    mcus_x = (h.width + 8 * h.h[0] - 1) / (8 * h.h[0]);
    mcus_y = (h.height + 8 * h.v[0] - 1) / (8 * h.v[0]);
    int64_t ncoef = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        if (h.blocks_w[c] != mcus_x * h.h[c] || h.blocks_h[c] != mcus_y * h.v[c] || h.nblocks[c] != (int64_t)h.blocks_w[c] * h.blocks_h[c])
            return fail(EP24JPEG_E_ARG, "jpeg encode: the block grid of component %d does not fit a %d x %d image", c, h.width, h.height);
        ncoef += 64 * h.nblocks[c];
        for (int k = 0; k < 64; ++k)
            if (h.qt[c][k] < 1 || h.qt[c][k] > 255)
                return fail(EP24JPEG_E_ARG, "jpeg encode: quantisation table entry %d of component %d is %d (baseline: 1 .. 255)", k, c, h.qt[c][k]);
    }
    if (h.ncoef != ncoef) return fail(EP24JPEG_E_ARG, "jpeg encode: ncoef %lld is not 64 x the %lld blocks", (long long)h.ncoef, (long long)(ncoef / 64));
    return EP24JPEG_OK;
}

int64_t encode_bound(const ep24jpeg_header& h, int mcus_x, int mcus_y) {
    // markers and tables stay below 1 KiB; a coefficient is at most a 16-bit code and 11 value bits, every byte of them stuffed: below
    // 8 bytes; a restart marker and the padding in front of it: 4 bytes per MCU at the most
    return 1024 + 8 * h.ncoef + 4 * (int64_t)mcus_x * mcus_y;
}

struct Writer {
    uint8_t* out;
    int64_t p, cap;
    uint64_t acc;
    int n;          // bits held in acc (below 32 between calls)
};

inline void put_byte(Writer& w, unsigned b) {
    if (w.p < w.cap) w.out[w.p] = (uint8_t)b;
    ++w.p;
}

inline void put_u16(Writer& w, unsigned v) {
    put_byte(w, v >> 8);
    put_byte(w, v & 255);
}

inline void put_bits(Writer& w, unsigned code, int len) {      // len <= 27
    w.acc = (w.acc << len) | code;
    w.n += len;
    while (w.n >= 8) {
        const unsigned b = (unsigned)(w.acc >> (w.n - 8)) & 255u;
        put_byte(w, b);
        if (b == 0xFF) put_byte(w, 0);
        w.n -= 8;
    }
}

inline void flush_bits(Writer& w) {                              // the last byte in front of a marker is filled with ones
    if (w.n > 0) put_bits(w, (1u << (8 - w.n)) - 1, 8 - w.n);
    w.acc = 0;
    w.n = 0;
}

inline int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

// the Annex K table (ac: 0 / 1, t: 0 luminance, 1 chrominance) of csrc/jpeg_huffenc_core.h as a DHT segment
void put_dht(Writer& w, int ac, int t) {
    int cnt = 0;
    for (int i = 0; i < 16; ++i) cnt += ac ? ep24huffenc_ac_bits(t, i) : ep24huffenc_dc_bits(t, i);
    put_u16(w, 0xFFC4);
    put_u16(w, 2 + 1 + 16 + cnt);
    put_byte(w, (unsigned)((ac << 4) | t));
    for (int i = 0; i < 16; ++i) put_byte(w, (unsigned)(ac ? ep24huffenc_ac_bits(t, i) : ep24huffenc_dc_bits(t, i)));
    for (int i = 0; i < cnt; ++i) put_byte(w, (unsigned)(ac ? ep24huffenc_ac_val(t, i) : ep24huffenc_dc_val(t, i)));
}

// SOI up to and including the SOS header
void put_header(Writer& w, const ep24jpeg_header& h) {
    put_u16(w, 0xFFD8);
    static const uint8_t kApp0[16] = {0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_u16(w, 0xFFE0);
    for (int i = 0; i < 16; ++i) put_byte(w, kApp0[i]);
    // Cb and Cr share table 1 when their tables are equal (what every common encoder writes); a third table otherwise
    int tq[3] = {0, 1, 1}, ntab = h.ncomp == 1 ? 1 : 2;
    if (h.ncomp == 3 && memcmp(h.qt[1], h.qt[2], sizeof(h.qt[1])) != 0) tq[2] = 2, ntab = 3;
    for (int t = 0; t < ntab; ++t) {
        put_u16(w, 0xFFDB);
        put_u16(w, 67);
        put_byte(w, (unsigned)t);
        for (int k = 0; k < 64; ++k) put_byte(w, h.qt[t][ep24huff_zigzag(k)]);
    }
    put_u16(w, 0xFFC0);
    put_u16(w, 8 + 3 * h.ncomp);
    put_byte(w, 8);
    put_u16(w, (unsigned)h.height);
    put_u16(w, (unsigned)h.width);
    put_byte(w, (unsigned)h.ncomp);
    for (int c = 0; c < h.ncomp; ++c) {
        put_byte(w, (unsigned)(c + 1));
        put_byte(w, (unsigned)((h.h[c] << 4) | h.v[c]));
        put_byte(w, (unsigned)tq[c]);
    }
    const int nh = h.ncomp == 1 ? 1 : 2;
    for (int t = 0; t < nh; ++t) {
        put_dht(w, 0, t);
        put_dht(w, 1, t);
    }
    if (h.restart_interval > 0) {
        put_u16(w, 0xFFDD);
        put_u16(w, 4);
        put_u16(w, (unsigned)h.restart_interval);
    }
    put_u16(w, 0xFFDA);
    put_u16(w, 6 + 2 * h.ncomp);
    put_byte(w, (unsigned)h.ncomp);
    for (int c = 0; c < h.ncomp; ++c) {
        put_byte(w, (unsigned)(c + 1));
        put_byte(w, c ? 0x11u : 0x00u);
    }
    put_byte(w, 0);
    put_byte(w, 63);
    put_byte(w, 0);
}

}  // namespace

extern "C" int ep24jpeg_quality_tables(int quality, uint16_t qt[2][64]) {
    if (!qt) return fail(EP24JPEG_E_ARG, "ep24jpeg_quality_tables: null pointer");
    if (quality < 1 || quality > 100) return fail(EP24JPEG_E_ARG, "ep24jpeg_quality_tables: quality %d outside 1 .. 100", quality);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            int v = (kBaseQ[t][k] * scale + 50) / 100;
            qt[t][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return EP24JPEG_OK;
}

extern "C" int64_t ep24jpeg_encode_bound(const ep24jpeg_header* header) {
    if (!header) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_bound: null pointer");
    int mx, my;
    const int rc = check_header(*header, mx, my);
    if (rc) return rc;
    return encode_bound(*header, mx, my);
}

extern "C" int ep24jpeg_entropy_encode(const ep24jpeg_header* header, const int16_t* coef, int64_t ncoef, uint8_t* out, int64_t capacity,
                                       int64_t* nbytes) {
    if (!header || !coef || !out || !nbytes) return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_encode: null pointer");
    const ep24jpeg_header& h = *header;
    int mcus_x, mcus_y;
    int rc = check_header(h, mcus_x, mcus_y);
    if (rc) return rc;
    if (ncoef != h.ncoef) return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_encode: %lld coefficients given, the header holds %lld", (long long)ncoef, (long long)h.ncoef);
    const int64_t bound = encode_bound(h, mcus_x, mcus_y);
    if (capacity < bound) return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_encode: capacity %lld below the bound %lld", (long long)capacity, (long long)bound);

    Writer w = {out, 0, capacity, 0, 0};
    put_header(w, h);

    uint32_t tab[EP24HUFFENC_TABLE] = {0};                 // code | length << 16 per symbol, the tables the device encoder builds
    for (int i = 0; i < EP24HUFFENC_ENTRIES; ++i) ep24huffenc_fill(tab, i);
    const int16_t* base[3];
    int64_t off = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        base[c] = coef + off;
        off += 64 * h.nblocks[c];
    }
    int pred[3] = {0, 0, 0};
    const int ri = h.restart_interval;
    int rst = 0, left = ri;
    for (int my = 0; my < mcus_y; ++my)
        for (int mx = 0; mx < mcus_x; ++mx) {
            if (ri) {
                if (left == 0) {
                    flush_bits(w);
                    put_u16(w, 0xFFD0u + (unsigned)rst);
                    rst = (rst + 1) & 7;
                    pred[0] = pred[1] = pred[2] = 0;
                    left = ri;
                }
                --left;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const uint32_t* hdc = tab + EP24HUFFENC_DC(c ? 1 : 0);
                const uint32_t* hac = tab + EP24HUFFENC_AC(c ? 1 : 0);
                for (int by = 0; by < h.v[c]; ++by)
                    for (int bx = 0; bx < h.h[c]; ++bx) {
                        const int16_t* blk = base[c] + ((int64_t)(my * h.v[c] + by) * h.blocks_w[c] + (mx * h.h[c] + bx)) * 64;
                        const int diff = blk[0] - pred[c];
                        pred[c] = blk[0];
                        if (diff < -2047 || diff > 2047)
                            return fail(EP24JPEG_E_ARG, "jpeg encode: DC difference %d in MCU %d is outside baseline's +-2047", diff, my * mcus_x + mx);
                        int a = diff < 0 ? -diff : diff;
                        int s = bit_size(a);
                        put_bits(w, hdc[s] & 0xFFFFu, (int)(hdc[s] >> 16));
                        if (s) put_bits(w, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            const int v = blk[ep24huff_zigzag(k)];
                            if (v == 0) {
                                ++run;
                                continue;
                            }
                            if (v < -1023 || v > 1023)
                                return fail(EP24JPEG_E_ARG, "jpeg encode: AC coefficient %d in MCU %d is outside baseline's +-1023", v, my * mcus_x + mx);
                            while (run > 15) {
                                put_bits(w, hac[0xF0] & 0xFFFFu, (int)(hac[0xF0] >> 16));
                                run -= 16;
                            }
                            a = v < 0 ? -v : v;
                            s = bit_size(a);
                            const int sym = (run << 4) | s;
                            put_bits(w, hac[sym] & 0xFFFFu, (int)(hac[sym] >> 16));
                            put_bits(w, (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
                            run = 0;
                        }
                        if (run) put_bits(w, hac[0] & 0xFFFFu, (int)(hac[0] >> 16));
                    }
            }
        }
    flush_bits(w);
    put_u16(w, 0xFFD9);
    if (w.p > capacity) return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_encode: the stream outgrew its bound (%lld > %lld)", (long long)w.p, (long long)capacity);
    *nbytes = w.p;
    return EP24JPEG_OK;
}

extern "C" int ep24jpeg_encode_header(const ep24jpeg_header* header, uint8_t* out, int64_t capacity, int64_t* nbytes) {
    if (!header || !out || !nbytes) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_header: null pointer");
    int mcus_x, mcus_y;
    const int rc = check_header(*header, mcus_x, mcus_y);
    if (rc) return rc;
    Writer w = {out, 0, capacity < 0 ? 0 : capacity, 0, 0};
    put_header(w, *header);
    if (w.p > capacity) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_header: capacity %lld below the %lld bytes of the header", (long long)capacity, (long long)w.p);
    *nbytes = w.p;
    return EP24JPEG_OK;
}

// ---- the device encoder's phases with threads as loops (csrc/jpeg_huffenc_core.h is the text both run) ----

namespace {

// the emit pass's store on the host: every word is ORed into the zeroed buffer, and a word a block claims to own must have been zero
struct EmuStore {
    uint32_t* words;
    int64_t cap;
    int bad;
    void operator()(int64_t w, uint32_t v, bool owned) {
        if (w < 0 || w >= cap || (owned && words[w])) {
            bad = 1;
            return;
        }
        words[w] |= v;
    }
};

}  // namespace

extern "C" int ep24jpeg_encode_emulate(const ep24jpeg_header* header, const int16_t* coef, int64_t ncoef, int tile, uint8_t* out,
                                       int64_t capacity, int64_t* nbytes) {
    if (!header || !coef || !out || !nbytes) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: null pointer");
    const ep24jpeg_header& h = *header;
    int mcus_x, mcus_y;
    int rc = check_header(h, mcus_x, mcus_y);
    if (rc) return rc;
    if (ncoef != h.ncoef) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: %lld coefficients given, the header holds %lld", (long long)ncoef, (long long)h.ncoef);
    if (tile < 1 || tile > 1 << 20) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: a tile of %d blocks (1 .. 2^20)", tile);
    const int64_t bound = encode_bound(h, mcus_x, mcus_y);
    if (capacity < bound) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: capacity %lld below the bound %lld", (long long)capacity, (long long)bound);

    // the descriptor rows ep24.jpeg uploads for one image, and what the kernels make of them
    const int64_t mcus = (int64_t)mcus_x * mcus_y, ri = h.restart_interval;
    const int bpm = h.ncomp == 1 ? 1 : h.h[0] * h.v[0] + 2;
    const int64_t nblocks = mcus * bpm, nseg = ri ? (mcus + ri - 1) / ri : 1;
    int64_t rows[2 * EP24HUFFENC_DESC] = {0};
    rows[2] = h.ncomp, rows[3] = h.h[0], rows[4] = h.v[0], rows[5] = mcus_x, rows[6] = mcus_y, rows[7] = ri;
    for (int c = 1; c < h.ncomp; ++c) rows[8 + c] = rows[8 + c - 1] + h.nblocks[c - 1];
    rows[EP24HUFFENC_DESC] = nblocks, rows[EP24HUFFENC_DESC + 1] = nseg;
    ep24huffenc_image I;
    if (!ep24huffenc_load(rows, nblocks, nseg, ncoef, I)) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: the descriptor does not fit the header");
    uint32_t tab[EP24HUFFENC_TABLE] = {0};
    for (int i = 0; i < EP24HUFFENC_ENTRIES; ++i) ep24huffenc_fill(tab, i);

    // count: every block on its own
    std::vector<int64_t> pos((size_t)nblocks);
    int status = 0;
    for (int64_t q = 0; q < nblocks; ++q) {
        const ep24huffenc_where W = ep24huffenc_locate(I, q);
        ep24huffenc_counter cnt = {0};
        status |= ep24huffenc_block(coef + W.at, W.pred_at < 0 ? 0 : coef[W.pred_at], tab + EP24HUFFENC_DC(W.chroma), tab + EP24HUFFENC_AC(W.chroma), cnt);
        pos[(size_t)q] = cnt.bits;
    }
    if (status & EP24HUFFENC_BAD_DC) return fail(EP24JPEG_E_ARG, "jpeg encode: a DC difference is outside baseline's +-2047");
    if (status & EP24HUFFENC_BAD_AC) return fail(EP24JPEG_E_ARG, "jpeg encode: an AC coefficient is outside baseline's +-1023");
    // scan: inclusive sums over the image, then the segments' bits and first words
    for (int64_t q = 1; q < nblocks; ++q) pos[(size_t)q] += pos[(size_t)q - 1];
    std::vector<int64_t> seg((size_t)nseg * 2);
    int64_t nwords = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = s * ri * bpm, e = ri && (s + 1) * ri * bpm < nblocks ? (s + 1) * ri * bpm : nblocks;
        const int64_t bits = pos[(size_t)e - 1] - (b ? pos[(size_t)b - 1] : 0);
        seg[(size_t)(2 * s)] = nwords, seg[(size_t)(2 * s + 1)] = bits;
        nwords += (bits + 31) >> 5;
    }
    // emit: the last tile first, and the last block of a tile first
    std::vector<uint32_t> words((size_t)nwords, 0u);
    EmuStore st = {words.data(), nwords, 0};
    for (int64_t t0 = (nblocks - 1) / tile * tile; t0 >= 0; t0 -= tile)
        for (int64_t q = (t0 + tile < nblocks ? t0 + tile : nblocks) - 1; q >= t0; --q) {
            const ep24huffenc_where W = ep24huffenc_locate(I, q);
            const int64_t in_seg = (q ? pos[(size_t)q - 1] : 0) - (W.seg_block ? pos[(size_t)W.seg_block - 1] : 0);
            ep24huffenc_emitter<EmuStore> em;
            em.begin(32 * seg[(size_t)(2 * W.seg)] + in_seg, &st);
            ep24huffenc_block(coef + W.at, W.pred_at < 0 ? 0 : coef[W.pred_at], tab + EP24HUFFENC_DC(W.chroma), tab + EP24HUFFENC_AC(W.chroma), em);
            if (W.seg_last) em.pad();
            em.finish();
        }
    if (st.bad) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: the emit pass left its words (count and emit disagree)");
    // stuff: count per chunk, sum, scatter - the last chunk first
    const int64_t nchunks = (nwords + EP24HUFFENC_CHUNK_WORDS - 1) / EP24HUFFENC_CHUNK_WORDS;
    std::vector<int64_t> at((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        ep24huffenc_byte_counter bc = {0};
        const int64_t w1 = (c + 1) * EP24HUFFENC_CHUNK_WORDS;
        ep24huffenc_chunk(words.data(), seg.data(), nseg, c * EP24HUFFENC_CHUNK_WORDS, w1 < nwords ? w1 : nwords, bc);
        at[(size_t)c + 1] = at[(size_t)c] + bc.n;
    }
    Writer w = {out, 0, capacity, 0, 0};
    put_header(w, h);
    const int64_t scan_bytes = at[(size_t)nchunks];
    if (w.p + scan_bytes + 2 > capacity) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: the stream outgrew its bound");
    for (int64_t c = nchunks - 1; c >= 0; --c) {
        ep24huffenc_byte_writer bw = {out + w.p, at[(size_t)c], scan_bytes, 0};
        const int64_t w1 = (c + 1) * EP24HUFFENC_CHUNK_WORDS;
        ep24huffenc_chunk(words.data(), seg.data(), nseg, c * EP24HUFFENC_CHUNK_WORDS, w1 < nwords ? w1 : nwords, bw);
        if (bw.dropped || bw.p != at[(size_t)c + 1]) return fail(EP24JPEG_E_ARG, "ep24jpeg_encode_emulate: the stuff passes disagree");
    }
    w.p += scan_bytes;
    put_u16(w, 0xFFD9);
    *nbytes = w.p;
    return EP24JPEG_OK;
}

extern "C" int ep24jpeg_abi_version(void) { return EP24JPEG_ABI_VERSION; }
extern "C" const char* ep24jpeg_last_error(void) { return g_err; }

extern "C" int ep24jpeg_parse(const uint8_t* bytes, int64_t n, ep24jpeg_header* header_out) {
    if (!bytes || !header_out || n < 0) return fail(EP24JPEG_E_ARG, "ep24jpeg_parse: null pointer or negative length");
    Parsed P;
    const int rc = parse(bytes, n, P);
    if (rc) return rc;
    *header_out = P.hd;
    return EP24JPEG_OK;
}

extern "C" int ep24jpeg_entropy_decode(const uint8_t* bytes, int64_t n, int16_t* coef_out, int64_t capacity) {
    if (!bytes || !coef_out || n < 0) return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_decode: null pointer or negative length");
    Parsed P;
    int rc = parse(bytes, n, P);
    if (rc) return rc;
    const ep24jpeg_header& h = P.hd;
    if (capacity < h.ncoef)
        return fail(EP24JPEG_E_ARG, "ep24jpeg_entropy_decode: capacity %lld below the %lld coefficients of the file", (long long)capacity, (long long)h.ncoef);
    memset(coef_out, 0, (size_t)h.ncoef * sizeof(int16_t));
    int16_t* base[3];
    int64_t off = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        base[c] = coef_out + off;
        off += 64 * h.nblocks[c];
    }
    Bits b = {bytes, P.scan_pos, n, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const int ri = h.restart_interval;
    int rst = 0, left = ri;
    for (int my = 0; my < P.mcus_y; ++my)
        for (int mx = 0; mx < P.mcus_x; ++mx) {
            if (ri) {
                if (left == 0) {
                    // the bits of the interval end inside the byte in front of the marker, so the reader has stopped at it
                    int64_t p = b.p;
                    if (!b.stop) fill(b), p = b.p;
                    while (p + 1 < n && bytes[p] == 0xFF && bytes[p + 1] == 0xFF) ++p;      // fill bytes
                    if (!b.stop || p + 1 >= n || bytes[p] != 0xFF || bytes[p + 1] != 0xD0 + rst)
                        return fail(EP24JPEG_E_DATA, "jpeg: RST%d expected before MCU %d", rst, my * P.mcus_x + mx);
                    rst = (rst + 1) & 7;
                    b = Bits{bytes, p + 2, n, 0, 0, 0, false};
                    pred[0] = pred[1] = pred[2] = 0;
                    left = ri;
                }
                --left;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const Huff& hdc = P.dc[P.td[c]];
                const Huff& hac = P.ac[P.ta[c]];
                for (int by = 0; by < h.v[c]; ++by)
                    for (int bx = 0; bx < h.h[c]; ++bx) {
                        int16_t* blk = base[c] + ((int64_t)(my * h.v[c] + by) * h.blocks_w[c] + (mx * h.h[c] + bx)) * 64;
                        if (b.n < 32) fill(b);
                        const int t = decode_symbol(b, hdc);
                        if (t < 0 || t > 11) return fail(EP24JPEG_E_DATA, "jpeg: bad DC code in MCU %d", my * P.mcus_x + mx);
                        if (t) pred[c] += receive_extend(b, t);
                        if (pred[c] < -32768 || pred[c] > 32767) return fail(EP24JPEG_E_DATA, "jpeg: DC value out of range in MCU %d", my * P.mcus_x + mx);
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            if (b.n < 32) fill(b);
                            const int rs = decode_symbol(b, hac);
                            if (rs < 0) return fail(EP24JPEG_E_DATA, "jpeg: bad AC code in MCU %d", my * P.mcus_x + mx);
                            const int r = rs >> 4, s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;       // end of block
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(EP24JPEG_E_DATA, "jpeg: AC run past the end of a block in MCU %d", my * P.mcus_x + mx);
                            blk[ep24huff_zigzag(k)] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                        if (b.pad > b.n) return fail(EP24JPEG_E_DATA, "jpeg: the entropy-coded data ends in MCU %d of %d", my * P.mcus_x + mx, P.mcus_x * P.mcus_y);
                    }
            }
        }
    return EP24JPEG_OK;
}

// ---- the device decoder's host side: the marker walk without Huffman work, and the kernel's phases with threads as loops ----

namespace {

// the end of the restart segment that starts at p: the first FF that is not followed by 00 (or the end of the file)
int64_t segment_end(const uint8_t* d, int64_t p, int64_t n) {
    while (p < n) {
        const uint8_t* q = (const uint8_t*)memchr(d + p, 0xFF, (size_t)(n - p));
        if (!q) return n;
        p = q - d;
        if (p + 1 < n && d[p + 1] == 0) {
            p += 2;
            continue;
        }
        return p;
    }
    return n;
}

void spec_of(ep24jpeg_huff_spec& s, const Huff& h) {
    memset(&s, 0, sizeof(s));
    memcpy(s.counts, h.bits, 16);
    memcpy(s.symbols, h.vals, (size_t)h.nvals);
    s.nsymbols = h.nvals;
}

int scan_layout(const uint8_t* d, int64_t n, ep24jpeg_scan_info& I, int64_t* segs, int64_t cap) {
    Parsed P;
    const int rc = parse(d, n, P);
    if (rc) return rc;
    const ep24jpeg_header& h = P.hd;
    memset(&I, 0, sizeof(I));
    I.header = h;
    I.mcus_x = P.mcus_x;
    I.mcus_y = P.mcus_y;
    I.blocks_per_mcu = 0;
    for (int c = 0; c < h.ncomp; ++c) {
        I.blocks_per_mcu += h.h[c] * h.v[c];
        spec_of(I.dc[c], P.dc[P.td[c]]);
        spec_of(I.ac[c], P.ac[P.ta[c]]);
    }
    const int64_t mcus = (int64_t)P.mcus_x * P.mcus_y;
    const int64_t ri = h.restart_interval;
    const int64_t nseg = ri ? (mcus + ri - 1) / ri : 1;
    I.nseg = (int32_t)nseg;
    I.scan_pos = P.scan_pos;
    if (segs && cap < nseg)
        return fail(EP24JPEG_E_ARG, "ep24jpeg_scan_layout: room for %lld restart segments, the file has %lld", (long long)cap, (long long)nseg);
    int64_t p = P.scan_pos;
    int rst = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t e = segment_end(d, p, n);
        if (segs) {
            segs[3 * s] = p - P.scan_pos;
            segs[3 * s + 1] = e - p;
            segs[3 * s + 2] = ri ? (s + 1 < nseg ? ri : mcus - ri * (nseg - 1)) : mcus;
        }
        I.scan_len = e - P.scan_pos;
        if (s + 1 == nseg) break;
        int64_t q = e;
        while (q + 1 < n && d[q] == 0xFF && d[q + 1] == 0xFF) ++q;          // fill bytes
        if (q + 1 >= n || d[q] != 0xFF || d[q + 1] != 0xD0 + rst)
            return fail(EP24JPEG_E_DATA, "jpeg: RST%d expected before MCU %lld", rst, (long long)((s + 1) * ri));
        rst = (rst + 1) & 7;
        p = q + 2;
    }
    return EP24JPEG_OK;
}

inline bool same(const ep24huff_state& a, const ep24huff_state& b) { return a.pos == b.pos && a.kj == b.kj; }

}  // namespace

extern "C" int ep24jpeg_scan_layout(const uint8_t* bytes, int64_t n, ep24jpeg_scan_info* info, int64_t* segments, int64_t seg_capacity) {
    if (!bytes || !info || n < 0 || seg_capacity < 0) return fail(EP24JPEG_E_ARG, "ep24jpeg_scan_layout: null pointer or negative length");
    return scan_layout(bytes, n, *info, segments, seg_capacity);
}

extern "C" int ep24jpeg_selfsync_emulate(const uint8_t* bytes, int64_t n, int subseq_bytes, int tile, int16_t* coef_out, int64_t capacity,
                                         int32_t* rounds_out) {
    if (!bytes || !coef_out || n < 0) return fail(EP24JPEG_E_ARG, "ep24jpeg_selfsync_emulate: null pointer or negative length");
    const int S = subseq_bytes;
    if ((S != 16 && S != 32 && S != 64 && S != 128 && S != 256) || tile < 1 || tile > 1024)
        return fail(EP24JPEG_E_ARG, "ep24jpeg_selfsync_emulate: subsequences of %d bytes (16, 32, 64, 128 or 256) in tiles of %d (1 .. 1024)", S, tile);
    if (rounds_out) *rounds_out = 0;
    ep24jpeg_scan_info I;
    int rc = scan_layout(bytes, n, I, nullptr, 0);
    if (rc) return rc;
    std::vector<int64_t> segs((size_t)I.nseg * 3);
    rc = scan_layout(bytes, n, I, segs.data(), I.nseg);
    if (rc) return rc;
    const ep24jpeg_header& h = I.header;
    if (capacity < h.ncoef)
        return fail(EP24JPEG_E_ARG, "ep24jpeg_selfsync_emulate: capacity %lld below the %lld coefficients of the file", (long long)capacity, (long long)h.ncoef);
    if (I.scan_len >= EP24JPEG_MAX_SCAN)
        return fail(EP24JPEG_E_UNSUPPORTED, "jpeg: a scan of %lld bytes is above the device decoder's %d", (long long)I.scan_len, EP24JPEG_MAX_SCAN);
    memset(coef_out, 0, (size_t)h.ncoef * sizeof(int16_t));

    // setup: the tables as the kernel stages them, the image's geometry
    std::vector<ep24huff_table> tab(6);
    ep24huff_image im;
    im.d = bytes + I.scan_pos;
    for (int c = 0; c < 3; ++c) {
        const int cc = c < h.ncomp ? c : 0;
        ep24huff_build(tab[c], I.dc[cc].counts, I.dc[cc].symbols, I.dc[cc].nsymbols);
        ep24huff_build(tab[3 + c], I.ac[cc].counts, I.ac[cc].symbols, I.ac[cc].nsymbols);
    }
    im.tabs = tab.data();
    im.ncomp = h.ncomp, im.h0 = h.h[0], im.v0 = h.v[0], im.mcus_x = I.mcus_x, im.bpm = I.blocks_per_mcu;
    im.ncoef = h.ncoef;
    int64_t comp_off[3] = {0, 0, 0};
    for (int c = 1; c < h.ncomp; ++c) comp_off[c] = comp_off[c - 1] + 64 * h.nblocks[c - 1];
    im.off1 = comp_off[1], im.off2 = comp_off[2];
    // the segment table with its cumulative subsequence count, as ep24.jpeg.pack uploads it
    const int nseg = I.nseg;
    std::vector<ep24huff_segment> sg((size_t)nseg);
    std::vector<int64_t> first((size_t)nseg + 1);
    int64_t mcu = 0;
    first[0] = 0;
    for (int s = 0; s < nseg; ++s) {
        sg[s].off = (uint32_t)segs[3 * s];
        sg[s].end = (uint32_t)(segs[3 * s] + segs[3 * s + 1]);
        sg[s].first_mcu = (int32_t)mcu;
        sg[s].expect = (int32_t)(segs[3 * s + 2] * im.bpm);
        mcu += segs[3 * s + 2];
        const int64_t ns = (segs[3 * s + 1] + S - 1) / S;
        first[s + 1] = first[s] + (ns < 1 ? 1 : ns);
    }
    const int64_t total = first[nseg];

    std::vector<ep24huff_state> start((size_t)tile), end((size_t)tile), prev((size_t)tile);
    std::vector<int> begun((size_t)tile), incl((size_t)tile), seg_of((size_t)tile);
    ep24huff_state carry = {0, 0};
    int carry_blocks = 0, status = 0, max_rounds = 0;
    int s_hint = 0;
    for (int64_t t0 = 0; t0 < total; t0 += tile) {
        const int act = (int)(total - t0 < tile ? total - t0 : tile);
        // round 0: every thread from its anchored, carried or speculative start
        for (int i = 0; i < act; ++i) {
            const int64_t g = t0 + i;
            while (first[s_hint + 1] <= g) ++s_hint;
            const int s = s_hint;
            seg_of[i] = s;
            const int64_t li = g - first[s];
            if (li == 0) start[i] = ep24huff_state{sg[s].off * 8u, 0};
            else if (i == 0) start[i] = carry;
            else start[i] = ep24huff_state{ep24huff_spec_start(im.d, sg[s].off, sg[s].off + (uint32_t)(li * S)), 0};
        }
        auto bound_of = [&](int i) {
            const int s = seg_of[i];
            const int64_t li = t0 + i - first[s];
            const int64_t b = (int64_t)sg[s].off + (li + 1) * S;
            return (uint32_t)(b < sg[s].end ? b : sg[s].end);
        };
        for (int i = 0; i < act; ++i) ep24huff_run<false>(im, sg[seg_of[i]], start[i], bound_of(i), &end[i], &begun[i], nullptr, 0, false);
        int rounds = 1;
        for (int r = 1; r <= act; ++r) {
            prev = end;                                   // what the threads read in front of the barrier
            bool decoded = false, changed = false;
            for (int i = 1; i < act; ++i) {
                if (t0 + i == first[seg_of[i]]) continue;      // anchored
                if (same(prev[i - 1], start[i])) continue;
                start[i] = prev[i - 1];
                const ep24huff_state was = end[i];
                ep24huff_run<false>(im, sg[seg_of[i]], start[i], bound_of(i), &end[i], &begun[i], nullptr, 0, false);
                decoded = true;
                if (!same(was, end[i])) changed = true;
            }
            if (decoded) ++rounds;
            if (!changed) break;
        }
        if (rounds > max_rounds) max_rounds = rounds;
        // the exclusive scan of the blocks begun, restarted at every segment, and the write pass
        int run = 0;
        for (int i = 0; i < act; ++i) run += begun[i], incl[i] = run;
        int last_excl = 0;
        for (int i = 0; i < act; ++i) {
            const int s = seg_of[i];
            const int64_t fs = first[s] > t0 ? first[s] : t0;
            const int f = (int)(fs - t0);
            const int excl = (incl[i] - begun[i]) - (incl[f] - begun[f]) + (first[s] < t0 ? carry_blocks : 0);
            const bool last = t0 + i + 1 == first[s + 1];
            if (ep24huff_run<true>(im, sg[s], start[i], bound_of(i), nullptr, nullptr, coef_out, excl, last)) status = EP24JPEG_E_DATA;
            last_excl = excl;
        }
        carry = end[act - 1];
        carry_blocks = last_excl + begun[act - 1];
    }
    // the DC pass: differences -> values per component in scan order, from zero at every restart segment
    for (int c = 0; c < h.ncomp; ++c) {
        const int hc = c ? 1 : im.h0, vc = c ? 1 : im.v0, hv = hc * vc;
        const int64_t nq = (int64_t)I.mcus_x * I.mcus_y * hv;
        const int64_t ri = h.restart_interval;
        int32_t sum = 0;
        for (int64_t q = 0; q < nq; ++q) {
            const int64_t m = q / hv;
            const int r = (int)(q - m * hv);
            if (r == 0 && (ri ? m % ri == 0 : m == 0)) sum = 0;
            const int64_t my = m / I.mcus_x, mx = m - my * I.mcus_x;
            const int by = r / hc, bx = r - by * hc;
            int16_t* at = coef_out + comp_off[c] + ((my * vc + by) * ((int64_t)I.mcus_x * hc) + (mx * hc + bx)) * 64;
            sum += *at;
            if (sum < -32768 || sum > 32767) status = EP24JPEG_E_DATA;
            *at = (int16_t)sum;
        }
    }
    if (rounds_out) *rounds_out = max_rounds;
    if (status) return fail(EP24JPEG_E_DATA, "jpeg: the device decoder's status word is set (invalid code, data ends early, or DC out of range)");
    return EP24JPEG_OK;
}
