// Stand-alone memory-safety check of the JPEG entropy ENCODER (jpeg_host.cpp), for a build with the host compiler's sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all jpeg_encode_check.cpp jpeg_host.cpp -o jpeg_encode_check
//   jpeg_encode_check A.jpg B.jpg ...
//
// Every file is decoded and written again; the result must equal the file when --exact precedes it (files written with the Annex K
// Huffman tables), and must decode to the same coefficients otherwise.  Then seeded coefficient arrays at baseline's limits (DC
// differences of +-2047, AC of +-1023, long zero runs, a full block, restart intervals 1, 2 and beyond the MCU count) are written and
// decoded back, and every refusal is provoked: capacity one byte short, a coefficient out of range, an inconsistent header, a table
// entry of 0.  Header, coefficients and output live in heap blocks of exactly their size, so a read or write one byte outside any of
// them is a sanitizer report.  Exit 0: no crash, every check held; tests/test_jpeg_encode_host.py runs it as a child process.
//
// Last, the kernel's quantisation by a reciprocal (jpeg_quant.h) is compared with libjpeg's integer division exhaustively: every
// |t| <= 32 768, every qt in 1 .. 255, every reciprocal within EP24_QUANT_RCP_ULPS of the host's 1.0f / (8 qt).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include <math.h>

#include "../../include/ep24_jpeg.h"
#include "jpeg_quant.h"

static long g_files = 0, g_seeded = 0, g_refused = 0;

#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");    \
            exit(2);                  \
        }                             \
    } while (0)

// encode from exact-size heap blocks -> the file; rc_out: the return code
static std::vector<uint8_t> encode(const ep24jpeg_header& h, const int16_t* coef_src, int64_t ncoef, int* rc_out, int64_t short_by = 0) {
    ep24jpeg_header* hd = (ep24jpeg_header*)malloc(sizeof(ep24jpeg_header));
    *hd = h;
    const int64_t bound = ep24jpeg_encode_bound(hd);
    std::vector<uint8_t> file;
    if (bound < 0) {
        *rc_out = (int)bound;
        free(hd);
        return file;
    }
    int16_t* coef = (int16_t*)malloc((size_t)(ncoef > 0 ? ncoef : 1) * sizeof(int16_t));
    memcpy(coef, coef_src, (size_t)ncoef * sizeof(int16_t));
    const int64_t cap = bound - short_by;
    uint8_t* out = (uint8_t*)malloc((size_t)cap);
    int64_t n = -1;
    *rc_out = ep24jpeg_entropy_encode(hd, coef, ncoef, out, cap, &n);
    if (*rc_out == EP24JPEG_OK) {
        CHECK(n > 0 && n <= cap, "encode wrote %lld bytes into %lld", (long long)n, (long long)cap);
        file.assign(out, out + n);
    } else {
        CHECK(*rc_out == EP24JPEG_E_ARG && ep24jpeg_last_error()[0], "encode returned %d", *rc_out);
    }
    free(out);
    free(coef);
    free(hd);
    return file;
}

static std::vector<int16_t> decode(const std::vector<uint8_t>& file, ep24jpeg_header* h) {
    uint8_t* bytes = (uint8_t*)malloc(file.size() ? file.size() : 1);
    memcpy(bytes, file.data(), file.size());
    CHECK(ep24jpeg_parse(bytes, (int64_t)file.size(), h) == EP24JPEG_OK, "parse failed: %s", ep24jpeg_last_error());
    std::vector<int16_t> coef((size_t)h->ncoef);
    CHECK(ep24jpeg_entropy_decode(bytes, (int64_t)file.size(), coef.data(), h->ncoef) == EP24JPEG_OK, "decode failed: %s", ep24jpeg_last_error());
    free(bytes);
    return coef;
}

static bool same_header(const ep24jpeg_header& a, const ep24jpeg_header& b) {
    if (a.width != b.width || a.height != b.height || a.ncomp != b.ncomp || a.restart_interval != b.restart_interval || a.ncoef != b.ncoef) return false;
    for (int c = 0; c < a.ncomp; ++c)
        if (a.h[c] != b.h[c] || a.v[c] != b.v[c] || a.blocks_w[c] != b.blocks_w[c] || a.blocks_h[c] != b.blocks_h[c] ||
            a.nblocks[c] != b.nblocks[c] || memcmp(a.qt[c], b.qt[c], sizeof(a.qt[c])) != 0)
            return false;
    return true;
}

static void round_trip(const ep24jpeg_header& h, const std::vector<int16_t>& coef, const char* what) {
    int rc;
    std::vector<uint8_t> file = encode(h, coef.data(), (int64_t)coef.size(), &rc);
    CHECK(rc == EP24JPEG_OK, "%s: encode refused: %s", what, ep24jpeg_last_error());
    ep24jpeg_header hb;
    std::vector<int16_t> back = decode(file, &hb);
    CHECK(same_header(h, hb), "%s: the header did not come back", what);
    CHECK(back == coef, "%s: the coefficients did not come back", what);
}

static ep24jpeg_header make_header(int w, int h, int ncomp, int hs, int vs, int ri, int quality) {
    ep24jpeg_header hd;
    memset(&hd, 0, sizeof(hd));
    hd.width = w, hd.height = h, hd.ncomp = ncomp, hd.restart_interval = ri;
    uint16_t qt[2][64];
    CHECK(ep24jpeg_quality_tables(quality, qt) == EP24JPEG_OK, "quality_tables(%d) failed", quality);
    const int mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs);
    for (int c = 0; c < ncomp; ++c) {
        hd.h[c] = c ? 1 : hs, hd.v[c] = c ? 1 : vs;
        hd.blocks_w[c] = mx * hd.h[c], hd.blocks_h[c] = my * hd.v[c];
        hd.nblocks[c] = (int64_t)hd.blocks_w[c] * hd.blocks_h[c];
        hd.ncoef += 64 * hd.nblocks[c];
        memcpy(hd.qt[c], qt[c ? 1 : 0], sizeof(hd.qt[c]));
    }
    return hd;
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

static void seeded() {
    const int samplings[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
    const int intervals[4] = {0, 1, 2, 1000};
    for (int s = 0; s < 4; ++s)
        for (int r = 0; r < 4; ++r)
            for (int kind = 0; kind < 5; ++kind) {
                ep24jpeg_header h = make_header(37, 21, samplings[s][0], samplings[s][1], samplings[s][2], intervals[r], 75);
                std::vector<int16_t> coef((size_t)h.ncoef, 0);
                const int64_t nb = h.ncoef / 64;
                for (int64_t b = 0; b < nb; ++b) {
                    int16_t* blk = coef.data() + b * 64;
                    if (kind == 0) {                     // DC swings of +-2047 between neighbours, AC at +-1023, every coefficient set
                        blk[0] = (int16_t)((b & 1) ? 1023 : -1024);
                        for (int k = 1; k < 64; ++k) blk[k] = (int16_t)((rnd() & 1) ? 1023 : -1023);
                    } else if (kind == 1) {              // one coefficient behind a zero run of 15, 16, 31, 62, 47 or 0
                        const int runs[6] = {15, 16, 31, 62, 47, 0};        // 62: the only AC is coefficient 63 (63 zeros: kind 4)
                        blk[0] = (int16_t)((int)(rnd() % 2048) - 1024);
                        static const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
                        blk[zz[1 + runs[b % 6]]] = (int16_t)((rnd() & 1) ? 1 : -700);
                    } else if (kind == 2) {              // values whose bits are all ones: streams rich in 0xFF
                        blk[0] = (int16_t)((b & 1) ? 0 : 2047 - 1024);
                        for (int k = 1; k < 64; ++k) blk[k] = (int16_t)((1 << (1 + rnd() % 10)) - 1);
                    } else if (kind == 3) {              // sparse noise
                        blk[0] = (int16_t)((int)(rnd() % 512) - 256);
                        for (int k = 1; k < 64; ++k)
                            if (rnd() % 7 == 0) blk[k] = (int16_t)((int)(rnd() % 2047) - 1023);
                    }                                    // kind 4: all zero
                }
                round_trip(h, coef, "seeded");
                ++g_seeded;
            }
}

static void refusals() {
    ep24jpeg_header h = make_header(17, 23, 3, 2, 2, 0, 75);
    std::vector<int16_t> coef((size_t)h.ncoef, 0);
    int rc;
    encode(h, coef.data(), h.ncoef, &rc, 1);
    CHECK(rc == EP24JPEG_E_ARG, "capacity one byte short was not refused");
    ++g_refused;
    coef[0] = 2048;                                                  // first DC difference
    encode(h, coef.data(), h.ncoef, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "a DC difference of 2048 was not refused");
    coef[0] = 1024, coef[64] = -1024;                                // blocks 0 and 1 of the first MCU: -1024 - 1024
    encode(h, coef.data(), h.ncoef, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "a DC difference of -2048 was not refused");
    coef[0] = coef[64] = 0, coef[5] = 1024;
    encode(h, coef.data(), h.ncoef, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "an AC coefficient of 1024 was not refused");
    coef[5] = -1024;
    encode(h, coef.data(), h.ncoef, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "an AC coefficient of -1024 was not refused");
    coef[5] = 0;
    g_refused += 4;
    ep24jpeg_header bad[8];
    for (int i = 0; i < 8; ++i) bad[i] = h;
    bad[0].blocks_w[0] += 1;
    bad[1].ncoef -= 64;
    bad[2].ncomp = 2;
    bad[3].width = EP24JPEG_MAX_SIDE + 1;
    bad[4].h[1] = 2;
    bad[5].qt[2][63] = 0;
    bad[6].qt[0][0] = 256;
    bad[7].restart_interval = 65536;
    for (int i = 0; i < 8; ++i) {
        encode(bad[i], coef.data(), h.ncoef, &rc);
        CHECK(rc == EP24JPEG_E_ARG, "inconsistent header %d was not refused", i);
        ++g_refused;
    }
    encode(h, coef.data(), h.ncoef - 64, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "a short coefficient array was not refused");
    uint16_t qt[2][64];
    CHECK(ep24jpeg_quality_tables(0, qt) == EP24JPEG_E_ARG && ep24jpeg_quality_tables(101, qt) == EP24JPEG_E_ARG, "quality outside 1 .. 100 was not refused");
    g_refused += 2;
    encode(h, coef.data(), h.ncoef, &rc);
    CHECK(rc == EP24JPEG_OK, "the consistent header was refused: %s", ep24jpeg_last_error());
}

static long quant_exhaustive() {
    long n_checked = 0;
    for (uint32_t qt = 1; qt <= 255; ++qt) {
        const uint32_t d = 8 * qt;
        float r = 1.0f / (float)d;
        for (int k = 0; k < EP24_QUANT_RCP_ULPS; ++k) r = nextafterf(r, 0.0f);
        for (int k = -EP24_QUANT_RCP_ULPS; k <= EP24_QUANT_RCP_ULPS; ++k, r = nextafterf(r, 1.0f))
            for (uint32_t t = 0; t <= EP24_QUANT_MAX_T; ++t, ++n_checked) {
                const uint32_t n = t + (d >> 1);
                CHECK(ep24_quant_div(n, r) == n / d, "quantisation: |t| %u, qt %u, reciprocal %+d ulps: %u instead of %u", t, qt, k,
                      ep24_quant_div(n, r), n / d);
            }
    }
    return n_checked;
}

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    bool exact = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--exact") || !strcmp(argv[i], "--coefficients")) {
            exact = !strcmp(argv[i], "--exact");
            continue;
        }
        std::vector<uint8_t> file = slurp(argv[i]);
        ep24jpeg_header h;
        std::vector<int16_t> coef = decode(file, &h);
        int rc;
        std::vector<uint8_t> again = encode(h, coef.data(), h.ncoef, &rc);
        CHECK(rc == EP24JPEG_OK, "%s: encode refused: %s", argv[i], ep24jpeg_last_error());
        if (exact) CHECK(again == file, "%s: the written file differs from the one read", argv[i]);
        round_trip(h, coef, argv[i]);
        ++g_files;
    }
    seeded();
    refusals();
    const long nq = quant_exhaustive();
    printf("jpeg_encode_check: %ld files, %ld seeded arrays, %ld refusals, %ld quantisation cases, no crash\n", g_files, g_seeded, g_refused, nq);
    return 0;
}
