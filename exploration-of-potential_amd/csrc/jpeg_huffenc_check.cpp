// Stand-alone memory-safety check of the DEVICE entropy encoder's shared text (jpeg_huffenc_core.h), for a build with the host
// compiler's sanitizers (make jpeg_huffenc_check):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all jpeg_huffenc_check.cpp jpeg_host.cpp -o jpeg_huffenc_check
//   jpeg_huffenc_check [A.jpg B.jpg ...]
//
// The kernels' phases are driven here from the core's routines, with threads as loops: count every block, sum, emit every block at its
// position into a zeroed word buffer of EXACTLY the counted size - in scan order, in reverse and in a seeded shuffle - then count and
// scatter the stuffed bytes chunk by chunk into a buffer of exactly the counted size.  A write one word or byte outside is a sanitizer
// report; a word a block claims to own that another block wrote is an error.  The bytes must equal what ep24jpeg_entropy_encode writes
// between the SOS header and FF D9, and ep24jpeg_encode_emulate (the library's own run of the same phases) must equal it whole, at
// tiles of 1, 7, 64 and 1 024.  Cases: seeded arrays in the four samplings at restart interval 0, 1, 5 and beyond the MCU count - values
// at +-2047 / +-1023, zero runs of 15, 16, 31 and 62, a run to the end, empty blocks, streams rich in FF - crafted blocks (one of
// maximum length between empty ones, runs of empty blocks that share a word), out-of-range DC and AC (refused by both), and every file
// named on the command line, decoded first.  Exit 0: no crash, every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/ep24_jpeg.h"
#include "jpeg_huffenc_core.h"

static long g_cases = 0, g_files = 0, g_refused = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(2);                      \
        }                                 \
    } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
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

// the serial writer, from exact-size heap blocks
static std::vector<uint8_t> reference(const ep24jpeg_header& h, const std::vector<int16_t>& coef, int* rc) {
    const int64_t bound = ep24jpeg_encode_bound(&h);
    CHECK(bound > 0, "encode_bound refused: %s", ep24jpeg_last_error());
    std::vector<uint8_t> out((size_t)bound);
    int64_t n = -1;
    *rc = ep24jpeg_entropy_encode(&h, coef.data(), (int64_t)coef.size(), out.data(), bound, &n);
    if (*rc) return std::vector<uint8_t>();
    out.resize((size_t)n);
    return out;
}

static std::vector<uint8_t> emulate(const ep24jpeg_header& h, const std::vector<int16_t>& coef, int tile, int* rc) {
    const int64_t bound = ep24jpeg_encode_bound(&h);
    std::vector<uint8_t> out((size_t)bound);
    int64_t n = -1;
    *rc = ep24jpeg_encode_emulate(&h, coef.data(), (int64_t)coef.size(), tile, out.data(), bound, &n);
    if (*rc) return std::vector<uint8_t>();
    out.resize((size_t)n);
    return out;
}

struct Store {
    std::vector<uint32_t>* words;
    std::vector<uint8_t>* owner;       // 1: some block stored the word as its own
    void operator()(int64_t w, uint32_t v, bool owned) {
        CHECK(w >= 0 && w < (int64_t)words->size(), "emit: word %lld of %lld", (long long)w, (long long)words->size());
        CHECK(!(*owner)[(size_t)w] && !(owned && (*words)[(size_t)w]), "emit: word %lld is owned by one block and written by another", (long long)w);
        if (owned) (*owner)[(size_t)w] = 1;
        CHECK(((*words)[(size_t)w] & v) == 0, "emit: two blocks set the same bit of word %lld", (long long)w);
        (*words)[(size_t)w] |= v;
    }
};

// the phases from the core's routines; order: 0 scan order, 1 reverse, 2 a seeded shuffle -> the scan's bytes
static std::vector<uint8_t> phases(const ep24jpeg_header& h, const std::vector<int16_t>& coef, int order, int* status_out) {
    const int mcus_x = h.blocks_w[0] / h.h[0], mcus_y = h.blocks_h[0] / h.v[0];
    const int64_t mcus = (int64_t)mcus_x * mcus_y, ri = h.restart_interval;
    const int bpm = h.ncomp == 1 ? 1 : h.h[0] * h.v[0] + 2;
    const int64_t nblocks = mcus * bpm, nseg = ri ? (mcus + ri - 1) / ri : 1;
    std::vector<int64_t> rows(2 * EP24HUFFENC_DESC, 0);
    rows[2] = h.ncomp, rows[3] = h.h[0], rows[4] = h.v[0], rows[5] = mcus_x, rows[6] = mcus_y, rows[7] = ri;
    for (int c = 1; c < h.ncomp; ++c) rows[8 + c] = rows[8 + c - 1] + h.nblocks[c - 1];
    rows[EP24HUFFENC_DESC] = nblocks, rows[EP24HUFFENC_DESC + 1] = nseg;
    ep24huffenc_image I;
    CHECK(ep24huffenc_load(rows.data(), nblocks, nseg, (int64_t)coef.size(), I), "the descriptor of a %d x %d image was refused", h.width, h.height);
    std::vector<uint32_t> tab(EP24HUFFENC_TABLE, 0u);
    for (int i = 0; i < EP24HUFFENC_ENTRIES; ++i) ep24huffenc_fill(tab.data(), i);

    std::vector<int64_t> pos((size_t)nblocks);
    int status = 0;
    for (int64_t q = 0; q < nblocks; ++q) {
        const ep24huffenc_where W = ep24huffenc_locate(I, q);
        CHECK(W.at >= 0 && W.at + 64 <= (int64_t)coef.size() && W.pred_at < (int64_t)coef.size(), "locate left the coefficients");
        ep24huffenc_counter cnt = {0};
        status |= ep24huffenc_block(coef.data() + W.at, W.pred_at < 0 ? 0 : coef[(size_t)W.pred_at], tab.data() + EP24HUFFENC_DC(W.chroma),
                                    tab.data() + EP24HUFFENC_AC(W.chroma), cnt);
        CHECK(cnt.bits <= 1658, "a block of %d bits", cnt.bits);
        pos[(size_t)q] = cnt.bits;
    }
    *status_out = status;
    for (int64_t q = 1; q < nblocks; ++q) pos[(size_t)q] += pos[(size_t)q - 1];
    std::vector<int64_t> seg((size_t)nseg * 2);
    int64_t nwords = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = s * ri * bpm, e = ri && (s + 1) * ri * bpm < nblocks ? (s + 1) * ri * bpm : nblocks;
        const int64_t bits = pos[(size_t)e - 1] - (b ? pos[(size_t)b - 1] : 0);
        seg[(size_t)(2 * s)] = nwords, seg[(size_t)(2 * s + 1)] = bits;
        nwords += (bits + 31) >> 5;
    }
    std::vector<int64_t> perm((size_t)nblocks);
    for (int64_t q = 0; q < nblocks; ++q) perm[(size_t)q] = order == 1 ? nblocks - 1 - q : q;
    if (order == 2)
        for (int64_t q = nblocks - 1; q > 0; --q) {
            const int64_t j = rnd() % (uint32_t)(q + 1);
            const int64_t t = perm[(size_t)q];
            perm[(size_t)q] = perm[(size_t)j], perm[(size_t)j] = t;
        }
    std::vector<uint32_t> words((size_t)nwords, 0u);
    std::vector<uint8_t> owner((size_t)nwords, 0);
    Store st = {&words, &owner};
    for (int64_t i = 0; i < nblocks; ++i) {
        const int64_t q = perm[(size_t)i];
        const ep24huffenc_where W = ep24huffenc_locate(I, q);
        const int64_t in_seg = (q ? pos[(size_t)q - 1] : 0) - (W.seg_block ? pos[(size_t)W.seg_block - 1] : 0);
        ep24huffenc_emitter<Store> em;
        em.begin(32 * seg[(size_t)(2 * W.seg)] + in_seg, &st);
        ep24huffenc_block(coef.data() + W.at, W.pred_at < 0 ? 0 : coef[(size_t)W.pred_at], tab.data() + EP24HUFFENC_DC(W.chroma),
                          tab.data() + EP24HUFFENC_AC(W.chroma), em);
        const int64_t end = 32 * em.w + em.n;
        CHECK(end == 32 * seg[(size_t)(2 * W.seg)] + in_seg + (pos[(size_t)q] - (q ? pos[(size_t)q - 1] : 0)), "count and emit disagree in block %lld", (long long)q);
        if (W.seg_last) em.pad();
        em.finish();
    }
    const int64_t nchunks = (nwords + EP24HUFFENC_CHUNK_WORDS - 1) / EP24HUFFENC_CHUNK_WORDS;
    std::vector<int64_t> at((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        ep24huffenc_byte_counter bc = {0};
        const int64_t w1 = (c + 1) * EP24HUFFENC_CHUNK_WORDS;
        ep24huffenc_chunk(words.data(), seg.data(), nseg, c * EP24HUFFENC_CHUNK_WORDS, w1 < nwords ? w1 : nwords, bc);
        at[(size_t)c + 1] = at[(size_t)c] + bc.n;
    }
    std::vector<uint8_t> out((size_t)at[(size_t)nchunks]);
    for (int64_t i = 0; i < nchunks; ++i) {
        const int64_t c = order ? nchunks - 1 - i : i;
        ep24huffenc_byte_writer bw = {out.data(), at[(size_t)c], (int64_t)out.size(), 0};
        const int64_t w1 = (c + 1) * EP24HUFFENC_CHUNK_WORDS;
        ep24huffenc_chunk(words.data(), seg.data(), nseg, c * EP24HUFFENC_CHUNK_WORDS, w1 < nwords ? w1 : nwords, bw);
        CHECK(!bw.dropped && bw.p == at[(size_t)c + 1], "the stuff passes disagree in chunk %lld", (long long)c);
    }
    return out;
}

static void compare(const ep24jpeg_header& h, const std::vector<int16_t>& coef, const char* what) {
    int rc;
    const std::vector<uint8_t> ref = reference(h, coef, &rc);
    CHECK(rc == EP24JPEG_OK, "%s: the writer refused: %s", what, ep24jpeg_last_error());
    std::vector<uint8_t> head(1024);
    int64_t nh = 0;
    CHECK(ep24jpeg_encode_header(&h, head.data(), 1024, &nh) == EP24JPEG_OK && nh > 0 && nh + 2 <= (int64_t)ref.size(), "%s: encode_header failed", what);
    CHECK(memcmp(head.data(), ref.data(), (size_t)nh) == 0, "%s: encode_header differs from the writer's header", what);
    CHECK(ref[ref.size() - 2] == 0xFF && ref[ref.size() - 1] == 0xD9, "%s: no EOI", what);
    for (int order = 0; order < 3; ++order) {
        int status;
        const std::vector<uint8_t> scan = phases(h, coef, order, &status);
        CHECK(status == 0, "%s: status %d", what, status);
        CHECK(scan.size() == ref.size() - (size_t)nh - 2 && memcmp(scan.data(), ref.data() + nh, scan.size()) == 0,
              "%s: the phases in order %d differ from the writer (%zu against %zu bytes)", what, order, scan.size(), ref.size() - (size_t)nh - 2);
    }
    const int tiles[4] = {1, 7, 64, 1024};
    for (int t = 0; t < 4; ++t) {
        const std::vector<uint8_t> got = emulate(h, coef, tiles[t], &rc);
        CHECK(rc == EP24JPEG_OK && got == ref, "%s: ep24jpeg_encode_emulate at tile %d differs from the writer", what, tiles[t]);
    }
    ++g_cases;
}

static void refused(const ep24jpeg_header& h, const std::vector<int16_t>& coef, int want, const char* what) {
    int rc, status;
    reference(h, coef, &rc);
    CHECK(rc == EP24JPEG_E_ARG, "%s: the writer returned %d", what, rc);
    emulate(h, coef, 64, &rc);
    CHECK(rc == EP24JPEG_E_ARG && ep24jpeg_last_error()[0], "%s: the emulation returned %d", what, rc);
    phases(h, coef, 2, &status);
    CHECK(status & want, "%s: status %d lacks bit %d", what, status, want);
    ++g_refused;
}

static const int kSamplings[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};

static void seeded() {
    const int intervals[4] = {0, 1, 5, 1000};
    const int runs[6] = {15, 16, 31, 62, -1, 47};
    for (int s = 0; s < 4; ++s)
        for (int r = 0; r < 4; ++r)
            for (int kind = 0; kind < 5; ++kind) {
                ep24jpeg_header h = make_header(37, 21, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], intervals[r], 75);
                std::vector<int16_t> coef((size_t)h.ncoef, 0);
                const int64_t nb = h.ncoef / 64;
                for (int64_t b = 0; b < nb; ++b) {
                    int16_t* blk = coef.data() + b * 64;
                    if (kind == 0) {                     // DC differences up to +-2047, AC at +-1023, every coefficient set
                        blk[0] = (int16_t)(rnd() & 1 ? 1023 : -1024);
                        for (int k = 1; k < 64; ++k) blk[k] = (int16_t)(rnd() & 1 ? 1023 : -1023);
                    } else if (kind == 1) {              // zero runs of 15, 16, 31, 62 in front of one coefficient, a run to the end
                        blk[0] = (int16_t)((int)(rnd() % 2048) - 1024);
                        const int run = runs[b % 6];
                        if (run >= 0) blk[ep24huff_zigzag(1 + run)] = (int16_t)(rnd() & 1 ? 1 : -700);
                    } else if (kind == 2) {              // values whose bits are all ones: streams rich in FF
                        blk[0] = (int16_t)(b & 1 ? 1023 : 0);
                        for (int k = 1; k < 64; ++k) blk[k] = (int16_t)((1 << (1 + rnd() % 10)) - 1);
                    } else if (kind == 3) {              // what a photograph gives: a few small values in front
                        blk[0] = (int16_t)((int)(rnd() % 200) - 100);
                        for (int k = 1; k < 1 + (int)(rnd() % 12); ++k) blk[ep24huff_zigzag(k)] = (int16_t)((int)(rnd() % 9) - 4);
                    }                                    // kind 4: all zero - six bits a luma block, shared words
                }
                // every DC difference must stay inside +-2047: kinds 0 and 2 swing by at most 2047 by construction
                char what[96];
                snprintf(what, sizeof(what), "seeded sampling %d interval %d kind %d", s, intervals[r], kind);
                compare(h, coef, what);
            }
}

static void crafted() {
    for (int s = 0; s < 4; ++s) {
        // one block of maximum length - DC difference 2047 on the longest DC code, all 63 AC at +-1023 - between empty blocks
        ep24jpeg_header h = make_header(40, 24, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], 0, 50);
        std::vector<int16_t> coef((size_t)h.ncoef, 0);
        int16_t* blk = coef.data() + 64 * (h.nblocks[0] / 2);
        blk[0] = 2047;
        for (int k = 1; k < 64; ++k) blk[k] = (int16_t)(k & 1 ? 1023 : -1023);
        if (h.ncomp == 3) {
            int16_t* cb = coef.data() + 64 * (h.nblocks[0] + 1);
            cb[0] = -2047;
            for (int k = 1; k < 64; ++k) cb[k] = (int16_t)(k & 1 ? -1023 : 1023);
        }
        compare(h, coef, "one block of maximum length between empty blocks");
        // sizes of one block, of one MCU row, and with restart interval 1 on more than eight segments
        compare(make_header(1, 1, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], 0, 75), std::vector<int16_t>((size_t)make_header(1, 1, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], 0, 75).ncoef, 0), "1 x 1");
        ep24jpeg_header r = make_header(50, 33, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], 1, 75);
        std::vector<int16_t> rc((size_t)r.ncoef, 0);
        for (size_t i = 0; i < rc.size(); ++i) rc[i] = (int16_t)(i % 64 == 0 ? (int)(rnd() % 64) - 32 : (rnd() % 5 == 0 ? (int)(rnd() % 7) - 3 : 0));
        compare(r, rc, "restart interval 1 on 33 x 50");
    }
}

static void refusals() {
    for (int s = 0; s < 4; ++s) {
        ep24jpeg_header h = make_header(37, 21, kSamplings[s][0], kSamplings[s][1], kSamplings[s][2], s == 2 ? 3 : 0, 75);
        std::vector<int16_t> coef((size_t)h.ncoef, 0);
        std::vector<int16_t> c = coef;
        c[64 * 3] = 2048;
        refused(h, c, EP24HUFFENC_BAD_DC, "DC difference 2048");
        c = coef;
        c[64 * 3] = -2048;
        refused(h, c, EP24HUFFENC_BAD_DC, "DC difference -2048");
        c = coef;
        c[64 * 2 + 5] = 1024;
        refused(h, c, EP24HUFFENC_BAD_AC, "AC 1024");
        c = coef;
        c[64 * 2 + 63] = -1024;
        refused(h, c, EP24HUFFENC_BAD_AC, "AC -1024");
    }
}

static void file(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    ep24jpeg_header h;
    CHECK(ep24jpeg_parse(data.data(), (int64_t)data.size(), &h) == EP24JPEG_OK, "%s: parse failed: %s", path, ep24jpeg_last_error());
    std::vector<int16_t> coef((size_t)h.ncoef);
    CHECK(ep24jpeg_entropy_decode(data.data(), (int64_t)data.size(), coef.data(), h.ncoef) == EP24JPEG_OK, "%s: decode failed", path);
    compare(h, coef, path);
    ++g_files;
}

int main(int argc, char** argv) {
    seeded();
    crafted();
    refusals();
    for (int i = 1; i < argc; ++i) file(argv[i]);
    printf("no crash: %ld cases (%ld files), %ld refusals\n", g_cases, g_files, g_refused);
    return 0;
}
