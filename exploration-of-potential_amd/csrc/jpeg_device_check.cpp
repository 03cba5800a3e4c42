// Stand-alone check of the device entropy decoder's state machine (jpeg_huff_core.h) on the host, for a build with the host
// compiler's sanitizers (the Makefile's `jpeg_device_check` target):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all jpeg_device_check.cpp jpeg_host.cpp -o jpeg_device_check
//   jpeg_device_check --all A.jpg B.jpg ... --prefix C.jpg D.jpg ... --corrupt E.jpg
//
// Every input goes through ep24jpeg_selfsync_emulate - the kernel's phases (round 0, rounds until no end state changes, tile chaining,
// write pass, DC pass) with threads as loops - at subsequences of 16 bytes in tiles of 64 and of 128 bytes in tiles of 1024, and through
// ep24jpeg_entropy_decode.  Both must reach the same verdict (OK / DATA / UNSUPPORTED) and, where it is OK, equal coefficients.
// --all: each file.  --prefix: every prefix of each file.  --corrupt: 2 000 seeded single-byte corruptions of the file (the ones
// jpeg_host_check makes).  --corrupt-rst: the same for a file with restart markers, where the one documented difference shows - bytes
// left over at the end of a restart segment, which the host decoder refuses ("RSTn expected") and the device decoder ignores: those
// inputs are counted and printed, every other disagreement is fatal as everywhere.  Input and output live in heap blocks of exactly
// their size, so a read or write one byte outside either is a sanitizer report.  Prints the largest number of rounds a tile needed per
// --all file; exit 0: no crash, no other disagreement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ep24_jpeg.h"

static long g_ok = 0, g_err = 0, g_surplus = 0;
static bool g_allow_surplus = false;      // --corrupt-rst: the one documented difference is counted, not fatal
static const int kS[2] = {16, 128}, kTile[2] = {64, 1024};

static void run(const uint8_t* src, size_t n, const char* what, int rounds[2]) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);          // exactly n bytes: an over-read is a report
    memcpy(bytes, src, n);
    ep24jpeg_header h;
    int want = ep24jpeg_parse(bytes, (int64_t)n, &h);
    int16_t* ref = nullptr;
    int64_t ncoef = 1;
    if (want == EP24JPEG_OK) {
        ncoef = h.ncoef;
        ref = (int16_t*)malloc((size_t)ncoef * sizeof(int16_t));
        want = ep24jpeg_entropy_decode(bytes, (int64_t)n, ref, ncoef);
    }
    for (int v = 0; v < 2; ++v) {
        int16_t* got = (int16_t*)malloc((size_t)ncoef * sizeof(int16_t));
        int32_t r = 0;
        const int rc = ep24jpeg_selfsync_emulate(bytes, (int64_t)n, kS[v], kTile[v], got, ref ? ncoef : 0, &r);
        rounds[v] = r;
        // a file the parser refuses never reaches the capacity check; one it accepts is given the room it asks for
        // The documented difference (include/ep24_jpeg.h): bytes left over at the end of a restart segment.  The host decoder wants the
        // marker within its next refill ("RSTn expected"); the device decoder ignores what lies behind the blocks a segment must hold.
        if (g_allow_surplus && rc == EP24JPEG_OK && want == EP24JPEG_E_DATA) {
            ep24jpeg_entropy_decode(bytes, (int64_t)n, ref, ncoef);          // its text again: the emulation has overwritten it
            if (strncmp(ep24jpeg_last_error(), "jpeg: RST", 9) == 0) {
                if (v == 0) ++g_surplus;
                free(got);
                continue;
            }
        }
        if (rc != want) {
            fprintf(stderr, "%s (%zu bytes) at S = %d: the emulation returned %d, ep24jpeg_entropy_decode %d (%s)\n", what, n, kS[v], rc, want,
                    ep24jpeg_last_error());
            exit(2);
        }
        if (rc == EP24JPEG_OK && memcmp(got, ref, (size_t)ncoef * sizeof(int16_t)) != 0) {
            int64_t at = 0;
            while (got[at] == ref[at]) ++at;
            fprintf(stderr, "%s (%zu bytes) at S = %d: coefficient %lld is %d, ep24jpeg_entropy_decode has %d\n", what, n, kS[v], (long long)at, got[at],
                    ref[at]);
            exit(2);
        }
        if (rc != EP24JPEG_OK && ep24jpeg_last_error()[0] == 0) {
            fprintf(stderr, "error %d without a message\n", rc);
            exit(2);
        }
        if (rc == EP24JPEG_OK && ep24jpeg_selfsync_emulate(bytes, (int64_t)n, kS[v], kTile[v], got, ncoef - 1, nullptr) != EP24JPEG_E_ARG) {
            fprintf(stderr, "a short output was not refused\n");
            exit(2);
        }
        free(got);
    }
    free(ref);
    free(bytes);
    (want == EP24JPEG_OK ? g_ok : g_err)++;
}

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    std::string mode;
    int rounds[2];
    for (int i = 1; i < argc; ++i) {
        if (argv[i][0] == '-' && argv[i][1] == '-') {
            mode = argv[i];
            continue;
        }
        std::vector<uint8_t> v = slurp(argv[i]);
        if (mode == "--all") {
            run(v.data(), v.size(), argv[i], rounds);
            const char* base = strrchr(argv[i], '/');
            printf("rounds %s: %d at S = 16, %d at S = 128\n", base ? base + 1 : argv[i], rounds[0], rounds[1]);
        } else if (mode == "--prefix") {
            for (size_t n = 0; n <= v.size(); ++n) run(v.data(), n, argv[i], rounds);
        } else if (mode == "--corrupt" || mode == "--corrupt-rst") {
            g_allow_surplus = mode == "--corrupt-rst";
            uint64_t s = 0x9E3779B97F4A7C15ull;            // seeded: the same 2 000 corruptions in every run
            for (int k = 0; k < 2000; ++k) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const size_t pos = (size_t)((s >> 33) % v.size());
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const uint8_t val = (uint8_t)(s >> 40);
                std::vector<uint8_t> w = v;
                w[pos] = val;
                run(w.data(), w.size(), argv[i], rounds);
            }
            g_allow_surplus = false;
        } else {
            fprintf(stderr, "usage: jpeg_device_check --all FILES --prefix FILES --corrupt FILES --corrupt-rst FILES\n");
            return 2;
        }
    }
    if (g_surplus) printf("surplus bytes in a restart segment, refused by the host decoder only: %ld inputs\n", g_surplus);
    printf("jpeg_device_check: %ld decoded, %ld refused or in error, no disagreement, no crash\n", g_ok, g_err);
    return 0;
}
