// Stand-alone memory-safety check of the JPEG entropy stage (jpeg_host.cpp), for a build with the host compiler's sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all jpeg_host_check.cpp jpeg_host.cpp -o jpeg_host_check
//   jpeg_host_check --all A.jpg B.jpg ... --prefix C.jpg D.jpg ... --corrupt E.jpg
//
// --all: parse + decode each file.  --prefix: every prefix of each file.  --corrupt: 2 000 seeded single-byte corruptions of the file.
// Input and output live in heap blocks of exactly their size, so a read or write one byte outside either is a sanitizer report.
// Exit 0: no crash and every return code is one of the documented ones; tests/test_jpeg_host.py runs it as a child process.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ep24_jpeg.h"

static long g_ok = 0, g_err = 0;

static bool known(int rc) { return rc == EP24JPEG_OK || rc == EP24JPEG_E_ARG || rc == EP24JPEG_E_UNSUPPORTED || rc == EP24JPEG_E_DATA; }

static int run(const uint8_t* src, size_t n) {
    uint8_t* bytes = (uint8_t*)malloc(n ? n : 1);          // exactly n bytes: an over-read is a report
    memcpy(bytes, src, n);
    ep24jpeg_header h;
    int rc = ep24jpeg_parse(bytes, (int64_t)n, &h);
    if (!known(rc)) {
        fprintf(stderr, "parse returned %d\n", rc);
        exit(2);
    }
    if (rc == EP24JPEG_OK) {
        if (h.ncoef <= 0 || h.ncoef > (int64_t)3 * (EP24JPEG_MAX_SIDE + 16) * (EP24JPEG_MAX_SIDE + 16)) {
            fprintf(stderr, "ncoef %lld out of range\n", (long long)h.ncoef);
            exit(2);
        }
        int16_t* coef = (int16_t*)malloc((size_t)h.ncoef * sizeof(int16_t));
        rc = ep24jpeg_entropy_decode(bytes, (int64_t)n, coef, h.ncoef);
        if (!known(rc)) {
            fprintf(stderr, "entropy_decode returned %d\n", rc);
            exit(2);
        }
        if (rc == EP24JPEG_OK && ep24jpeg_entropy_decode(bytes, (int64_t)n, coef, h.ncoef - 1) != EP24JPEG_E_ARG) {
            fprintf(stderr, "a short output was not refused\n");
            exit(2);
        }
        free(coef);
    }
    if (rc != EP24JPEG_OK && ep24jpeg_last_error()[0] == 0) {
        fprintf(stderr, "error %d without a message\n", rc);
        exit(2);
    }
    free(bytes);
    (rc == EP24JPEG_OK ? g_ok : g_err)++;
    return rc;
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
    for (int i = 1; i < argc; ++i) {
        if (argv[i][0] == '-' && argv[i][1] == '-') {
            mode = argv[i];
            continue;
        }
        std::vector<uint8_t> v = slurp(argv[i]);
        if (mode == "--all") {
            run(v.data(), v.size());
        } else if (mode == "--prefix") {
            for (size_t n = 0; n <= v.size(); ++n) run(v.data(), n);
        } else if (mode == "--corrupt") {
            uint64_t s = 0x9E3779B97F4A7C15ull;            // seeded: the same 2 000 corruptions in every run
            for (int k = 0; k < 2000; ++k) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const size_t pos = (size_t)((s >> 33) % v.size());
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const uint8_t val = (uint8_t)(s >> 40);
                std::vector<uint8_t> w = v;
                w[pos] = val;
                run(w.data(), w.size());
            }
        } else {
            fprintf(stderr, "usage: jpeg_host_check --all FILES --prefix FILES --corrupt FILES\n");
            return 2;
        }
    }
    printf("jpeg_host_check: %ld decoded, %ld refused or in error, no crash\n", g_ok, g_err);
    return 0;
}
