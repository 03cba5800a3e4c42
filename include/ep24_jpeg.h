/* ep24 - host entropy stage of the JPEG decoder and encoder: libep24jpeg.so (csrc/jpeg_host.cpp).
 *
 * A second, host-only library: no HIP runtime, no device code.  Loader processes load it without opening the GPU (they never load
 * libep24.so).  It parses a baseline JPEG file and undoes its Huffman coding; everything arithmetic (dequantisation, IDCT, chroma
 * upsampling, colour conversion) is ep24_jpeg_idct / ep24_jpeg_color of libep24.so (include/ep24.h).
 *
 * Conventions, as in ep24.h: plain C types, return 0 on success and a negative code otherwise (the EP24_E_* values of ep24.h plus
 * EP24JPEG_E_DATA), text via ep24jpeg_last_error() (per thread), no allocation of caller memory, no global state besides that text.
 *
 * Supported: SOF0, and SOF1 with 8-bit samples and Huffman coding; 1 or 3 components; luma sampling 1x1, 2x1 or 2x2 with chroma
 * 1x1; up to 4 DC and 4 AC tables, redefined anywhere before the scan; DRI and RST0-7; APPn / COM skipped; fill bytes accepted.
 * EP24JPEG_E_UNSUPPORTED (the message names the reason): progressive (SOF2), lossless and arithmetic coding, 12-bit precision,
 * 4 components, any other sampling (1x2 among them), more than one scan, width or height above EP24JPEG_MAX_SIDE.
 * EP24JPEG_E_DATA: corrupt or truncated input.  Nothing is ever read outside bytes[0, n) or written outside the given output.
 */
#ifndef EP24_JPEG_H
#define EP24_JPEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EP24JPEG_OK 0
#define EP24JPEG_E_ARG (-1)          /* = EP24_E_ARG */
#define EP24JPEG_E_UNSUPPORTED (-3)  /* = EP24_E_UNSUPPORTED */
#define EP24JPEG_E_DATA (-4)         /* corrupt or truncated file */
#define EP24JPEG_MAX_SIDE 8192
#define EP24JPEG_ABI_VERSION 1

typedef struct ep24jpeg_header {
    int32_t width, height;
    int32_t ncomp;                   /* 1 or 3 */
    int32_t restart_interval;        /* MCUs between restart markers, 0 = none */
    int32_t h[3], v[3];              /* sampling factors (a one-component file: 1 x 1) */
    int32_t blocks_w[3], blocks_h[3];/* the MCU-padded block grid of each component */
    int64_t nblocks[3];              /* blocks_w * blocks_h */
    int64_t ncoef;                   /* 64 * sum of nblocks: the int16 count ep24jpeg_entropy_decode writes */
    uint16_t qt[3][64];              /* the quantisation table of each component, natural (row-major) order */
} ep24jpeg_header;

int ep24jpeg_abi_version(void);
const char* ep24jpeg_last_error(void);

/* Reads the markers up to the start of the scan. */
int ep24jpeg_parse(const uint8_t* bytes, int64_t n, ep24jpeg_header* header_out);

/* Undoes the Huffman coding of the one scan.  coef_out[0, ncoef) is zeroed and filled: component-major, block row-major within a
 * component over the MCU-padded grid, 64 int16 per block in natural order (de-zigzagged, DC prediction undone, not dequantised).
 * capacity (in int16) below ncoef is EP24JPEG_E_ARG.  On an error the contents of coef_out are unspecified (but in bounds). */
int ep24jpeg_entropy_decode(const uint8_t* bytes, int64_t n, int16_t* coef_out, int64_t capacity);

/* ---- the writer: the host half of the baseline encoder (the arithmetic is ep24_jpeg_sample / ep24_jpeg_fdct of libep24.so) ---- */

/* jpeg_set_quality's scaling of the Annex K tables, natural order: qt[0] luminance, qt[1] chrominance.  quality 1 .. 100
 * (scale = q < 50 ? 5000 / q : 200 - 2 q; entry = (base * scale + 50) / 100 clamped to 1 .. 255); anything else: EP24JPEG_E_ARG. */
int ep24jpeg_quality_tables(int quality, uint16_t qt[2][64]);

/* The capacity in bytes ep24jpeg_entropy_encode needs for this header whatever the coefficients are (negative: the header is refused). */
int64_t ep24jpeg_encode_bound(const ep24jpeg_header* header);

/* Writes a baseline JFIF file from a header as ep24jpeg_parse fills it and coefficients in ep24jpeg_entropy_decode's layout: SOI, APP0
 * (JFIF 1.01, density 1 x 1 without a unit), one DQT segment per table in zig-zag order (one table for one component; two for three,
 * Cb and Cr sharing table 1 - three when their tables differ), SOF0, the Annex K Huffman tables as separate DHT segments (DC0, AC0,
 * DC1, AC1; two for one component), DRI when restart_interval > 0, SOS, the interleaved scan (DC prediction, run/size coding with ZRL
 * and EOB, FF 00 stuffing, 1-padding of the last byte in front of every marker, RSTn with the predictors reset), EOI.  *nbytes: the
 * file's length.  EP24JPEG_E_ARG: capacity below ep24jpeg_encode_bound, ncoef other than the header's, a header ep24jpeg_parse
 * could not have made (component count, side, sampling, block grid), a table entry outside 1 .. 255, a restart interval outside
 * 0 .. 65535, a DC difference outside +-2047 or an AC coefficient outside +-1023.  Nothing is written outside out[0, capacity). */
int ep24jpeg_entropy_encode(const ep24jpeg_header* header, const int16_t* coef, int64_t ncoef, uint8_t* out, int64_t capacity,
                            int64_t* nbytes);

#ifdef __cplusplus
}
#endif
#endif
