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

/* ---- the host side of the DEVICE entropy decoder (ep24_jpeg_huffman / ep24_jpeg_dc of libep24.so; DESIGN.md, "JPEG decode: Huffman
 * stage on the GPU"): the marker walk without any Huffman work, and the kernel's phases run on the host ---- */

#define EP24JPEG_MAX_SCAN (1 << 28)  /* the device decoder addresses the bits of a scan in 32 bits */

typedef struct ep24jpeg_huff_spec {
    uint8_t counts[16];              /* codes of length 1 .. 16 */
    uint8_t symbols[256];
    int32_t nsymbols;
} ep24jpeg_huff_spec;

typedef struct ep24jpeg_scan_info {
    ep24jpeg_header header;
    int32_t mcus_x, mcus_y;
    int32_t blocks_per_mcu;
    int32_t nseg;                    /* restart segments the scan must hold: ceil(MCUs / restart_interval), 1 without restarts */
    int64_t scan_pos, scan_len;      /* the entropy-coded data: bytes[scan_pos, scan_pos + scan_len), up to the end of the last segment */
    ep24jpeg_huff_spec dc[3], ac[3]; /* the tables of each component as the file specifies them */
} ep24jpeg_scan_info;

/* ep24jpeg_parse plus what the device needs to decode the one scan.  segments (may be null: only info is filled) receives nseg rows of
 * {byte offset relative to scan_pos, length in bytes, MCUs the segment must hold}; seg_capacity (in rows) below nseg is EP24JPEG_E_ARG.
 * A segment ends in front of the first FF that is not followed by 00; between two segments the walk accepts fill bytes and wants RSTn
 * in sequence (EP24JPEG_E_DATA otherwise, as ep24jpeg_entropy_decode: "RSTn expected"), so a file with fewer segments than nseg is
 * refused here.  Like ep24jpeg_entropy_decode it does not look behind the last segment: a file whose EOI is missing is accepted. */
int ep24jpeg_scan_layout(const uint8_t* bytes, int64_t n, ep24jpeg_scan_info* info, int64_t* segments, int64_t seg_capacity);

/* The device decoder with threads as loops (csrc/jpeg_huff_core.h is the text both run): subsequences of subseq_bytes (16, 32, 64, 128
 * or 256) in tiles of `tile` (1 .. 1024) threads, speculative round 0, rounds until no end state changes, write pass, DC pass.  Output
 * and codes as ep24jpeg_entropy_decode, with one difference in what is accepted: bytes left over at the end of a restart segment,
 * behind the blocks it must hold, are ignored here, where ep24jpeg_entropy_decode wants the marker within its next refill ("RSTn
 * expected") - 47 of 2 000 single-byte corruptions of a file with restart markers (csrc/jpeg_device_check.cpp --corrupt-rst).  *rounds_out (may be null): the largest number of rounds in which any thread of a tile decoded (round 0 included). */
int ep24jpeg_selfsync_emulate(const uint8_t* bytes, int64_t n, int subseq_bytes, int tile, int16_t* coef_out, int64_t capacity,
                              int32_t* rounds_out);

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

/* The bytes ep24jpeg_entropy_encode writes in front of the entropy-coded data: SOI up to and including the SOS header (it calls this
 * routine's text).  *nbytes: their count (below 1 KiB).  EP24JPEG_E_ARG: a header ep24jpeg_entropy_encode refuses, or capacity below
 * the count.  What the device encoder (ep24_jpeg_huffenc_count / _emit of libep24.so) leaves to the host, with the final FF D9. */
int ep24jpeg_encode_header(const ep24jpeg_header* header, uint8_t* out, int64_t capacity, int64_t* nbytes);

/* The device encoder with threads as loops (csrc/jpeg_huffenc_core.h is the text both run; DESIGN.md, "JPEG encode: Huffman stage on
 * the GPU"): count every block's bits, sum them into positions (every restart segment on a fresh 32-bit word), emit every block at its
 * position by ORing into zeroed words - the tiles of `tile` blocks (1 .. 2^20) last first, and the blocks of a tile last first - then
 * count, sum and scatter the stuffed bytes in chunks of 64 unstuffed bytes, last chunk first.  Arguments, output and codes as
 * ep24jpeg_entropy_encode, byte for byte. */
int ep24jpeg_encode_emulate(const ep24jpeg_header* header, const int16_t* coef, int64_t ncoef, int tile, uint8_t* out, int64_t capacity,
                            int64_t* nbytes);

#ifdef __cplusplus
}
#endif
#endif
