// ep24 - the JPEG encoder's quantisation division by a reciprocal, shared by the kernel (jpeg_encode.hip) and the host check that
// proves it (jpeg_encode_check.cpp).
//
// libjpeg quantises a forward-DCT output t (scaled by 8) by the table entry qt as sign(t) * ((|t| + (d >> 1)) / d) with d = 8 qt.
// ep24_quant_div(n, r) is floor(n / d) for the dividend n = |t| + (d >> 1), given a float r close to 1 / d:
//
//     floor(n / d) = (uint32_t)(((float)n + 0.5f) * r)
//
// Why: (n + 0.5) / d lies at least 0.5 / d above floor(n / d) and at least 0.5 / d below floor(n / d) + 1.  n + 0.5 is exact in float
// (n < 2^23), so the computed product differs from (n + 0.5) / d by the error of r and one rounding: with r within U ulps of 1 / d that
// is below (n + 0.5) / d * (U + 1) * 2^-23 <= 33 789 / d * (U + 1) * 1.2e-7 = 0.0041 (U + 1) / d, far below 0.5 / d for U up to
// EP24_QUANT_RCP_ULPS.  The hardware reciprocal (v_rcp_f32) is within 1 ulp; 1.0f / d on the host is within half of one.
// jpeg_encode_check.cpp does not rely on this argument: it compares with the integer division for EVERY |t| <= 32 768, every qt in
// 1 .. 255 and every r from EP24_QUANT_RCP_ULPS below the host's 1.0f / d to as many above.
#ifndef EP24_JPEG_QUANT_H
#define EP24_JPEG_QUANT_H

#include <stdint.h>

#ifdef __HIPCC__
#define EP24_QUANT_FN __host__ __device__ __forceinline__
#else
#define EP24_QUANT_FN static inline
#endif

#define EP24_QUANT_MAX_T 32768       /* |t| up to here is proven; the islow forward DCT of 8-bit samples stays below 2^14 */
#define EP24_QUANT_RCP_ULPS 4        /* r may be this many units in the last place away from the correctly rounded 1 / d */

EP24_QUANT_FN uint32_t ep24_quant_div(uint32_t n, float r) { return (uint32_t)(((float)n + 0.5f) * r); }

#endif
