/*
 * jx_idct.h -- the arithmetic of the pixel half of the decoder, one source for the
 * host routine (csrc/jpgx_pixels_host.cpp, g++) and the kernels (csrc/jpgx_pixels.hip):
 * dequantisation, the 13-bit fixed-point 8-point inverse transform applied down the columns and
 * along the rows, the wrapping range limit, the triangle-filter chroma upsampling and the 16-bit
 * fixed-point YCbCr -> RGB conversion -- the integer arithmetic of libjpeg's default decoder -- and the
 * 4-, 2- and 1-point transforms of its decode at 1/2, 1/4 and 1/8 of the size.
 *
 * Every value is an int32 in two's complement that wraps: sums, products and left shifts are
 * written on uint32_t, so that no input is undefined behaviour, and >> is the arithmetic shift of
 * the int32.  The coefficients and the tables come from untrusted files: they only ever become
 * values here, never an index or an address.
 */
#ifndef JX_IDCT_H
#define JX_IDCT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define JXI_FN __host__ __device__ static inline
#else
#define JXI_FN static inline
#endif

/* natural index (row * 8 + column) of zig-zag position k */
#define JXI_ZZ_INIT                                                                              \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,     \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,     \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

#define JXI_PASS1_SHIFT 11
#define JXI_PASS2_SHIFT 18

/* the arithmetic shift of the int32 that u holds */
JXI_FN uint32_t jxi_sar(uint32_t u, int s) { return (uint32_t)((int32_t)u >> s); }

JXI_FN uint32_t jxi_dequant(int16_t coef, uint16_t q) { return (uint32_t)(int32_t)coef * (uint32_t)q; }

/* a * c mod 2^32.  M24: for |a| < 2^23 and |c| < 2^23 the same number from the 24-bit multiplier,
 * which runs at the full VALU rate on the device where the 32-bit one runs at a quarter of it */
template <int M24>
JXI_FN uint32_t jxi_mul(uint32_t a, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (M24) return (uint32_t)__mul24((int)a, (int)c);
#endif
    return a * (uint32_t)c;
}

/* T(i0..i7, s) in place.  M24 = 1 needs every input inside +-2^21, so that every number that is
 * multiplied -- an input or a sum of up to four -- is inside +-2^23; the products may still wrap.
 * Pass 2 always meets that: its inputs are int32 values shifted right by 11, inside +-2^20 whatever
 * the data.  Pass 1 meets it where no table entry is above 63 (|coefficient| <= 2^15, so |d| <= 2^15 * 63
 * < 2^21) and where JXI_SMALL holds for every dequantised coefficient d of the block. */
template <int M24>
JXI_FN void jxi_idct8(uint32_t v[8], int s)
{
    const int32_t c298 = 2446, c390 = 3196, c541 = 4433, c765 = 6270, c899 = 7373, c1175 = 9633, c1501 = 12299,
                  c1847 = 15137, c1961 = 16069, c2053 = 16819, c2562 = 20995, c3072 = 25172;
    uint32_t z1 = jxi_mul<M24>(v[2] + v[6], c541);
    const uint32_t t2 = z1 - jxi_mul<M24>(v[6], c1847), t3 = z1 + jxi_mul<M24>(v[2], c765);
    const uint32_t t0 = (v[0] + v[4]) << 13, t1 = (v[0] - v[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = jxi_mul<M24>(z3 + z4, c1175);
    a0 = jxi_mul<M24>(a0, c298);
    a1 = jxi_mul<M24>(a1, c2053);
    a2 = jxi_mul<M24>(a2, c3072);
    a3 = jxi_mul<M24>(a3, c1501);
    z1 = jxi_mul<M24>(z1, -c899);
    z2 = jxi_mul<M24>(z2, -c2562);
    z3 = jxi_mul<M24>(z3, -c1961) + z5;
    z4 = jxi_mul<M24>(z4, -c390) + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    const uint32_t r = 1u << (s - 1);
    v[0] = jxi_sar(t10 + a3 + r, s);
    v[7] = jxi_sar(t10 - a3 + r, s);
    v[1] = jxi_sar(t11 + a2 + r, s);
    v[6] = jxi_sar(t11 - a2 + r, s);
    v[2] = jxi_sar(t12 + a1 + r, s);
    v[5] = jxi_sar(t12 - a1 + r, s);
    v[3] = jxi_sar(t13 + a0 + r, s);
    v[4] = jxi_sar(t13 - a0 + r, s);
}

/* The reduced-size transforms of a 1/2, 1/4 and 1/8 scale decode (libjpeg's
 * jpeg_idct_4x4, jpeg_idct_2x2 and jpeg_idct_1x1): v[0..7] are the eight inputs, the first 4, 2 or 1
 * entries the outputs.  Pass 1 runs down the columns and pass 2 along the rows, as jxi_idct8's. */
#define JXI_PASS1_SHIFT4 12
#define JXI_PASS2_SHIFT4 19
#define JXI_PASS1_SHIFT2 13
#define JXI_PASS2_SHIFT2 20

/* v[4] is never read.  M24 = 1 needs every input inside +-2^23: each factor is one input times a
 * constant below 2^15.  Pass 2's inputs are int32 values shifted right by 12, inside +-2^19 */
template <int M24>
JXI_FN void jxi_idct4(uint32_t v[8], int s)
{
    const uint32_t tmp0 = v[0] << 14;
    const uint32_t tmp2 = jxi_mul<M24>(v[2], 15137) - jxi_mul<M24>(v[6], 6270);
    const uint32_t t10 = tmp0 + tmp2, t12 = tmp0 - tmp2;
    const uint32_t o0 = jxi_mul<M24>(v[5], 11893) + jxi_mul<M24>(v[1], 8697) - jxi_mul<M24>(v[7], 1730) -
                        jxi_mul<M24>(v[3], 17799);
    const uint32_t o2 = jxi_mul<M24>(v[3], 7373) + jxi_mul<M24>(v[1], 20995) - jxi_mul<M24>(v[7], 4176) -
                        jxi_mul<M24>(v[5], 4926);
    const uint32_t r = 1u << (s - 1);
    v[0] = jxi_sar(t10 + o2 + r, s);
    v[1] = jxi_sar(t12 + o0 + r, s);
    v[2] = jxi_sar(t12 - o0 + r, s);
    v[3] = jxi_sar(t10 - o2 + r, s);
}

/* v[2], v[4] and v[6] are never read.  M24: as jxi_idct4's; pass 2's inputs are inside +-2^18 */
template <int M24>
JXI_FN void jxi_idct2(uint32_t v[8], int s)
{
    const uint32_t t10 = v[0] << 15;
    const uint32_t o = jxi_mul<M24>(v[5], 6967) + jxi_mul<M24>(v[1], 29692) - jxi_mul<M24>(v[7], 5906) -
                       jxi_mul<M24>(v[3], 10426);
    const uint32_t r = 1u << (s - 1);
    v[0] = jxi_sar(t10 + o + r, s);
    v[1] = jxi_sar(t10 - o + r, s);
}

/* the 1-point transform of the dequantised DC d, before the range limit */
JXI_FN uint32_t jxi_idct1(uint32_t d) { return jxi_sar(d + 4u, 3); }

/* pass `pass` (1 or 2) of the N-point transform, N = 4 or 2 */
template <int N, int M24>
JXI_FN void jxi_idctn(uint32_t v[8], int pass)
{
    if (N == 4) jxi_idct4<M24>(v, pass == 1 ? JXI_PASS1_SHIFT4 : JXI_PASS2_SHIFT4);
    else jxi_idct2<M24>(v, pass == 1 ? JXI_PASS1_SHIFT2 : JXI_PASS2_SHIFT2);
}

/* -2^15 <= d < 2^15 */
#define JXI_SMALL(d) ((uint32_t)(d) + 0x8000u < 0x10000u)

JXI_FN uint32_t jxi_clamp255(uint32_t u)
{
    const int32_t x = (int32_t)u;
    return x < 0 ? 0u : x > 255 ? 255u : (uint32_t)x;
}

/* the sample of a pass-2 value x, libjpeg's wrapping table on t = x & 1023: t + 128 below 128, 255
 * below 512, 0 below 896, t - 896 from there on.  With t read as the 10-bit two's complement number
 * xs in [-512, 511] that is clamp(xs + 128, 0, 255) */
JXI_FN uint32_t jxi_range(uint32_t x)
{
    const int32_t xs = (int32_t)(x << 22) >> 22;
    return jxi_clamp255((uint32_t)(xs + 128));
}

/* Upsampling, on 0..255 samples.  c is sample i, l and r are samples i - 1 and i + 1 with the index
 * clamped to the plane: with l == c (r == c) the formulas give the edge rules, out[0] = p[0] and
 * (4 s[0] + 8) >> 4, out[2n-1] = p[n-1] and (4 s[n-1] + 7) >> 4.
 * 4:2:2 takes the samples p themselves (v2 = 0); 4:2:0 takes s = 3 p[near row] + p[far row] (v2 = 1). */
JXI_FN uint32_t jxi_vsum(uint32_t pnear, uint32_t pfar) { return 3u * pnear + pfar; }
JXI_FN uint32_t jxi_up_even(uint32_t c, uint32_t l, int v2) { return v2 ? (3u * c + l + 8u) >> 4 : (3u * c + l + 1u) >> 2; }
JXI_FN uint32_t jxi_up_odd(uint32_t c, uint32_t r, int v2) { return v2 ? (3u * c + r + 7u) >> 4 : (3u * c + r + 2u) >> 2; }

/* samples 0..255 -> the three output bytes, byte 0 = R */
JXI_FN void jxi_rgb(uint32_t y, uint32_t cb, uint32_t cr, uint32_t *r, uint32_t *g, uint32_t *b)
{
    /* k (c - 128) + 32768 = k c + (32768 - 128 k) mod 2^32 */
    *r = jxi_clamp255(y + jxi_sar(91881u * cr + (32768u - 128u * 91881u), 16));
    *g = jxi_clamp255(y + jxi_sar((0u - 22554u) * cb + (0u - 46802u) * cr + (32768u + 128u * (22554u + 46802u)), 16));
    *b = jxi_clamp255(y + jxi_sar(116130u * cb + (32768u - 128u * 116130u), 16));
}

#endif
