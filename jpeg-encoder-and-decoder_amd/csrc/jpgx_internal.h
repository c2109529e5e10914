/*
 * jpgx_internal.h -- what the library's translation units share: the launch arguments the device
 * C ABI (jpgx_device.hip) passes by value to the kernels of either implementation (jpgx_mx.hip;
 * jpgx_kernels.hip in the test-only library), the table layouts the host plan (jpgx_plan.cpp)
 * fills, and the internal entry points.  No HIP types: jpgx_plan.cpp is built without them (jx_hip.h).
 */
#ifndef JPGX_INTERNAL_H
#define JPGX_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/jpgx.h"

#define JX_WG 256           /* threads per workgroup for the transform (4 waves)           */

/* unsigned 32-bit division by a launch constant d >= 1 as a multiply-high (Granlund and
 * Montgomery's round-up method): q = (t + ((n - t) >> s1)) >> s2, t = mulhi(m, n); exact for
 * every 32-bit n.  Lets a wave find its position with a few scalar operations instead of the
 * ~35-instruction software division. */
struct jx_udiv {
    uint32_t m, s1, s2;
};
static inline struct jx_udiv jx_udiv_make(uint32_t d)
{
    unsigned l = 0;
    while (l < 32 && (1ull << l) < (unsigned long long)d) l++;
    struct jx_udiv r;
    r.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    r.s1 = l ? 1u : 0u;
    r.s2 = l ? l - 1u : 0u;
    return r;
}

struct jx_geom {
    const uint8_t *rgb;     /* pixel (0, 8*row_begin) of frame 0                          */
    int16_t *out;           /* frame 0 output [3][nb][64]                                 */
    long long in_pitch;     /* bytes                                                      */
    long long in_fstride;   /* bytes                                                      */
    long long out_fstride;  /* int16 elements                                             */
    int bpr;                /* blocks per block-row (width/8)                             */
    int nb;                 /* blocks per frame in this stripe                            */
    int nframes;
    int row0;               /* frame block-row of stripe row 0 (underflow only at row 0)  */
    uint32_t under[6];      /* the underflow pixel row, interleaved (u0 u0 u0 u1 u1 u1..)  */
    struct jx_udiv dnb, dbpr;   /* division by nb and by bpr                              */
    uint32_t mpr, nmcu;         /* true 4:2:0: MCUs per MCU row, per frame (16x16 MCUs)       */
    struct jx_udiv dmpr, dnmcu; /* division by them                                       */
};

/* Per-quality tables, device resident (one copy per quality 1..97, built once per device).
 * Column-major ([ch][u][v]) so one column's 8 entries are one scalar load. */
struct jx_qtab {
    float w[3][8][8];       /* [ch][u][v]: fp32 scale of coefficient (u,v), 1/Q folded    */
    int16_t q[2][64];       /* scaled tables, q[t][u*8+v] = Qs[u][v] as the reference
                               indexes them (src/quantise.c:58)                           */
};

/* guard band: |t - rint(t)| >= lim -> exact path.  [0] = rigorous band, [1] = FORCE_EXACT
 * (every entry -1: every coefficient takes the exact path) */
struct jx_limtab {
    float lim[3][8][8];     /* [ch][u][v] */
};

#define JX_MAXQ 97

/* k_mxs, k_mxs422, k_mxs420 (csrc/jpgx_mx.hip): the colour conversion + row DCT of each pixel row
 * is an f16 MFMA product with B split into two f16 parts: hi (its products exact) and lo, stored
 * at the hi part's scale, so R = acc_h + acc_l is one add.  Per quality, plan column n = 8c + u
 * holds the scales and guard band of coefficients (c, u, v = 0..7).  (Earlier rounds built a third
 * part and a lo part stored x 2^12; DESIGN.md 4.3 records what they measured.) */
#define JX_MX_PARTS 2       /* sizes the operand arrays of the plan / kernel interface */
struct jx_mxtab {
    float w[24][8];         /* 1/4 a(u) a(v) k(v) / Q[u][v] (row transform uses exact cosines) */
    float lsq[24][8];       /* a float <= lim^2 of the rigorous band (flag: d*d - lsq >= 0);
                               -1 with FORCE_EXACT                                            */
    int16_t q[2][64];       /* scaled tables, q[t][u*8+v] = Qs[u][v] (src/quantise.c:58)       */
    double r[2][64];        /* fl(fl(1/4 a(u) a(v)) / q[t][u*8+v]): the exact pass's fast decision */
};

/* built by blocks_gpu (jpgx_device.hip) for either launcher; every kernel's by-value argument */
struct jx_xform_args {
    struct jx_geom g;
    int quality;            /* index into the device table                                */
    int force_exact;        /* JPGX_FLAG_FORCE_EXACT: flag every coefficient              */
    int luma_only;          /* true 4:2:x; read by k_xform only: Y only, chroma from k_chroma */
    int sub;                /* set by jx_launch_alt for k_chroma: 1 = true 4:2:2, 2 = 4:2:0   */
};


#ifdef __cplusplus
extern "C" {
#endif
/* host plan (jpgx_plan.cpp) */
int jx_plan_tables(int quality, float w[3][64], float lim[3][64], int16_t q[2][64]);
/* the same for true chroma subsampling: sub 1 = 4:2:2 averages, 2 = 4:2:0 (chroma bounds) */
int jx_plan_tables_mode(int quality, int sub, float w[3][64], float lim[3][64], int16_t q[2][64]);
void jx_under_dwords(const uint8_t under[3][8], uint32_t out[6]);
/* packed-pair vs scalar transform, bit for bit (host; returns the mismatch count) */
long long jx_selftest_pk(long long nblocks, unsigned long long seed);
int jx_mx_parts(void);
int jx_mx_loexp(void);
/* the MFMA kernels' host plan: per-quality tables, f16 B operands and the band's emulation
 * self-test for k_mxs (4:4:4: operands [3 part + which][lane]), k_mxs422 and k_mxs420 (true
 * 4:2:2 / 4:2:0: operands [part][which][lane]) */
int jx_plan_tables_mx(int quality, float w[24][8], float lim[24][8], int16_t q[2][64]);
int jx_plan_tables_mx422(int quality, float w[24][8], float lim[24][8], int16_t q[2][64]);
int jx_plan_tables_mx420(int quality, float w[24][8], float lim[24][8], int16_t q[2][64]);
int jx_mx_operands(uint16_t ops[3 * JX_MX_PARTS][64][8]);
int jx_mxs_device_operands(uint16_t out[3][64][8]);   /* k_mxs's three device tiles (g_mxs_B) */
int jx_mx422_operands(uint16_t ops[JX_MX_PARTS][4][64][8]);
int jx_mx420_operands(uint16_t ops[JX_MX_PARTS][5][64][8]);
long long jx_selftest_mx(long long nblocks, unsigned long long seed, int quality,
                         long long *flagged, double *ratio);
long long jx_selftest_mx422(long long nblocks, unsigned long long seed, int quality,
                            long long *flagged, double *ratio);
long long jx_selftest_mx420(long long nblocks, unsigned long long seed, int quality,
                            long long *flagged, double *ratio);
/* device side (jpgx_mx.hip): launch the kernel of sample ratio sr (0: k_mxs, 1: k_mxs422,
 * 2: k_mxs420); the workgroup image it would upload for (force, quality), host only */
int jx_launch_mx(const struct jx_xform_args *xa, int sr, void *stream, void *ev_start, void *ev_stop);
long long jx_mx_image(int sr, int force, int quality, void *dst, long long cap);
/* the second implementation's launcher (jpgx_kernels.hip, libjpgx_alt.so only): k_xform, and for
 * sr 1 / 2 k_chroma<sr> over the nbc chroma blocks of each frame */
int jx_launch_alt(const struct jx_xform_args *xa, int sr, size_t nbc, void *stream, void *ev_start, void *ev_stop);
/* the JFIF writer's tables and header bytes (host/jpgx_jfif.c), shared by the host scan writer
 * (csrc/jpgx_jfif_write.cpp: jpgx_write_jfif_opt and the entry points before it) and the device
 * coder (csrc/jpgx_jfif.hip).  What the two code with them -- a block's symbols, the clamps, the
 * scan order -- is csrc/jx_jfif_enc.h, included by both.
 * jx_jfif_build_codes: the canonical Huffman codes (T.81 Annex C) of the table bits[16] / vals,
 * indexed by symbol, packed code << 8 | length (0: the table has no such symbol).
 * jx_jfif_codes: the same for the Annex K.3 tables; cl[0] DC luminance, cl[1] AC luminance, cl[2] DC
 * chrominance, cl[3] AC chrominance.
 * jx_jfif_header: SOI .. SOS for a width x height frame of `quality`, Y sampled hs x vs by
 * sample_ratio (0: 1x1, 1: 2x1, 2: 2x2), with a DRI segment of `ri` MCUs when ri != 0.  Writes
 * the first `cap` of them into out and returns their number (at most JX_JFIF_HDR_MAX; 0 when
 * the quality is outside 1..97). */
#define JX_JFIF_HDR_MAX 768
void jx_jfif_build_codes(const uint8_t bits[16], const uint8_t *vals, uint32_t cl[256]);
void jx_jfif_codes(uint32_t cl[4][256]);
size_t jx_jfif_header(int width, int height, int quality, int sample_ratio, unsigned ri,
                      uint8_t *out, size_t cap);
/* The same with the four DHT segments (DC luminance, AC luminance, DC chrominance, AC chrominance)
 * holding bits[k] / vals[k] (bits NULL: the Annex K.3 tables, i.e. jx_jfif_header); *dht_at, when
 * asked for, is where the first DHT segment begins: the bytes before it and the bytes after the
 * fourth segment (DRI, SOS) do not depend on the tables.  The K.3 segments are JX_JFIF_DHT_STD
 * bytes together; no table of jx_jfif_optimal is longer (DC <= 12 values, AC <= 162). */
#define JX_JFIF_DHT_STD 432
size_t jx_jfif_header_tabs(int width, int height, int quality, int sample_ratio, unsigned ri,
                           const uint8_t bits[4][16], const uint8_t vals[4][256], uint8_t *out,
                           size_t cap, size_t *dht_at);
/* jx_jfif_optimal: a table for the symbol counts by T.81 Annex K.2, stated exactly because the
 * device coder (k_jf_tables, csrc/jpgx_jfif.hip) reproduces it bit for bit.
 * Figure K.1: freq[0..255] = counts, freq[256] = 1 (the reserved point: no code is all ones).
 * v1 = the index of the least nonzero freq, on a tie the largest index; v2 = the same among the
 * indices != v1; none: done.  freq[v1] += freq[v2], freq[v2] = 0 (64-bit sums); codesize + 1 along
 * v1's `others` chain, the chain's end linked to v2, codesize + 1 along v2's chain.
 * Figure K.2: the number of codes of each size (sizes up to 256: the array is sized by the symbol
 * count, not by 32).  Figure K.3: from the deepest size i down to 17, while bits[i] > 0:
 * j = i - 2 stepped down to the first nonzero bits[j]; bits[i] -= 2, bits[i - 1]++,
 * bits[j + 1] += 2, bits[j]--.  Then the reserved point leaves the largest nonzero size <= 16.
 * Figure K.4: vals = the symbols 0..255 with codesize > 0, ordered by codesize, then by value.
 * Returns the number of values (0 when every count is 0). */
int jx_jfif_optimal(const uint64_t counts[256], uint8_t bits[16], uint8_t vals[256]);
#ifdef __cplusplus
}
#endif

#endif
