/*
 * jpgx_jfif.c -- the baseline JFIF writer's tables, header bytes and file-level entry points
 * (host C99).  The scan itself is written by csrc/jpgx_jfif_write.cpp on the host and by
 * csrc/jpgx_jfif.hip on the device, both from the routines of csrc/jx_jfif_enc.h and both with
 * the tables and header bytes of this file (csrc/jpgx_internal.h).
 *
 * The reference never writes a file: its huffman_encode() does not terminate and only counts
 * symbols (src/huffman.c:23-235), and its dpcm() is an alternating-sign
 * recurrence, not a DC prediction (src/dpcm.c:10-20).  This is the build's own entropy stage
 * (parity unpinned): baseline sequential DCT, 8-bit, one interleaved scan, 4:4:4
 * (the reference's output for every sample_ratio), the standard Huffman tables of ITU-T T.81
 * Annex K.3, true DC prediction per component.
 *
 * The coefficients are the reference's, quirks included, and the file describes them
 * faithfully: the DQT entries are the divisors the reference actually applied, i.e. the scaled
 * table transposed (src/quantise.c:58); when one exceeds 255 (q <= 23) the tables are 16-bit
 * and the frame is extended sequential (SOF1) instead of baseline.  A standard decoder therefore reproduces the
 * reference's pipeline output -- including the effects of its Cb sign error
 * (src/preprocess.c:161) and of the x0 = -8 last-column quirk.  AC magnitudes beyond the baseline
 * range (possible only for chroma at q >= 93 with the sign error) are clamped to it
 * (JXE_AC_MAX, csrc/jx_jfif_enc.h).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/jpgx_compat.h"
#include "../csrc/jx_consts.h"
#include "../csrc/jpgx_internal.h"
#include "../csrc/jx_frame.h"
#include "../csrc/jx_jfif_gray.h"

/* ITU-T T.81 Annex K.3, Tables K.3-K.6: code-length counts and symbol values */
static const uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
    0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52,
    0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25,
    0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8,
    0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
    0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33,
    0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18,
    0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63,
    0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7,
    0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

/* ---- header bytes (fixed-size segments before the scan) ------------------------------------ */
typedef struct {
    uint8_t *p;
    size_t n, cap;
    int overflow;
} Out;

static void put_byte(Out *o, uint8_t b)
{
    if (o->n < o->cap) o->p[o->n] = b;
    else o->overflow = 1;
    o->n++;
}

static void put_u16(Out *o, unsigned v)
{
    put_byte(o, (uint8_t)(v >> 8));
    put_byte(o, (uint8_t)v);
}

static void put_dht(Out *o, int cls_id, const uint8_t bits[16], const uint8_t *vals)
{
    int n = 0;
    for (int i = 0; i < 16; i++) n += bits[i];
    put_u16(o, 0xffc4);
    put_u16(o, (unsigned)(2 + 1 + 16 + n));
    put_byte(o, (uint8_t)cls_id);
    for (int i = 0; i < 16; i++) put_byte(o, bits[i]);
    for (int i = 0; i < n; i++) put_byte(o, vals[i]);
}

/* canonical Huffman codes (T.81 Annex C) indexed by symbol, packed: code << 8 | length */
void jx_jfif_build_codes(const uint8_t bits[16], const uint8_t *vals, uint32_t cl[256])
{
    memset(cl, 0, 256 * sizeof cl[0]);
    unsigned code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1]; i++, k++) cl[vals[k]] = (code++) << 8 | (unsigned)l;
        code <<= 1;
    }
}

void jx_jfif_codes(uint32_t cl[4][256])
{
    jx_jfif_build_codes(kDcLumBits, kDcVals, cl[0]);
    jx_jfif_build_codes(kAcLumBits, kAcLumVals, cl[1]);
    jx_jfif_build_codes(kDcChrBits, kDcVals, cl[2]);
    jx_jfif_build_codes(kAcChrBits, kAcChrVals, cl[3]);
}

/* ---- per-image tables: ITU-T T.81 Annex K.2 (see csrc/jpgx_internal.h) ---------------------- */
int jx_jfif_optimal(const uint64_t counts[256], uint8_t bits[16], uint8_t vals[256])
{
    uint64_t freq[257];
    int codesize[257], others[257];
    int nsz[258];                                          /* codes of each size: a tree of 257 leaves
                                                              is at most 256 deep */
    for (int i = 0; i < 256; i++) freq[i] = counts[i];
    freq[256] = 1;                                         /* the reserved point: no code is all ones */
    for (int i = 0; i < 257; i++) codesize[i] = 0, others[i] = -1;
    for (;;) {                                             /* Figure K.1 */
        int v1 = -1, v2 = -1;
        for (int i = 0; i < 257; i++)                      /* the least, on a tie the largest index */
            if (freq[i] && (v1 < 0 || freq[i] <= freq[v1])) v1 = i;
        for (int i = 0; i < 257; i++)
            if (freq[i] && i != v1 && (v2 < 0 || freq[i] <= freq[v2])) v2 = i;
        if (v2 < 0) break;
        freq[v1] += freq[v2];
        freq[v2] = 0;
        for (codesize[v1]++; others[v1] >= 0; codesize[v1]++) v1 = others[v1];
        others[v1] = v2;
        for (codesize[v2]++; others[v2] >= 0; codesize[v2]++) v2 = others[v2];
    }
    memset(nsz, 0, sizeof nsz);                            /* Figure K.2 */
    int deepest = 0;
    for (int i = 0; i < 257; i++)
        if (codesize[i]) {
            nsz[codesize[i]]++;
            if (codesize[i] > deepest) deepest = codesize[i];
        }
    for (int i = deepest; i > 16; i--)                     /* Figure K.3 */
        while (nsz[i] > 0) {
            int j = i - 2;
            while (j > 0 && nsz[j] == 0) j--;
            nsz[i] -= 2;
            nsz[i - 1]++;
            nsz[j + 1] += 2;
            nsz[j]--;
        }
    int last = 16;
    while (last > 0 && nsz[last] == 0) last--;
    if (last) nsz[last]--;                                 /* the reserved point leaves */
    for (int i = 0; i < 16; i++) bits[i] = (uint8_t)nsz[i + 1];
    int n = 0;                                             /* Figure K.4 */
    for (int sz = 1; sz <= deepest; sz++)
        for (int i = 0; i < 256; i++)
            if (codesize[i] == sz) vals[n++] = (uint8_t)i;
    return n;
}

/* the two DQT tables of `quality`, zig-zag order: the divisors applied (include/jpgx.h) */
int jpgx_jfif_qt(int quality, uint16_t qt[2][64])
{
    int qs[2][8][8];
    static const int scan[8][8] = JX_SCAN_ORDER_INIT;
    if (!qt) return JPGX_EARG;
    if (jpgx_scale_table(0, quality, qs[0]) || jpgx_scale_table(1, quality, qs[1])) return JPGX_EQUALITY;
    for (int t = 0; t < 2; t++)
        for (int v = 0; v < 8; v++)
            for (int u = 0; u < 8; u++) {
                const int q = qs[t][u][v];                 /* coefficient (row v, col u) was
                                                              divided by Qs[u][v] */
                qt[t][scan[v][u]] = (uint16_t)(q < 1 ? 1 : q);
            }
    return JPGX_OK;
}

/* SOI and the APP0 segment every file of this writer begins with (JFIF 1.01, aspect 1:1, no thumbnail) */
static void put_soi_app0(Out *o)
{
    put_u16(o, 0xffd8);                                    /* SOI */
    put_u16(o, 0xffe0);                                    /* APP0 JFIF 1.01 */
    put_u16(o, 16);
    put_byte(o, 'J'); put_byte(o, 'F'); put_byte(o, 'I'); put_byte(o, 'F'); put_byte(o, 0);
    put_u16(o, 0x0101);
    put_byte(o, 0);
    put_u16(o, 1);
    put_u16(o, 1);
    put_byte(o, 0); put_byte(o, 0);
}

/* SOI, APP0, DQT x 2, SOF, DHT x 4, DRI (ri != 0), SOS: see csrc/jpgx_internal.h */
size_t jx_jfif_header(int width, int height, int quality, int sample_ratio, unsigned ri,
                      uint8_t *out, size_t cap)
{
    return jx_jfif_header_tabs(width, height, quality, sample_ratio, ri, NULL, NULL, out, cap, NULL);
}

size_t jx_jfif_header_tabs(int width, int height, int quality, int sample_ratio, unsigned ri,
                           const uint8_t bits[4][16], const uint8_t vals[4][256], uint8_t *out,
                           size_t cap, size_t *dht_at)
{
    uint16_t zz[2][64];
    if (jpgx_jfif_qt(quality, zz)) return 0;
    uint32_t hs, vs;                                       /* Y sampling */
    jx_frame_sampling(sample_ratio, &hs, &vs);
    Out o = {out, 0, cap, 0};
    put_soi_app0(&o);
    /* DQT: the divisors applied.  For q <= 23 some exceed 255 (q = 1: 6050); baseline allows
     * only 8-bit tables, so then both tables are written with 16-bit precision (Pq = 1) and
     * the frame is extended sequential (SOF1, same Huffman coding), as libjpeg does. */
    int wide = 0;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++)
            if (zz[t][k] > 255) wide = 1;
    for (int t = 0; t < 2; t++) {
        put_u16(&o, 0xffdb);
        put_u16(&o, (unsigned)(2 + 1 + 64 * (wide ? 2 : 1)));
        put_byte(&o, (uint8_t)(wide << 4 | t));
        for (int k = 0; k < 64; k++) {
            if (wide) put_u16(&o, (unsigned)zz[t][k]);
            else put_byte(&o, (uint8_t)zz[t][k]);
        }
    }
    put_u16(&o, wide ? 0xffc1 : 0xffc0);                   /* SOF1 / SOF0 */
    put_u16(&o, 8 + 3 * 3);
    put_byte(&o, 8);
    put_u16(&o, (unsigned)height);
    put_u16(&o, (unsigned)width);
    put_byte(&o, 3);
    for (int c = 0; c < 3; c++) {
        put_byte(&o, (uint8_t)(c + 1));
        put_byte(&o, (uint8_t)(c ? 0x11 : (hs << 4 | vs)));   /* 0x11, 0x21 or 0x22 */
        put_byte(&o, (uint8_t)(c ? 1 : 0));
    }
    if (dht_at) *dht_at = o.n;
    if (bits) {
        put_dht(&o, 0x00, bits[0], vals[0]);
        put_dht(&o, 0x10, bits[1], vals[1]);
        put_dht(&o, 0x01, bits[2], vals[2]);
        put_dht(&o, 0x11, bits[3], vals[3]);
    } else {
        put_dht(&o, 0x00, kDcLumBits, kDcVals);
        put_dht(&o, 0x10, kAcLumBits, kAcLumVals);
        put_dht(&o, 0x01, kDcChrBits, kDcVals);
        put_dht(&o, 0x11, kAcChrBits, kAcChrVals);
    }
    if (ri) {                                              /* DRI (T.81 B.2.4.4) */
        put_u16(&o, 0xffdd);
        put_u16(&o, 4);
        put_u16(&o, ri);
    }
    put_u16(&o, 0xffda);                                   /* SOS */
    put_u16(&o, 6 + 2 * 3);
    put_byte(&o, 3);
    for (int c = 0; c < 3; c++) {
        put_byte(&o, (uint8_t)(c + 1));
        put_byte(&o, (uint8_t)(c ? 0x11 : 0x00));
    }
    put_byte(&o, 0);
    put_byte(&o, 63);
    put_byte(&o, 0);
    return o.n;
}

/* The header of a one-component file (csrc/jx_jfif_gray.h): SOI, the colour writer's APP0, one DQT
 * (table 0: jpgx_jfif_qt(quality)[0]; 16-bit and SOF1 where an entry exceeds 255, as above), SOF with
 * Nf = 1 (component 1, sampling 0x11, Tq 0), DHT DC 0x00 and AC 0x10, DRI (ri != 0, in blocks), SOS with
 * Ns = 1, Td / Ta 0 / 0, Ss 0, Se 63 */
size_t jx_jfif_header_gray(int width, int height, int quality, unsigned ri, const uint8_t bits[2][16],
                           const uint8_t vals[2][256], uint8_t *out, size_t cap, size_t *dht_at)
{
    uint16_t zz[2][64];
    if (jpgx_jfif_qt(quality, zz)) return 0;
    Out o = {out, 0, cap, 0};
    put_soi_app0(&o);
    int wide = 0;
    for (int k = 0; k < 64; k++)
        if (zz[0][k] > 255) wide = 1;
    put_u16(&o, 0xffdb);                                   /* DQT 0 */
    put_u16(&o, (unsigned)(2 + 1 + 64 * (wide ? 2 : 1)));
    put_byte(&o, (uint8_t)(wide << 4));
    for (int k = 0; k < 64; k++) {
        if (wide) put_u16(&o, (unsigned)zz[0][k]);
        else put_byte(&o, (uint8_t)zz[0][k]);
    }
    put_u16(&o, wide ? 0xffc1 : 0xffc0);                   /* SOF1 / SOF0 */
    put_u16(&o, 8 + 3);
    put_byte(&o, 8);
    put_u16(&o, (unsigned)height);
    put_u16(&o, (unsigned)width);
    put_byte(&o, 1);
    put_byte(&o, 1);
    put_byte(&o, 0x11);
    put_byte(&o, 0);
    if (dht_at) *dht_at = o.n;
    put_dht(&o, 0x00, bits ? bits[0] : kDcLumBits, bits ? vals[0] : kDcVals);
    put_dht(&o, 0x10, bits ? bits[1] : kAcLumBits, bits ? vals[1] : kAcLumVals);
    if (ri) {                                              /* DRI (T.81 B.2.4.4) */
        put_u16(&o, 0xffdd);
        put_u16(&o, 4);
        put_u16(&o, ri);
    }
    put_u16(&o, 0xffda);                                   /* SOS */
    put_u16(&o, 6 + 2);
    put_byte(&o, 1);
    put_byte(&o, 1);
    put_byte(&o, 0x00);
    put_byte(&o, 0);
    put_byte(&o, 63);
    put_byte(&o, 0);
    return o.n;
}

/* ---- the file-level entry points -------------------------------------------------------------
 * Their common frame: room for `nblocks` blocks of coefficients and for the largest file
 * (jpgx_jfif_bound), the caller's own step that fills the coefficients, then the scan -- sr 0:
 * jpgx_write_jfif, else jpgx_write_jfif_sub -- and the file.  A failed malloc is reported as
 * `nomem`, which is JPGX_ENOMEM for jpgx_encode_rgb_to_jpeg and JPGX_EARG for the two BMP entry
 * points: an inconsistency of the ABI as released, kept as it is here. */
typedef struct {
    int16_t *coef;
    uint8_t *buf;
    size_t cap;
} FileJob;

/* the blocks of the frame that sample ratio sr codes, for a size the forward path takes */
static int frame_blocks(int width, int height, const jpgx_params *p, int sr, size_t *nblocks)
{
    jx_frame f;
    int rc = jpgx_validate(width, height, p);
    if (!rc) rc = jx_frame_rc_coder(jx_frame_make(width, height, sr, &f));
    if (!rc) *nblocks = f.nblk;
    return rc;
}

static int file_begin(FileJob *j, size_t nblocks, int width, int height, int nomem)
{
    j->coef = (int16_t *)malloc(nblocks * 64 * sizeof(int16_t));
    j->cap = jpgx_jfif_bound(width, height);
    j->buf = (uint8_t *)malloc(j->cap);
    return (j->coef && j->buf) ? JPGX_OK : nomem;
}

/* rc: what came of the scan; the first len bytes of j->buf become the file, and the job ends */
static int file_put(FileJob *j, int rc, size_t len, const char *output)
{
    if (!rc) {
        FILE *f = fopen(output, "wb");
        if (!f || fwrite(j->buf, 1, len, f) != len) rc = JPGX_EARG;
        if (f && fclose(f)) rc = JPGX_EARG;
    }
    free(j->coef);
    free(j->buf);
    return rc;
}

/* rc: what came of filling j->coef */
static int file_end(FileJob *j, int rc, int width, int height, int quality, int sr, const char *output)
{
    size_t len = 0;
    if (!rc)
        rc = sr ? jpgx_write_jfif_sub(j->coef, width, height, quality, sr, j->buf, j->cap, &len)
                : jpgx_write_jfif(j->coef, width, height, quality, j->buf, j->cap, &len);
    return file_put(j, rc, len, output);
}

int jpgx_encode_rgb_to_jpeg(const uint8_t *rgb, int width, int height, size_t pitch,
                            const char *output, int quality, int sample_ratio, unsigned flags,
                            int device)
{
    if (!rgb || !output) return JPGX_EARG;
    jpgx_params p;
    jpgx_default_params(&p, width, height, quality, sample_ratio);
    /* true subsampling needs a ratio; with sample_ratio 0 the flag means plain 4:4:4 (as in
     * jpgx_encode_bmp_to_jpeg_ex) */
    const int sub = (flags & JPGX_FLAG_SUBSAMPLE) && sample_ratio != 0;
    p.flags = sub ? JPGX_FLAG_SUBSAMPLE : 0u;
    size_t nblocks;
    int rc = frame_blocks(width, height, &p, sub ? sample_ratio : 0, &nblocks);
    if (rc) return rc;
    FileJob j;
    rc = file_begin(&j, nblocks, width, height, JPGX_ENOMEM);
    if (!rc) rc = jpgx_blocks(rgb, width, height, pitch, &p, j.coef, device);
    return file_end(&j, rc, width, height, quality, sub ? sample_ratio : 0, output);
}

/* jpgx_encode_rgb_to_jpeg for an image of any width and height: the coded frame by the edge rule
 * (jpgx_pad_edge) into a staging buffer, the forward path over it, then jpgx_write_jfif_any */
int jpgx_encode_rgb_to_jpeg_any(const uint8_t *rgb, int width, int height, size_t pitch,
                                const char *output, int quality, int sample_ratio, unsigned flags,
                                int device)
{
    if (!rgb || !output) return JPGX_EARG;
    const int sub = (flags & JPGX_FLAG_SUBSAMPLE) && sample_ratio != 0;
    const int sr = sub ? sample_ratio : 0;                 /* the file's, and the coded frame's */
    if (sample_ratio < 0 || sample_ratio > 2) return JPGX_ESAMPLE;
    if (quality < 1 || quality > JX_MAXQ) return JPGX_EQUALITY;
    jx_frame_any a;
    if (jx_frame_make_any(width, height, sr, &a)) return JPGX_EGEOMETRY;
    if (pitch < (size_t)width * 3) return JPGX_EARG;
    const int cw = (int)a.c.bw * 8, ch = (int)a.c.bh * 8;
    jpgx_params p;
    jpgx_default_params(&p, cw, ch, quality, sr);
    p.flags = sub ? JPGX_FLAG_SUBSAMPLE : 0u;
    FileJob j;
    uint8_t *coded = (uint8_t *)malloc((size_t)cw * 3 * (size_t)ch);
    int rc = file_begin(&j, a.c.nblk, cw, ch, JPGX_ENOMEM);
    if (!coded) rc = JPGX_ENOMEM;
    if (!rc) rc = jpgx_pad_edge(rgb, width, height, pitch, cw, ch, coded);
    if (!rc) rc = jpgx_blocks(coded, cw, ch, (size_t)cw * 3, &p, j.coef, device);
    free(coded);
    size_t len = 0;
    if (!rc) rc = jpgx_write_jfif_any(j.coef, width, height, quality, sr, 0, 1, 0u, j.buf, j.cap, &len);
    return file_put(&j, rc, len, output);
}

int jpgx_encode_bmp_to_jpeg_ex(const char *input, const char *output, int quality,
                               int sample_ratio, unsigned flags, int device)
{
    if (!input || !output) return JPGX_EARG;
    if (!(flags & JPGX_FLAG_SUBSAMPLE) || sample_ratio == 0)
        return jpgx_encode_bmp_to_jpeg(input, output, quality, sample_ratio);
    int W = 0, H = 0;
    uint8_t *rgb = NULL;
    size_t fsize = 0;
    int rc = jpgx_bmp_read(input, &rgb, &W, &H, &fsize);
    if (rc) return rc;
    jpgx_params p;
    jpgx_default_params(&p, W, H, quality, sample_ratio);
    p.flags = flags;
    size_t nblocks;
    rc = frame_blocks(W, H, &p, sample_ratio, &nblocks);
    if (!rc) {
        FileJob j;
        rc = file_begin(&j, nblocks, W, H, JPGX_EARG);
        if (!rc) rc = jpgx_blocks(rgb, W, H, (size_t)W * 3, &p, j.coef, device);
        rc = file_end(&j, rc, W, H, quality, sample_ratio, output);
    }
    jpgx_free(rgb);
    return rc;
}

int jpgx_encode_bmp_to_jpeg(const char *input, const char *output, int quality,
                            int sample_ratio)
{
    if (!input || !output) return JPGX_EARG;
    jpgx_jpeg_data d;
    memset(&d, 0, sizeof d);
    int rc = jpgx_encode_bmp(input, quality, sample_ratio, 0, 0, &d);
    if (rc) return rc;
    const size_t nb = (size_t)d.num_blocks_Y;
    FileJob j;
    rc = file_begin(&j, nb * 3, d.width, d.height, JPGX_EARG);
    if (!rc) {
        int **zz[3] = {d.zig_zag_Y, d.zig_zag_Cb, d.zig_zag_Cr};
        for (int c = 0; c < 3; c++)
            for (size_t i = 0; i < nb; i++)
                for (int k = 0; k < 64; k++) j.coef[((size_t)c * nb + i) * 64 + k] = (int16_t)zz[c][i][k];
    }
    rc = file_end(&j, rc, d.width, d.height, quality, 0, output);
    jpgx_free_jpgdata(&d);
    return rc;
}
