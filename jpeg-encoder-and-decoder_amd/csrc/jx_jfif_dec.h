/*
 * jx_jfif_dec.h -- the baseline JFIF entropy decoder's routines, one source for the
 * host decoder (csrc/jpgx_jfif_read.cpp, g++) and the device decoder (csrc/jpgx_jfif_dec.hip):
 * the header walk SOI .. SOS, the decode tables of T.81 Annex C, and the decoding of one restart
 * interval (T.81 F.2.2) into the library's coefficient layout.  Plain functions, no allocation,
 * no I/O, no global state.
 *
 * The bytes are untrusted.  The rules every routine here keeps:
 *   - a byte of the file is read only at an index below the file's length (the header walk) or
 *     inside the interval's [begin, end) (the scan), both checked at the read;
 *   - a coefficient is written only into a block whose index is below the frame's block count, at
 *     an index 0 .. 63;
 *   - every loop is bounded by the bytes left, by the 16 code lengths, or by index 63;
 *   - a table index is bounded by construction (8-bit lookahead, values counted against 256);
 *   - anything else ends the routine with a status.
 */
#ifndef JX_JFIF_DEC_H
#define JX_JFIF_DEC_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/jpgx.h"

#if defined(__HIPCC__)
#define JXD_FN __host__ __device__ static inline
#else
#define JXD_FN static inline
#endif

/* one Huffman table: an 8-bit lookahead for the codes of up to 8 bits, maxcode / valoff for the
 * longer ones (T.81 F.2.2.3 with the first level in front) */
struct jxd_tab {
    uint16_t look[256];     /* length << 8 | value of the code that starts these 8 bits; 0: none */
    int32_t maxcode[17];    /* [l], l = 1 .. 16: the largest code of length l, -1: no such code  */
    int32_t valoff[17];     /* [l]: index of the first value of length l - the first code        */
    uint8_t vals[256];
};

/* what the header walk leaves */
struct jxd_frame {
    uint32_t width, height;
    uint32_t hs, vs;        /* luma sampling: 1x1, 2x1, 2x2 (chroma 1x1)                         */
    uint32_t ri;            /* DRI's interval in MCUs, 0: none                                   */
    uint32_t bpr, cpr;      /* Y blocks per block row, MCUs per MCU row                          */
    uint32_t mrows, nmcu;   /* MCU rows, MCUs                                                    */
    uint32_t nb, nbc, nblk; /* blocks: Y, per chroma plane, all                                  */
    uint32_t mpi, ni;       /* MCUs per interval (nmcu when ri = 0), intervals                   */
    uint32_t tdc[3], tac[3];/* per component: index into the four tables (class + 2 x id)        */
    uint32_t sof;           /* 0xC0 or 0xC1                                                      */
    uint64_t scan_off;      /* the first entropy-coded byte                                      */
    /* the walk's own notes (kept here, not in local arrays: a lane's arrays indexed at run time
     * would live in scratch memory on the device) */
    uint32_t cid[3], tq[3]; /* SOF: component ids and DQT selectors                              */
    uint32_t q_pq[4];       /* DQT id -> 16-bit entries?                                         */
    uint64_t q_at[4];       /* DQT id -> where its entries are in the file                       */
    uint16_t qt[2][64];     /* the tables Y and Cb / Cr select, zig-zag order as in the file     */
};

JXD_FN uint32_t jxd_u16(const uint8_t *b, size_t i) { return (uint32_t)b[i] << 8 | b[i + 1]; }

/* bits[16] / vals -> t; the caller has checked sum(bits) <= 256.  Nonzero: over-subscribed */
JXD_FN int jxd_build_table(const uint8_t *bits, const uint8_t *vals, jxd_tab *t)
{
    for (int i = 0; i < 256; i++) t->look[i] = 0;
    t->maxcode[0] = -1;
    t->valoff[0] = 0;
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= 16; l++) {
        const uint32_t n = bits[l - 1];
        t->maxcode[l] = n ? (int32_t)(code + n - 1) : -1;
        t->valoff[l] = (int32_t)k - (int32_t)code;
        if (code + n > (1u << l)) return 1;             /* more codes than l bits hold */
        if (l <= 8)
            for (uint32_t c = 0; c < n; c++) {
                const uint32_t first = (code + c) << (8 - l);
                for (uint32_t pad = 0; pad < (1u << (8 - l)); pad++)
                    t->look[first | pad] = (uint16_t)(l << 8 | vals[k + c]);
            }
        code = (code + n) << 1;
        k += n;
    }
    for (uint32_t i = 0; i < k; i++) t->vals[i] = vals[i];
    for (uint32_t i = k; i < 256; i++) t->vals[i] = 0;
    return 0;
}

/* SOI .. the end of SOS.  Accepts baseline SOF0 and SOF1 with 8-bit samples, 3 components in one
 * interleaved scan, luma sampled 1x1, 2x1 or 2x2 and chroma 1x1, width and height multiples of the
 * MCU, DQT with 8- or 16-bit entries, DHT (classes 0 / 1, ids 0 / 1), DRI; skips APPn and COM.
 * ANY = 1 (the _any entry points): any width and height 1 .. 65535; fr->width and fr->height are the
 * SOF's, the counts bpr .. nblk those of the coded frame, the size rounded up to the MCU.
 * GRAY = 1 (the _gray entry points, with ANY = 1): instead ONE component in a scan of its own, any
 * component id, Tq <= 3, sampling factors 1 .. 4 each, which are ignored: such a scan is not
 * interleaved, its MCU is one block (T.81 A.2.2) and the frame has ceil(w / 8) x ceil(h / 8) of them
 * in raster order.  hs = vs = 1, nbc = 0, DRI counts blocks, the one table is qt[0]; only the DQT and
 * the two DHT tables the component selects need to be there.
 * Returns 0 or JPGX_EJFIF_HEADER. */
template <int ANY = 0, int GRAY = 0>
JXD_FN int jxd_parse_header(const uint8_t *file, size_t len, jxd_frame *fr, jxd_tab *tabs /*[4]*/)
{
    const int bad = JPGX_EJFIF_HEADER;
    if (len < 4 || file[0] != 0xff || file[1] != 0xd8) return bad;
    size_t i = 2;
    uint32_t have_tab = 0, have_q = 0, have_sof = 0;
    /* DQT ids 0 .. 3 are noted where they are in the file and read when SOS is reached */
    fr->ri = 0;
    for (;;) {
        if (len - i < 4 || file[i] != 0xff) return bad;
        const uint32_t m = file[i + 1];
        const size_t ln = jxd_u16(file, i + 2);
        if (ln < 2 || ln > len - i - 2) return bad;
        const uint8_t *seg = file + i + 4;
        const size_t n = ln - 2;
        if (m == 0xdb) {
            size_t j = 0;
            while (j < n) {
                const uint32_t pq = seg[j] >> 4, id = seg[j] & 15u;
                if (pq > 1 || id > 3 || n - j < 1 + 64 * (size_t)(pq + 1)) return bad;
                fr->q_at[id] = i + 4 + j + 1;
                fr->q_pq[id] = pq;
                have_q |= 1u << id;
                j += 1 + 64 * (size_t)(pq + 1);
            }
        } else if (m == 0xc4) {
            size_t j = 0;
            while (j < n) {
                if (n - j < 17) return bad;
                const uint32_t tc = seg[j] >> 4, th = seg[j] & 15u;
                if (tc > 1 || th > 1) return bad;
                uint32_t total = 0;
                for (int l = 0; l < 16; l++) total += seg[j + 1 + l];
                if (total > 256 || n - j - 17 < total) return bad;
                if (jxd_build_table(seg + j + 1, seg + j + 17, tabs + (tc + 2 * th))) return bad;
                have_tab |= 1u << (tc + 2 * th);
                j += 17 + total;
            }
        } else if (GRAY && (m == 0xc0 || m == 0xc1)) {
            if (have_sof || n != 6 + 3 || seg[0] != 8 || seg[5] != 1) return bad;
            fr->sof = m;
            fr->height = jxd_u16(seg, 1);
            fr->width = jxd_u16(seg, 3);
            const uint32_t s = seg[7];
            if ((s >> 4) < 1 || (s >> 4) > 4 || (s & 15u) < 1 || (s & 15u) > 4 || seg[8] > 3) return bad;
            /* the other components' places name the one component and its table */
            fr->cid[0] = fr->cid[1] = fr->cid[2] = seg[6];
            fr->tq[0] = fr->tq[1] = fr->tq[2] = seg[8];
            fr->hs = fr->vs = 1;
            if (!fr->width || !fr->height) return bad;
            have_sof = 1;
        } else if (m == 0xc0 || m == 0xc1) {
            if (have_sof || n != 6 + 9 || seg[0] != 8 || seg[5] != 3) return bad;
            fr->sof = m;
            fr->height = jxd_u16(seg, 1);
            fr->width = jxd_u16(seg, 3);
            for (int c = 0; c < 3; c++) {
                fr->cid[c] = seg[6 + 3 * c];
                fr->tq[c] = seg[8 + 3 * c];
                if (fr->tq[c] > 3) return bad;
            }
            const uint32_t s = seg[7];
            if (s != 0x11 && s != 0x21 && s != 0x22) return bad;
            if (seg[10] != 0x11 || seg[13] != 0x11 || fr->tq[1] != fr->tq[2]) return bad;
            fr->hs = s >> 4;
            fr->vs = s & 15u;
            if (!fr->width || !fr->height) return bad;
            if (!ANY && (fr->width % (8 * fr->hs) || fr->height % (8 * fr->vs))) return bad;
            have_sof = 1;
        } else if (m == 0xdd) {
            if (n != 2) return bad;
            fr->ri = jxd_u16(seg, 0);
        } else if (GRAY && m == 0xda) {
            if (!have_sof || n != 6 || seg[0] != 1) return bad;
            const uint32_t t = seg[2];
            if (seg[1] != fr->cid[0] || (t >> 4) > 1 || (t & 15u) > 1) return bad;
            fr->tdc[0] = fr->tdc[1] = fr->tdc[2] = 0 + 2 * (t >> 4);
            fr->tac[0] = fr->tac[1] = fr->tac[2] = 1 + 2 * (t & 15u);
            if (!(have_tab >> fr->tdc[0] & 1u) || !(have_tab >> fr->tac[0] & 1u)) return bad;
            if (seg[3] != 0 || seg[4] != 63 || seg[5] != 0) return bad;       /* Ss, Se, Ah / Al */
            if (!(have_q >> fr->tq[0] & 1u)) return bad;
            const size_t at = (size_t)fr->q_at[fr->tq[0]];
            const uint32_t wide = fr->q_pq[fr->tq[0]];
            for (int k = 0; k < 64; k++)   /* both places: the table is one */
                fr->qt[0][k] = fr->qt[1][k] = (uint16_t)(wide ? jxd_u16(file, at + 2 * (size_t)k) : file[at + k]);
            fr->scan_off = i + 2 + ln;
            break;
        } else if (m == 0xda) {
            if (!have_sof || n != 10 || seg[0] != 3) return bad;
            for (int c = 0; c < 3; c++) {
                const uint32_t t = seg[2 + 2 * c];
                if (seg[1 + 2 * c] != fr->cid[c] || (t >> 4) > 1 || (t & 15u) > 1) return bad;
                fr->tdc[c] = 0 + 2 * (t >> 4);
                fr->tac[c] = 1 + 2 * (t & 15u);
                if (!(have_tab >> fr->tdc[c] & 1u) || !(have_tab >> fr->tac[c] & 1u)) return bad;
            }
            if (seg[7] != 0 || seg[8] != 63 || seg[9] != 0) return bad;       /* Ss, Se, Ah / Al */
            if (!(have_q >> fr->tq[0] & 1u) || !(have_q >> fr->tq[1] & 1u)) return bad;
            for (int t = 0; t < 2; t++) {
                const size_t at = (size_t)fr->q_at[fr->tq[t]];
                const uint32_t wide = fr->q_pq[fr->tq[t]];
                for (int k = 0; k < 64; k++)
                    fr->qt[t][k] = (uint16_t)(wide ? jxd_u16(file, at + 2 * (size_t)k) : file[at + k]);
            }
            fr->scan_off = i + 2 + ln;
            break;
        } else if (!((m >= 0xe0 && m <= 0xef) || m == 0xfe)) {
            return bad;
        }
        i += 2 + ln;
    }
    if (ANY) {
        fr->cpr = (fr->width + 8 * fr->hs - 1) / (8 * fr->hs);
        fr->mrows = (fr->height + 8 * fr->vs - 1) / (8 * fr->vs);
        fr->bpr = fr->cpr * fr->hs;
        fr->nb = fr->bpr * (fr->mrows * fr->vs);
    } else {
        fr->bpr = fr->width / 8;
        fr->cpr = fr->bpr / fr->hs;
        fr->mrows = fr->height / 8 / fr->vs;
        fr->nb = fr->bpr * (fr->height / 8);
    }
    fr->nmcu = fr->cpr * fr->mrows;
    fr->nbc = GRAY ? 0u : fr->nmcu;
    fr->nblk = fr->nb + 2 * fr->nbc;
    fr->mpi = fr->ri && fr->ri < fr->nmcu ? fr->ri : fr->nmcu;
    fr->ni = (fr->nmcu + fr->mpi - 1) / fr->mpi;
    return 0;
}

/* 0, 1, 2 for luma 1x1, 2x1, 2x2 */
JXD_FN int jxd_sample_ratio(const jxd_frame *fr) { return fr->hs == 1 ? 0 : fr->vs == 1 ? 1 : 2; }

/* a restart marker's 0xFF at p?  Such a pair cannot occur inside entropy-coded data */
JXD_FN bool jxd_is_rst(const uint8_t *file, size_t len, size_t scan_off, size_t p)
{
    return p >= scan_off && p < len && len - p > 1 && file[p] == 0xff && (file[p + 1] & 0xf8u) == 0xd0u;
}

/* the scan must leave room for EOI, which ends the file */
JXD_FN bool jxd_has_eoi(const uint8_t *file, size_t len, size_t scan_off)
{
    return len >= scan_off + 2 && file[len - 2] == 0xff && file[len - 1] == 0xd9;
}

/* MSB-first bits of [pos, end) with the byte stuffing removed on the way (T.81 F.1.2.3) */
struct jxd_bits {
    const uint8_t *d;
    size_t pos, end;
    uint64_t acc;           /* the low n bits are pending */
    uint32_t n;
    uint32_t bad;           /* an 0xFF without its 0x00 inside the interval */
};

JXD_FN void jxd_fill(jxd_bits *b)
{
    while (b->n <= 56 && b->pos < b->end) {
        const uint32_t x = b->d[b->pos++];
        if (x == 0xff) {
            if (b->pos < b->end && b->d[b->pos] == 0) {
                b->pos++;
            } else {                                    /* a marker, or the interval ends in 0xFF */
                b->bad = 1;
                b->end = b->pos;
                return;
            }
        }
        b->acc = b->acc << 8 | x;
        b->n += 8;
    }
}

/* the next symbol of table t; -1: no such code, or the bits ran out */
JXD_FN int jxd_symbol(jxd_bits *b, const jxd_tab *t)
{
    const uint32_t peek = (uint32_t)(b->n >= 16 ? b->acc >> (b->n - 16) : b->acc << (16 - b->n)) & 0xffffu;
    const uint32_t e = t->look[peek >> 8];
    uint32_t l = e >> 8, v = e & 255u;
    if (!e) {
        for (l = 9; l <= 16; l++) {
            const int32_t code = (int32_t)(peek >> (16 - l));
            if (code <= t->maxcode[l]) {
                v = t->vals[(uint32_t)(code + t->valoff[l]) & 255u];
                break;
            }
        }
        if (l > 16) return -1;
    }
    if (l > b->n) return -1;
    b->n -= l;
    return (int)v;
}

/* s more bits (1 <= s <= 16) as the value they stand for (T.81 F.2.2.1 EXTEND); ok = 0: ran out */
JXD_FN int jxd_receive(jxd_bits *b, uint32_t s, int *ok)
{
    if (s > b->n) {
        *ok = 0;
        return 0;
    }
    b->n -= s;
    const int v = (int)((uint32_t)(b->acc >> b->n) & ((1u << s) - 1u));
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

JXD_FN void jxd_zero_block(int16_t *z)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t jxd_u4 __attribute__((ext_vector_type(4)));
    const jxd_u4 zero = {0u, 0u, 0u, 0u};
    for (int r = 0; r < 8; r++) ((jxd_u4 *)z)[r] = zero;    /* blocks are 128-byte aligned on the device */
#else
    for (int k = 0; k < 64; k++) z[k] = 0;
#endif
}

/* one block (T.81 F.2.2.1, F.2.2.2): all 64 coefficients of z are written.  Nonzero: scan error */
JXD_FN int jxd_block(jxd_bits *b, const jxd_tab *dc, const jxd_tab *ac, int *pred, int16_t *z)
{
    int ok = 1;
    jxd_zero_block(z);
    if (b->n < 32) jxd_fill(b);
    const int s = jxd_symbol(b, dc);
    if (s < 0 || s > 11) return 1;
    if (s) *pred += jxd_receive(b, (uint32_t)s, &ok);
    if (!ok || *pred < -32768 || *pred > 32767) return 1;
    z[0] = (int16_t)*pred;
    uint32_t k = 1;
    while (k < 64) {
        if (b->n < 32) jxd_fill(b);
        const int rs = jxd_symbol(b, ac);
        if (rs < 0) return 1;
        const uint32_t r = (uint32_t)rs >> 4, sz = (uint32_t)rs & 15u;
        if (!sz) {
            if (r == 0) break;                          /* EOB */
            if (r != 15) return 1;
            k += 16;                                    /* ZRL */
            if (k > 64) return 1;
            continue;
        }
        k += r;
        if (k > 63 || sz > 10) return 1;
        z[k] = (int16_t)jxd_receive(b, sz, &ok);
        if (!ok) return 1;
        k++;
    }
    return 0;
}

/* The MCUs [mcu0, mcu0 + count) of the frame from the bytes [begin, end) of the file (one restart
 * interval: DC predictors start at 0), into coef = Y [nb][64] | Cb [nbc][64] | Cr [nbc][64]
 * ([3][nb][64] for 4:4:4).  The interval must hold exactly these MCUs: every byte used, fewer than
 * 8 padding bits left.  Returns 0 or JPGX_EJFIF_SCAN. */
JXD_FN int jxd_decode_interval(const uint8_t *file, size_t len, size_t begin, size_t end, const jxd_frame *fr,
                               const jxd_tab *tabs /*[4]*/, uint32_t mcu0, uint32_t count, int16_t *coef)
{
    const int bad = JPGX_EJFIF_SCAN;
    if (begin > end || end > len || mcu0 > fr->nmcu || count > fr->nmcu - mcu0) return bad;
    jxd_bits b;
    b.d = file;
    b.pos = begin;
    b.end = end;
    b.acc = 0;
    b.n = 0;
    b.bad = 0;
    const uint32_t hs = fr->hs, vs = fr->vs, bpr = fr->bpr, cpr = fr->cpr, nb = fr->nb, nbc = fr->nbc;
    const jxd_tab *ydc = tabs + fr->tdc[0], *yac = tabs + fr->tac[0];
    const jxd_tab *bdc = tabs + fr->tdc[1], *bac = tabs + fr->tac[1];
    const jxd_tab *rdc = tabs + fr->tdc[2], *rac = tabs + fr->tac[2];
    int py = 0, pb = 0, pr = 0;
    uint32_t my = mcu0 / cpr, mx = mcu0 - my * cpr;
    for (uint32_t m = 0; m < count; m++) {
        for (uint32_t dy = 0; dy < vs; dy++)
            for (uint32_t dx = 0; dx < hs; dx++) {
                const size_t blk = (size_t)(my * vs + dy) * bpr + mx * hs + dx;
                if (blk >= nb || jxd_block(&b, ydc, yac, &py, coef + blk * 64)) return bad;
            }
        const size_t cb = (size_t)my * cpr + mx;
        if (cb >= nbc) return bad;
        if (jxd_block(&b, bdc, bac, &pb, coef + ((size_t)nb + cb) * 64)) return bad;
        if (jxd_block(&b, rdc, rac, &pr, coef + ((size_t)nb + nbc + cb) * 64)) return bad;
        if (++mx == cpr) mx = 0, my++;
    }
    if (b.bad || b.pos != b.end || b.n >= 8) return bad;
    return 0;
}

/* jxd_decode_interval for the one-component frame (jxd_parse_header's GRAY): an MCU is a block, MCU m
 * is block m of coef = Y [nb][64], one predictor.  The same contract and return codes. */
JXD_FN int jxd_decode_interval_gray(const uint8_t *file, size_t len, size_t begin, size_t end, const jxd_frame *fr,
                                    const jxd_tab *tabs /*[4]*/, uint32_t mcu0, uint32_t count, int16_t *coef)
{
    const int bad = JPGX_EJFIF_SCAN;
    if (begin > end || end > len || mcu0 > fr->nmcu || count > fr->nmcu - mcu0) return bad;
    jxd_bits b;
    b.d = file;
    b.pos = begin;
    b.end = end;
    b.acc = 0;
    b.n = 0;
    b.bad = 0;
    const jxd_tab *dc = tabs + fr->tdc[0], *ac = tabs + fr->tac[0];
    const uint32_t nb = fr->nb;
    int pred = 0;
    for (uint32_t m = 0; m < count; m++) {
        const size_t blk = (size_t)mcu0 + m;
        if (blk >= nb || jxd_block(&b, dc, ac, &pred, coef + blk * 64)) return bad;
    }
    if (b.bad || b.pos != b.end || b.n >= 8) return bad;
    return 0;
}

#endif
