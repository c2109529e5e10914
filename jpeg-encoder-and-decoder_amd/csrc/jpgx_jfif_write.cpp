/*
 * jpgx_jfif_write.cpp -- the host JFIF writer's scan: jpgx_write_jfif,
 * jpgx_write_jfif_sub, jpgx_write_jfif_ex, jpgx_write_jfif_opt, jpgx_write_jfif_any, jpgx_write_jfif_gray, jpgx_jfif_bound
 * (include/jpgx_compat.h).  What a block's symbols are, the clamps, the scan's geometry and its
 * block order are jx_jfif_enc.h's, the routines the device coder (jpgx_jfif.hip) runs; this file
 * adds the bit writer with its 0xFF stuffing, the restart-row policy and the threads.  Tables and
 * header bytes come from host/jpgx_jfif.c.  No HIP: built with g++, as jpgx_jfif_read.cpp.
 */
#include <stdlib.h>
#include <string.h>
#ifdef __SSE2__
#include <emmintrin.h>
#endif

#include "../../include/jpgx_compat.h"
#include "jpgx_internal.h"
#include "jx_consts.h"
#include "jx_jfif_enc.h"
#include "jx_jfif_gray.h"
#include "jx_par.h"

namespace {

/* ---- entropy-coded data: a word-at-a-time bit writer into a growable buffer ---------------
 * Bits accumulate MSB first in a 64-bit register; every 32 bits leave as four bytes at once
 * unless one of them is 0xFF (then byte by byte with the 0x00 stuffing of T.81 F.1.2.3). */
struct BW {
    uint8_t *p;
    size_t n, cap;
    uint64_t acc;     /* the low nacc bits are pending */
    int nacc;
    int oom;
};

int bw_reserve(BW *w, size_t more)
{
    if (w->n + more <= w->cap) return 1;
    size_t nc = w->cap ? w->cap : 1u << 16;
    while (nc < w->n + more) nc *= 2;
    uint8_t *q = (uint8_t *)realloc(w->p, nc);
    if (!q) {
        w->oom = 1;
        return 0;
    }
    w->p = q;
    w->cap = nc;
    return 1;
}

inline void bw_byte(BW *w, uint8_t b)
{
    w->p[w->n++] = b;
    if (b == 0xff) w->p[w->n++] = 0x00;
}

/* v < 2^nb, nb <= 32 (a Huffman code and its additional bits in one call); the caller has
 * reserved room (bw_reserve) */
inline void bw_bits(BW *w, uint32_t v, int nb)
{
    w->acc = (w->acc << nb) | v;
    w->nacc += nb;
    if (w->nacc >= 32) {
        w->nacc -= 32;
        const uint32_t x = (uint32_t)(w->acc >> w->nacc);
        if (((~x - 0x01010101u) & x & 0x80808080u) == 0) {       /* no 0xFF byte in x */
            uint8_t *d = w->p + w->n;
            d[0] = (uint8_t)(x >> 24);
            d[1] = (uint8_t)(x >> 16);
            d[2] = (uint8_t)(x >> 8);
            d[3] = (uint8_t)x;
            w->n += 4;
        } else {
            bw_byte(w, (uint8_t)(x >> 24));
            bw_byte(w, (uint8_t)(x >> 16));
            bw_byte(w, (uint8_t)(x >> 8));
            bw_byte(w, (uint8_t)x);
        }
    }
}

/* pad to a byte boundary with 1-bits and emit the pending bytes */
void bw_flush(BW *w)
{
    const int pad = (8 - (w->nacc & 7)) & 7;
    if (pad) {
        w->acc = (w->acc << pad) | ((1u << pad) - 1u);
        w->nacc += pad;
    }
    while (w->nacc >= 8) {
        w->nacc -= 8;
        bw_byte(w, (uint8_t)(w->acc >> w->nacc));
    }
}

/* worst-case coded bytes of one block, stuffing included */
#define JX_BLOCK_MAX (2 * (22 + 63 * 26 + 11 + 8) / 8 + 16)

/* bit k set: z[k] != 0 */
inline uint64_t nonzero_mask(const int16_t *z)
{
#ifdef __SSE2__
    const __m128i zero = _mm_setzero_si128();
    uint64_t m = 0;
    for (int i = 0; i < 4; i++) {
        const __m128i a = _mm_loadu_si128((const __m128i *)(z + 16 * i));
        const __m128i b = _mm_loadu_si128((const __m128i *)(z + 16 * i + 8));
        const __m128i e = _mm_packs_epi16(_mm_cmpeq_epi16(a, zero), _mm_cmpeq_epi16(b, zero));
        m |= (uint64_t)(uint16_t)~_mm_movemask_epi8(e) << (16 * i);
    }
    return m;
#else
    uint64_t m = 0;
    for (int k = 0; k < 64; k++) m |= (uint64_t)(z[k] != 0) << k;
    return m;
#endif
}

/* The scan's geometry and tables, shared by the coding threads */
struct Scan {
    const int16_t *coef;
    jx_frame g;
    size_t rows_per_interval, nintervals;
    uint32_t cl[4][256];                /* jx_jfif_codes' order and packing: code << 8 | length */
};

/* jxe_walk's sinks.  Both take the scan's four tables in one order -- DC luma, AC luma, DC chroma,
 * AC chroma (Cb and Cr together) -- and the interval loop's calls: component() before a block,
 * row() before an MCU row (false: give up), end() after an interval (false: give up). */

/* codes the symbols into w: room for an MCU row reserved ahead; after an interval the padding and,
 * but for the scan's last, RSTm (T.81 F.1.2.1.3, B.2.4.4) */
struct CodeSink {
    const Scan *S;
    BW *w;
    const uint32_t *dct, *act;
    void component(int chroma) { dct = S->cl[2 * chroma], act = S->cl[2 * chroma + 1]; }
    void put(uint32_t c, uint32_t s, uint32_t extra) { bw_bits(w, (c >> 8) << s | extra, (int)((c & 0xffu) + s)); }
    void dc(uint32_t s, uint32_t extra) { put(dct[s], s, extra); }
    void ac(uint32_t sym, uint32_t s, uint32_t extra) { put(act[sym], s, extra); }
    bool row() { return bw_reserve(w, (size_t)S->g.cbw * S->g.bpm * JX_BLOCK_MAX) != 0; }
    bool end(size_t iv)
    {
        if (!bw_reserve(w, 16)) return false;
        bw_flush(w);
        if (iv + 1 < S->nintervals) {
            w->p[w->n++] = 0xff;
            w->p[w->n++] = (uint8_t)(0xd0 + (iv & 7));
        }
        return true;
    }
};

/* counts the symbols: cnt[table][symbol] */
struct CountSink {
    uint64_t (*cnt)[256];
    uint64_t *dct, *act;
    void component(int chroma) { dct = cnt[2 * chroma], act = cnt[2 * chroma + 1]; }
    void dc(uint32_t s, uint32_t) { dct[s]++; }
    void ac(uint32_t sym, uint32_t, uint32_t) { act[sym]++; }
    bool row() { return true; }
    bool end(size_t) { return true; }
};

/* jxe_walk's view of a block in memory */
struct Block {
    const int16_t *z;
    int fetch(uint32_t k) const { return z[k]; }
    int value(int v, uint32_t) const { return v; }
};

/* restart intervals [i0, i1) into the sink, MCU by MCU; the DC predictors reset at each */
template <class Sink>
void walk_intervals(const Scan *S, size_t i0, size_t i1, Sink sink)
{
    const jx_frame &g = S->g;
    for (size_t iv = i0; iv < i1; iv++) {
        int pred[3] = {0, 0, 0};
        const size_t r0 = iv * S->rows_per_interval;
        size_t r1 = r0 + S->rows_per_interval;
        if (r1 > g.cbh) r1 = g.cbh;
        for (size_t my = r0; my < r1; my++) {
            if (!sink.row()) return;
            for (uint32_t mx = 0; mx < g.cbw; mx++)
                for (uint32_t j = 0; j < g.bpm; j++) {
                    const int16_t *z = S->coef + jx_frame_block(&g, (uint32_t)my, mx, j) * 64;
                    const uint32_t comp = j < g.lum ? 0u : j - g.lum + 1u;
                    const int diff = jxe_dc_diff(z[0], pred[comp]);
                    pred[comp] = z[0];
                    sink.component(comp != 0);
                    jxe_walk(sink, Block{z}, nonzero_mask(z) & ~1ull, diff);
                }
        }
        if (!sink.end(iv)) return;
    }
}

struct Job {
    const Scan *S;
    BW w;
    uint64_t (*cnt)[256];                                  /* non-NULL: count, do not code */
};

/* job t of jobs[T]: restart intervals [t NI / T, (t + 1) NI / T) (jx_par.h) */
void job_main(void *jobs, uint32_t t, uint64_t i0, uint64_t i1)
{
    Job *j = (Job *)jobs + t;
    if (j->cnt) walk_intervals(j->S, (size_t)i0, (size_t)i1, CountSink{j->cnt, NULL, NULL});
    else walk_intervals(j->S, (size_t)i0, (size_t)i1, CodeSink{j->S, &j->w, NULL, NULL});
}

/* which frame a writer codes: whole MCUs only, the coded frame of a file of any size, or a
 * one-component file's blocks */
enum Kind { kWhole, kAny, kGray };

/* jpgx_write_jfif_opt, and with kAny jpgx_write_jfif_any: the scan of the coded frame of a
 * width x height file; the header states the file's own size, the restart interval counts the coded
 * frame's MCUs.  With kGray jpgx_write_jfif_gray: the one-component frame (sample_ratio unused), whose MCU
 * is a block; two tables, the luminance ones, are used, counted and written. */
int write_jfif(Kind kind, const int16_t *coef, int width, int height, int quality, int sample_ratio,
               int restart_rows, int nthreads, unsigned jfif_flags, uint8_t *out, size_t cap, size_t *len)
{
    if (jfif_flags & ~JPGX_JFIF_OPTIMIZE) return JPGX_EARG;
    if (!coef || !out || restart_rows < -1 || nthreads < 0) return JPGX_EARG;
    Scan S;
    jx_frame_any fa;
    const bool any = kind == kAny, gray = kind == kGray;
    const int ntab = gray ? 2 : 4;
    int rc = jx_frame_rc_coder(gray  ? jx_frame_make_gray_coded(width, height, &S.g)
                               : any ? jx_frame_make_any(width, height, sample_ratio, &fa)
                                     : jx_frame_make(width, height, sample_ratio, &S.g));
    if (rc) return rc;
    if (any) S.g = fa.c;
    if (quality < 1 || quality > JX_MAXQ) return JPGX_EQUALITY;
    S.coef = coef;
    const size_t mrows = S.g.cbh;
    /* T enters the automatic restart interval below, so a file's bytes depend on it: a stated count is
     * taken as it is, above 64 as well, and only the automatic one goes through jx_thread_count */
    long T = nthreads ? nthreads : (long)jx_thread_count(0);
    /* restart interval: rows of MCUs, Ri = rows x MCUs per row (a 16-bit field) */
    const size_t maxrows = jx_frame_max_rows(&S.g);
    size_t rr = 0;
    if (restart_rows > 0) {
        rr = (size_t)restart_rows;
        if (rr > maxrows) return JPGX_EARG;
    } else if (restart_rows == -1) {                       /* auto: ~4 intervals per thread */
        rr = (mrows + 4 * (size_t)T - 1) / (4 * (size_t)T);
        if (rr > maxrows) rr = maxrows;
        if (rr < 1) rr = 1;
    }
    S.rows_per_interval = rr ? rr : mrows;
    S.nintervals = (mrows + S.rows_per_interval - 1) / S.rows_per_interval;
    if ((size_t)T > S.nintervals) T = (long)S.nintervals;
    const int opt = (jfif_flags & JPGX_JFIF_OPTIMIZE) != 0;

    /* a job per thread, T of them */
    Job *jobs = (Job *)calloc((size_t)T, sizeof(Job));
    uint64_t (*cnt)[256] = opt ? (uint64_t (*)[256])calloc((size_t)T * 4, sizeof *cnt) : NULL;
    rc = (jobs && (cnt || !opt)) ? JPGX_OK : JPGX_ENOMEM;
    for (long t = 0; t < T && !rc; t++) jobs[t].S = &S;

    /* the tables: Annex K.3's, or Annex K.2's from the image's own symbols (each thread counts the
     * intervals it will code; integer sums, so the thread count does not show) */
    uint8_t (*bits)[16] = NULL, (*vals)[256] = NULL;
    uint8_t obits[4][16], ovals[4][256];
    if (opt && !rc) {
        for (long t = 0; t < T; t++) jobs[t].cnt = cnt + 4 * t;
        jx_par_run(S.nintervals, (uint64_t)T, job_main, jobs);
        for (long t = 1; t < T; t++)
            for (int k = 0; k < ntab; k++)
                for (int s = 0; s < 256; s++) cnt[k][s] += cnt[4 * t + k][s];
        memset(ovals, 0, sizeof ovals);
        for (int k = 0; k < ntab; k++) {
            jx_jfif_optimal(cnt[k], obits[k], ovals[k]);
            jx_jfif_build_codes(obits[k], ovals[k], S.cl[k]);
        }
        for (long t = 0; t < T; t++) jobs[t].cnt = NULL;
        bits = obits;
        vals = ovals;
    } else if (!rc) {
        jx_jfif_codes(S.cl);
    }

    /* headers */
    size_t n = 0;
    int overflow = 0;
    if (!rc) {
        const unsigned ri = (unsigned)(rr * S.g.cbw);
        n = gray ? jx_jfif_header_gray(width, height, quality, ri, (const uint8_t (*)[16])bits,
                                       (const uint8_t (*)[256])vals, out, cap, NULL)
                 : jx_jfif_header_tabs(width, height, quality, sample_ratio, ri, (const uint8_t (*)[16])bits,
                                       (const uint8_t (*)[256])vals, out, cap, NULL);
        if (!n) rc = JPGX_EQUALITY;
        if (n > cap) overflow = 1;
    }

    /* the scan: every thread codes into its own buffer */
    if (!rc) jx_par_run(S.nintervals, (uint64_t)T, job_main, jobs);
    for (long t = 0; t < T && !rc; t++)
        if (jobs[t].w.oom) rc = JPGX_ENOMEM;
    if (!rc) {
        for (long t = 0; t < T; t++) {
            if (n + jobs[t].w.n <= cap) memcpy(out + n, jobs[t].w.p, jobs[t].w.n);
            else overflow = 1;
            n += jobs[t].w.n;
        }
        for (int b = 0; b < 2; b++, n++) {                 /* EOI */
            if (n < cap) out[n] = b ? 0xd9 : 0xff;
            else overflow = 1;
        }
        if (len) *len = n;
        if (overflow) rc = JPGX_EARG;
    }
    if (jobs)
        for (long t = 0; t < T; t++) free(jobs[t].w.p);
    free(jobs);
    free(cnt);
    return rc;
}

}  // namespace

extern "C" {

size_t jpgx_jfif_bound(int width, int height)
{
    if (width <= 0 || height <= 0) return 0;
    /* headers + a per-block maximum with margin -- DC code + magnitude <= 16 + 16 bits, 63 AC
     * codes + magnitudes <= 63 x (16 + 16) bits, EOB <= 16 bits -- doubled for 0xFF stuffing,
     * plus per restart interval (at most one per MCU row) the padding byte, its possible stuffing
     * byte and RSTm: 4 bytes */
    const size_t blocks = (size_t)(width / 8 + 1) * (height / 8 + 1) * 3;
    return 1024 + blocks * 2 * (32 + 63 * 32 + 16) / 8 + 4 * (size_t)(height / 8 + 1);
}

int jpgx_write_jfif(const int16_t *coef, int width, int height, int quality, uint8_t *out,
                    size_t cap, size_t *len)
{
    return jpgx_write_jfif_ex(coef, width, height, quality, 0, 0, 1, out, cap, len);
}

int jpgx_write_jfif_sub(const int16_t *coef, int width, int height, int quality,
                        int sample_ratio, uint8_t *out, size_t cap, size_t *len)
{
    return jpgx_write_jfif_ex(coef, width, height, quality, sample_ratio, 0, 1, out, cap, len);
}

int jpgx_write_jfif_ex(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                       int restart_rows, int nthreads, uint8_t *out, size_t cap, size_t *len)
{
    return jpgx_write_jfif_opt(coef, width, height, quality, sample_ratio, restart_rows, nthreads, 0u, out,
                               cap, len);
}

int jpgx_write_jfif_opt(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                        int restart_rows, int nthreads, unsigned jfif_flags, uint8_t *out, size_t cap,
                        size_t *len)
{
    return write_jfif(kWhole, coef, width, height, quality, sample_ratio, restart_rows, nthreads, jfif_flags, out,
                      cap, len);
}

int jpgx_write_jfif_any(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                        int restart_rows, int nthreads, unsigned jfif_flags, uint8_t *out, size_t cap,
                        size_t *len)
{
    return write_jfif(kAny, coef, width, height, quality, sample_ratio, restart_rows, nthreads, jfif_flags, out,
                      cap, len);
}

int jpgx_write_jfif_gray(const int16_t *coef, int width, int height, int quality, int restart_rows,
                         int nthreads, unsigned jfif_flags, uint8_t *out, size_t cap, size_t *len)
{
    return write_jfif(kGray, coef, width, height, quality, 0, restart_rows, nthreads, jfif_flags, out, cap, len);
}

}  /* extern "C" */
