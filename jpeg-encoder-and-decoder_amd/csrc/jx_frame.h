/*
 * jx_frame.h -- a coded frame, stated once: what width, height and sample ratio make
 * of the sampling factors, the block and MCU counts and the place of an MCU's blocks in the
 * coefficient array Y [nb][64] | Cb [nbc][64] | Cr [nbc][64].  One source for the JFIF coder (host and
 * device), the pixel path and the device decoder's entry point; the decoder's routines keep their own
 * copy in jxd_frame (jx_jfif_dec.h; DESIGN.md 4.7 says why).  Plain C99 that is also C++ and HIP.
 */
#ifndef JX_FRAME_H
#define JX_FRAME_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/jpgx.h"

#if defined(__HIPCC__)
#define JXF_FN __host__ __device__ static inline
#else
#define JXF_FN static inline
#endif

/* Y sampled hs x vs, Cb and Cr 1 x 1, one interleaved scan */
typedef struct jx_frame {
    uint32_t hs, vs;        /* Y blocks per MCU, across and down: 1x1, 2x1, 2x2                  */
    uint32_t lum, bpm;      /* Y blocks per MCU (hs x vs); blocks per MCU (lum + 2)              */
    uint32_t bw, bh;        /* Y blocks per block row, block rows                                */
    uint32_t cbw, cbh;      /* the same of a chroma plane: MCUs per MCU row, MCU rows            */
    uint32_t nb, nbc, nblk; /* blocks: Y, per chroma plane (= MCUs), per frame                   */
} jx_frame;

/* why a frame is refused; the first that applies */
enum {
    JXF_SAMPLE = 1,         /* sample_ratio is not 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)             */
    JXF_RANGE,              /* a side <= 0 or > 65535 (SOF's 16-bit fields)                      */
    JXF_MULT8,              /* a side is not a multiple of 8                                     */
    JXF_MCU                 /* a side is not a multiple of the MCU (8 hs x 8 vs)                 */
};

/* the luma sampling factors of sample_ratio 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) */
JXF_FN void jx_frame_sampling(int sample_ratio, uint32_t *hs, uint32_t *vs)
{
    *hs = sample_ratio ? 2u : 1u;
    *vs = sample_ratio == 2 ? 2u : 1u;
}

JXF_FN int jx_frame_make(int width, int height, int sample_ratio, jx_frame *f)
{
    if (sample_ratio < 0 || sample_ratio > 2) return JXF_SAMPLE;
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return JXF_RANGE;
    if (width % 8 || height % 8) return JXF_MULT8;
    jx_frame_sampling(sample_ratio, &f->hs, &f->vs);
    f->bw = (uint32_t)width / 8u;
    f->bh = (uint32_t)height / 8u;
    if (f->bw % f->hs || f->bh % f->vs) return JXF_MCU;
    f->lum = f->hs * f->vs;
    f->bpm = f->lum + 2u;
    f->cbw = f->bw / f->hs;
    f->cbh = f->bh / f->vs;
    f->nb = f->bw * f->bh;
    f->nbc = f->cbw * f->cbh;
    f->nblk = f->nb + 2u * f->nbc;
    return 0;
}

/* A file of any width and height (the decode side's _any entry points): the coded
 * frame is the file's size rounded up to the MCU, and everything above holds for it; the visible
 * frame is the SOF's w x h, of which a chroma plane really has wc = ceil(w / hs) samples per row and
 * hc = ceil(h / vs) rows -- the extent the upsampling clamps at. */
typedef struct jx_frame_any {
    jx_frame c;             /* the coded frame                                                   */
    uint32_t w, h;          /* the visible frame, 1 .. 65535 each                                */
    uint32_t wc, hc;        /* a chroma plane's real extent                                      */
} jx_frame_any;

/* the coded size of width x height: both rounded up to the MCU */
JXF_FN void jx_frame_coded(uint32_t width, uint32_t height, uint32_t hs, uint32_t vs, uint32_t *cw, uint32_t *ch)
{
    *cw = (width + 8u * hs - 1u) / (8u * hs) * (8u * hs);
    *ch = (height + 8u * vs - 1u) / (8u * vs) * (8u * vs);
}

/* jx_frame_make without the multiple-of-the-MCU tests: JXF_SAMPLE or JXF_RANGE are all it refuses.
 * For a size that is a multiple of the MCU, a->c is what jx_frame_make fills. */
JXF_FN int jx_frame_make_any(int width, int height, int sample_ratio, jx_frame_any *a)
{
    if (sample_ratio < 0 || sample_ratio > 2) return JXF_SAMPLE;
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return JXF_RANGE;
    jx_frame *f = &a->c;
    uint32_t cw, ch;
    jx_frame_sampling(sample_ratio, &f->hs, &f->vs);
    jx_frame_coded((uint32_t)width, (uint32_t)height, f->hs, f->vs, &cw, &ch);
    f->bw = cw / 8u;
    f->bh = ch / 8u;
    f->lum = f->hs * f->vs;
    f->bpm = f->lum + 2u;
    f->cbw = f->bw / f->hs;
    f->cbh = f->bh / f->vs;
    f->nb = f->bw * f->bh;
    f->nbc = f->cbw * f->cbh;
    f->nblk = f->nb + 2u * f->nbc;
    a->w = (uint32_t)width;
    a->h = (uint32_t)height;
    a->wc = (a->w + f->hs - 1u) / f->hs;
    a->hc = (a->h + f->vs - 1u) / f->vs;
    return 0;
}

/* A decode at 1 / d of the size, d = 2, 4 or 8 (the _scaled entry points): the output is
 * ow x oh = ceil(w / d) x ceil(h / d); a luma block becomes m x m = 8 / d samples and a chroma block n x n.
 * The rule for n is libjpeg's (one DCT_scaled_size per component): it starts at m and doubles while it is
 * below 8 and divides the MCU's scaled extent both ways.  4:4:4 and 4:2:2: n = m; 4:2:0: n = 2 m, the
 * chroma plane then has the luma's size.  jx_scaled_ok: d is one of the three. */
JXF_FN int jx_scaled_ok(int scale_denom) { return scale_denom == 2 || scale_denom == 4 || scale_denom == 8; }

JXF_FN uint32_t jx_scaled_chroma_n(uint32_t m, uint32_t hs, uint32_t vs)
{
    uint32_t n = m;
    while (n < 8u && (hs * m) % (2u * n) == 0u && (vs * m) % (2u * n) == 0u) n *= 2u;
    return n;
}

typedef struct jx_frame_scaled {
    uint32_t d, m, n;       /* the denominator; samples per luma block and per chroma block, each way */
    uint32_t ow, oh;        /* the output                                                        */
    uint32_t wc, hc;        /* a chroma plane's real extent at n: ceil(w n / (8 hs)), ceil(h n / (8 vs)) */
    uint32_t hfac;          /* luma samples per chroma sample across: hs m / n, 1 or 2 (down: always 1) */
} jx_frame_scaled;

/* of a visible frame w x h with sampling hs x vs (1 x 1 for a one-component frame) */
JXF_FN void jx_frame_make_scaled(uint32_t w, uint32_t h, uint32_t hs, uint32_t vs, uint32_t d, jx_frame_scaled *s)
{
    s->d = d;
    s->m = 8u / d;
    s->n = jx_scaled_chroma_n(s->m, hs, vs);
    s->ow = (w + d - 1u) / d;
    s->oh = (h + d - 1u) / d;
    s->wc = (w * s->n + 8u * hs - 1u) / (8u * hs);
    s->hc = (h * s->n + 8u * vs - 1u) / (8u * vs);
    s->hfac = hs * s->m / s->n;
}

/* A one-component (grayscale) file (the decode side's _gray entry points): its scan is
 * not interleaved, so whatever sampling factors SOF states, the MCU is one block and the frame codes
 * bw x bh = ceil(w / 8) x ceil(h / 8) blocks in raster order: coefficients Y [nb][64], no chroma. */
typedef struct jx_frame_gray {
    uint32_t w, h;          /* the visible frame, 1 .. 65535 each                                */
    uint32_t bw, bh, nb;    /* blocks per block row, block rows, blocks (= MCUs)                 */
} jx_frame_gray;

/* JXF_RANGE is all it refuses */
JXF_FN int jx_frame_make_gray(int width, int height, jx_frame_gray *g)
{
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return JXF_RANGE;
    g->w = (uint32_t)width;
    g->h = (uint32_t)height;
    g->bw = (g->w + 7u) / 8u;
    g->bh = (g->h + 7u) / 8u;
    g->nb = g->bw * g->bh;
    return 0;
}

/* The same frame as the JFIF coder walks it (the encode side's _gray entry points): one block per MCU,
 * hs = vs = lum = bpm = 1, an MCU row is a block row (cbw = bw, cbh = bh), no chroma (nbc = 0, nblk = nb);
 * jx_frame_block(f, my, mx, 0) is block my * bw + mx.  JXF_RANGE is all it refuses. */
JXF_FN int jx_frame_make_gray_coded(int width, int height, jx_frame *f)
{
    jx_frame_gray g;
    if (jx_frame_make_gray(width, height, &g)) return JXF_RANGE;
    f->hs = f->vs = f->lum = f->bpm = 1u;
    f->bw = f->cbw = g.bw;
    f->bh = f->cbh = g.bh;
    f->nb = f->nblk = g.nb;
    f->nbc = 0u;
    return 0;
}

/* The codes the entry points refuse with are part of the ABI and differ; each is one mapping of
 * the reason:            SAMPLE         RANGE           MULT8           MCU
 *   the JFIF coder       EARG           EARG            EARG            EGEOMETRY
 *   the device decoder   EARG           EARG            EGEOMETRY       EGEOMETRY
 *   the pixel path       ESAMPLE        EGEOMETRY       EGEOMETRY       EGEOMETRY           */
JXF_FN int jx_frame_rc_coder(int why) { return !why ? JPGX_OK : why == JXF_MCU ? JPGX_EGEOMETRY : JPGX_EARG; }
JXF_FN int jx_frame_rc_decoder(int why) { return !why ? JPGX_OK : why >= JXF_MULT8 ? JPGX_EGEOMETRY : JPGX_EARG; }
JXF_FN int jx_frame_rc_pixels(int why) { return !why ? JPGX_OK : why == JXF_SAMPLE ? JPGX_ESAMPLE : JPGX_EGEOMETRY; }

/* the most MCU rows a restart interval may have: Ri = rows x MCUs per row is DRI's 16-bit field */
JXF_FN uint32_t jx_frame_max_rows(const jx_frame *f) { return 65535u / f->cbw; }

/* block indices in the frame's coefficient array: luma block (dy, dx) of MCU (my, mx), and the
 * MCU's block of chroma plane c (0: Cb, 1: Cr) */
JXF_FN size_t jx_frame_luma(const jx_frame *f, uint32_t my, uint32_t mx, uint32_t dy, uint32_t dx)
{
    return (size_t)(my * f->vs + dy) * f->bw + mx * f->hs + dx;
}

JXF_FN size_t jx_frame_chroma(const jx_frame *f, uint32_t c, uint32_t my, uint32_t mx)
{
    return (size_t)f->nb + (size_t)c * f->nbc + (size_t)my * f->cbw + mx;
}

/* position j of MCU (my, mx) in scan order: the hs x vs luma blocks in raster order within the
 * MCU, then Cb, then Cr (T.81 A.2.3) */
JXF_FN size_t jx_frame_block(const jx_frame *f, uint32_t my, uint32_t mx, uint32_t j)
{
    if (j < f->lum) {
        const uint32_t dy = j / f->hs;
        return jx_frame_luma(f, my, mx, dy, j - dy * f->hs);
    }
    return jx_frame_chroma(f, j - f->lum, my, mx);
}

#endif
