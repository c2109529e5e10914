/*
 * jpgx_pixels_host.cpp -- the host twin of the pixel kernels: jpgx_pixels_host and
 * jpgx_pixels_host_any, a frame of any width and height (include/jpgx_compat.h).  The arithmetic is jx_idct.h's, the source the kernels
 * (jpgx_pixels.hip) compile; this file adds the planes and the threads.  No HIP: built with g++,
 * as jpgx_jfif_read.cpp.
 *
 * Two phases, each over MCU rows on the threads: every block of Y, Cb and Cr to its 0..255
 * samples in three planes; then, pixel row by pixel row, the chroma upsampled (4:2:2 / 4:2:0)
 * and the colour converted.  A thread writes only its own rows, so the result does not depend on
 * the thread count.
 *
 * jpgx_pixels_host_gray (a one-component frame): one phase over block rows; a block's samples go
 * straight to the output, once per channel.
 *
 * jpgx_pixels_host_scaled, jpgx_pixels_host_gray_scaled (1/2, 1/4, 1/8 of the size): the
 * same phases with the reduced-size transforms, a luma block m x m samples and a chroma block n x n.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/jpgx_compat.h"
#include "jx_frame.h"
#include "jx_idct.h"
#include "jx_par.h"

namespace {

const uint8_t kZZ[64] = JXI_ZZ_INIT;

struct Ctx {
    const int16_t *coef;
    const uint16_t (*qt)[64];
    jx_frame g;                     /* the coded frame */
    uint32_t w, h, wc, hc;          /* the visible frame and a chroma plane's real extent (jx_frame_any) */
    uint8_t *plane[3];              /* Y: 8 bh x 8 bw, Cb / Cr: 8 cbh x 8 cbw */
    uint8_t *rgb;
    size_t pitch;
};

/* one block: dequantise, columns, rows, range limit */
void block_samples(const int16_t *coef, const uint16_t *qt, uint8_t *dst, size_t dpitch)
{
    uint32_t d[64], v[8];
    for (int k = 0; k < 64; k++) d[kZZ[k]] = jxi_dequant(coef[k], qt[k]);
    for (int c = 0; c < 8; c++) {
        for (int r = 0; r < 8; r++) v[r] = d[r * 8 + c];
        jxi_idct8<0>(v, JXI_PASS1_SHIFT);
        for (int r = 0; r < 8; r++) d[r * 8 + c] = v[r];
    }
    for (int r = 0; r < 8; r++) {
        jxi_idct8<0>(d + r * 8, JXI_PASS2_SHIFT);
        for (int c = 0; c < 8; c++) dst[r * dpitch + c] = (uint8_t)jxi_range(d[r * 8 + c]);
    }
}

void samples_rows(const Ctx &c, uint32_t m0, uint32_t m1)
{
    const jx_frame &g = c.g;
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t bw = ch ? g.cbw : g.bw, per = ch ? 1u : g.vs;
        const int16_t *src = c.coef + (ch == 0 ? 0 : ((size_t)g.nb + (size_t)(ch - 1) * g.nbc) * 64);
        const size_t pp = (size_t)bw * 8;
        for (uint32_t by = m0 * per; by < m1 * per; by++)
            for (uint32_t bx = 0; bx < bw; bx++)
                block_samples(src + ((size_t)by * bw + bx) * 64, c.qt[ch ? 1 : 0],
                              c.plane[ch] + (size_t)by * 8 * pp + (size_t)bx * 8, pp);
    }
}

void pixel_rows(const Ctx &c, uint32_t m0, uint32_t m1)
{
    const jx_frame &g = c.g;
    /* the planes are the coded frame's; the clamps are at the chroma's real extent, and with two
     * samples or fewer per row the chroma is replicated, not filtered */
    const uint32_t P = g.bw * 8, Pc = g.cbw * 8, W = c.w, Wc = c.wc, Hc = c.hc;
    const int v2 = g.vs == 2, rep = Wc <= 2;
    for (uint32_t y = m0 * 8 * g.vs; y < m1 * 8 * g.vs && y < c.h; y++) {
        const uint8_t *yrow = c.plane[0] + (size_t)y * P;
        uint8_t *out = c.rgb + (size_t)y * c.pitch;
        const uint32_t cy = y / g.vs;
        const uint32_t far = !v2 ? cy : (y & 1u) ? (cy + 1 < Hc ? cy + 1 : cy) : (cy ? cy - 1 : 0);
        const uint8_t *n1 = c.plane[1] + (size_t)cy * Pc, *f1 = c.plane[1] + (size_t)far * Pc;
        const uint8_t *n2 = c.plane[2] + (size_t)cy * Pc, *f2 = c.plane[2] + (size_t)far * Pc;
        for (uint32_t x = 0; x < W; x++) {
            uint32_t cb, cr, r, gg, b;
            if (g.hs == 1) {
                cb = n1[x];
                cr = n2[x];
            } else if (rep) {
                cb = n1[x >> 1];
                cr = n2[x >> 1];
            } else {
                const uint32_t i = x >> 1;
                const uint32_t j = (x & 1u) ? (i + 1 < Wc ? i + 1 : i) : (i ? i - 1 : 0);   /* clamped to the plane */
                if (v2) {
                    const uint32_t sc1 = jxi_vsum(n1[i], f1[i]), sn1 = jxi_vsum(n1[j], f1[j]);
                    const uint32_t sc2 = jxi_vsum(n2[i], f2[i]), sn2 = jxi_vsum(n2[j], f2[j]);
                    cb = (x & 1u) ? jxi_up_odd(sc1, sn1, 1) : jxi_up_even(sc1, sn1, 1);
                    cr = (x & 1u) ? jxi_up_odd(sc2, sn2, 1) : jxi_up_even(sc2, sn2, 1);
                } else {
                    cb = (x & 1u) ? jxi_up_odd(n1[i], n1[j], 0) : jxi_up_even(n1[i], n1[j], 0);
                    cr = (x & 1u) ? jxi_up_odd(n2[i], n2[j], 0) : jxi_up_even(n2[i], n2[j], 0);
                }
            }
            jxi_rgb(yrow[x], cb, cr, &r, &gg, &b);
            out[3 * x] = (uint8_t)r;
            out[3 * x + 1] = (uint8_t)gg;
            out[3 * x + 2] = (uint8_t)b;
        }
    }
}

/* the two phases over a thread's MCU rows (jx_par.h) */
void run_samples(void *c, uint32_t, uint64_t m0, uint64_t m1) { samples_rows(*(const Ctx *)c, (uint32_t)m0, (uint32_t)m1); }

void run_pixels(void *c, uint32_t, uint64_t m0, uint64_t m1) { pixel_rows(*(const Ctx *)c, (uint32_t)m0, (uint32_t)m1); }

int pixels_host(bool any, const int16_t *coef, int width, int height, int sample_ratio, const uint16_t qt[2][64],
                uint8_t *rgb, size_t pitch, int nthreads)
{
    if (!coef || !qt || !rgb || nthreads < 0) return JPGX_EARG;
    Ctx c;
    memset(&c, 0, sizeof c);
    jx_frame_any a;
    const int rc = jx_frame_rc_pixels(any ? jx_frame_make_any(width, height, sample_ratio, &a)
                                          : jx_frame_make(width, height, sample_ratio, &c.g));
    if (rc) return rc;
    if (any) c.g = a.c;
    c.w = (uint32_t)width;
    c.h = (uint32_t)height;
    c.wc = any ? a.wc : c.g.cbw * 8;
    c.hc = any ? a.hc : c.g.cbh * 8;
    if (pitch < (size_t)width * 3) return JPGX_EARG;
    const size_t ny = (size_t)c.g.nb * 64, nc = (size_t)c.g.nbc * 64;
    uint8_t *planes = (uint8_t *)malloc(ny + 2 * nc);
    if (!planes) return JPGX_ENOMEM;
    c.coef = coef;
    c.qt = qt;
    c.plane[0] = planes;
    c.plane[1] = planes + ny;
    c.plane[2] = planes + ny + nc;
    c.rgb = rgb;
    c.pitch = pitch;
    const uint32_t nt = jx_thread_count(nthreads);
    /* over MCU rows, a chroma block row each; joined: every plane is whole before a pixel row reads its neighbours */
    jx_par_run(c.g.cbh, nt, run_samples, &c);
    jx_par_run(c.g.cbh, nt, run_pixels, &c);
    free(planes);
    return JPGX_OK;
}

/* ---- the one-component frame: Y [nb][64] and one table to 1 or 3 equal channels ---------------- */
struct GrayCtx {
    const int16_t *coef;
    const uint16_t *qt;
    jx_frame_gray g;
    uint8_t *out;
    size_t pitch;
    uint32_t channels;
};

/* a thread's block rows (jx_par.h) */
void run_gray(void *ctx, uint32_t, uint64_t r0, uint64_t r1)
{
    const GrayCtx &c = *(const GrayCtx *)ctx;
    const uint32_t ch = c.channels;
    for (uint32_t by = (uint32_t)r0; by < (uint32_t)r1; by++)
        for (uint32_t bx = 0; bx < c.g.bw; bx++) {
            uint8_t s[64];
            block_samples(c.coef + ((size_t)by * c.g.bw + bx) * 64, c.qt, s, 8);
            for (uint32_t r = 0; r < 8 && by * 8 + r < c.g.h; r++) {
                uint8_t *row = c.out + (size_t)(by * 8 + r) * c.pitch;
                for (uint32_t x = bx * 8; x < bx * 8 + 8 && x < c.g.w; x++)
                    for (uint32_t k = 0; k < ch; k++) row[(size_t)ch * x + k] = s[r * 8 + (x & 7u)];
            }
        }
}

int pixels_host_gray(const int16_t *coef, int width, int height, const uint16_t *qt, uint8_t *out, size_t pitch,
                     int channels, int nthreads)
{
    if (!coef || !qt || !out || nthreads < 0 || (channels != 1 && channels != 3)) return JPGX_EARG;
    GrayCtx c;
    memset(&c, 0, sizeof c);
    const int rc = jx_frame_rc_pixels(jx_frame_make_gray(width, height, &c.g));
    if (rc) return rc;
    if (pitch < (size_t)width * (size_t)channels) return JPGX_EARG;
    c.coef = coef;
    c.qt = qt;
    c.out = out;
    c.pitch = pitch;
    c.channels = (uint32_t)channels;
    jx_par_run(c.g.bh, jx_thread_count(nthreads), run_gray, &c);
    return JPGX_OK;
}

/* ---- 1 / d of the size ------------------------------------------------------ */
/* one block to n x n samples, n = 4, 2 or 1 */
void block_samples_n(const int16_t *coef, const uint16_t *qt, uint32_t n, uint8_t *dst, size_t dpitch)
{
    if (n == 1) {
        dst[0] = (uint8_t)jxi_range(jxi_idct1(jxi_dequant(coef[0], qt[0])));
        return;
    }
    uint32_t d[64], v[8];
    for (int k = 0; k < 64; k++) d[kZZ[k]] = jxi_dequant(coef[k], qt[k]);
    for (int c = 0; c < 8; c++) {
        for (int r = 0; r < 8; r++) v[r] = d[r * 8 + c];
        if (n == 4) jxi_idctn<4, 0>(v, 1);
        else jxi_idctn<2, 0>(v, 1);
        for (uint32_t r = 0; r < n; r++) d[r * 8 + c] = v[r];
    }
    for (uint32_t r = 0; r < n; r++) {
        if (n == 4) jxi_idctn<4, 0>(d + r * 8, 2);
        else jxi_idctn<2, 0>(d + r * 8, 2);
        for (uint32_t c = 0; c < n; c++) dst[r * dpitch + c] = (uint8_t)jxi_range(d[r * 8 + c]);
    }
}

struct ScaledCtx {
    const int16_t *coef;
    const uint16_t (*qt)[64];
    jx_frame g;                     /* the coded frame */
    jx_frame_scaled s;
    uint8_t *plane[3];              /* Y: m bh x m bw, Cb / Cr: n cbh x n cbw */
    uint8_t *rgb;
    size_t pitch;
};

/* a thread's MCU rows: every block to its samples */
void run_samples_scaled(void *ctx, uint32_t, uint64_t m0, uint64_t m1)
{
    const ScaledCtx &c = *(const ScaledCtx *)ctx;
    const jx_frame &g = c.g;
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t bw = ch ? g.cbw : g.bw, per = ch ? 1u : g.vs, n = ch ? c.s.n : c.s.m;
        const int16_t *src = c.coef + (ch == 0 ? 0 : ((size_t)g.nb + (size_t)(ch - 1) * g.nbc) * 64);
        const size_t pp = (size_t)bw * n;
        for (uint32_t by = (uint32_t)m0 * per; by < (uint32_t)m1 * per; by++)
            for (uint32_t bx = 0; bx < bw; bx++) {
                const int16_t *blk = src + ((size_t)by * bw + bx) * 64;
                uint8_t *dst = c.plane[ch] + (size_t)by * n * pp + (size_t)bx * n;
                if (n == 8) block_samples(blk, c.qt[ch ? 1 : 0], dst, pp);
                else block_samples_n(blk, c.qt[ch ? 1 : 0], n, dst, pp);
            }
    }
}

/* a thread's MCU rows of pixels: the chroma plane has the luma's size (hfac 1), or half its width: then
 * the h2v1 triangle filter clamped at the chroma's real extent, or, with two samples or fewer per row
 * or at 1/8 of the size, replication */
void run_pixels_scaled(void *ctx, uint32_t, uint64_t m0, uint64_t m1)
{
    const ScaledCtx &c = *(const ScaledCtx *)ctx;
    const jx_frame &g = c.g;
    const uint32_t P = g.bw * c.s.m, Pc = g.cbw * c.s.n, Wc = c.s.wc, rows = c.s.m * g.vs;
    const bool rep = Wc <= 2 || c.s.m == 1;
    for (uint32_t y = (uint32_t)m0 * rows; y < (uint32_t)m1 * rows && y < c.s.oh; y++) {
        const uint8_t *yrow = c.plane[0] + (size_t)y * P;
        const uint8_t *n1 = c.plane[1] + (size_t)y * Pc, *n2 = c.plane[2] + (size_t)y * Pc;
        uint8_t *out = c.rgb + (size_t)y * c.pitch;
        for (uint32_t x = 0; x < c.s.ow; x++) {
            uint32_t cb, cr, r, gg, b;
            if (c.s.hfac == 1) {
                cb = n1[x];
                cr = n2[x];
            } else if (rep) {
                cb = n1[x >> 1];
                cr = n2[x >> 1];
            } else {
                const uint32_t i = x >> 1;
                const uint32_t j = (x & 1u) ? (i + 1 < Wc ? i + 1 : i) : (i ? i - 1 : 0);
                cb = (x & 1u) ? jxi_up_odd(n1[i], n1[j], 0) : jxi_up_even(n1[i], n1[j], 0);
                cr = (x & 1u) ? jxi_up_odd(n2[i], n2[j], 0) : jxi_up_even(n2[i], n2[j], 0);
            }
            jxi_rgb(yrow[x], cb, cr, &r, &gg, &b);
            out[3 * x] = (uint8_t)r;
            out[3 * x + 1] = (uint8_t)gg;
            out[3 * x + 2] = (uint8_t)b;
        }
    }
}

int pixels_host_scaled(const int16_t *coef, int width, int height, int sample_ratio, int scale_denom,
                       const uint16_t qt[2][64], uint8_t *rgb, size_t pitch, int nthreads)
{
    if (scale_denom == 1) return pixels_host(true, coef, width, height, sample_ratio, qt, rgb, pitch, nthreads);
    if (!coef || !qt || !rgb || nthreads < 0 || !jx_scaled_ok(scale_denom)) return JPGX_EARG;
    ScaledCtx c;
    memset(&c, 0, sizeof c);
    jx_frame_any a;
    const int rc = jx_frame_rc_pixels(jx_frame_make_any(width, height, sample_ratio, &a));
    if (rc) return rc;
    c.g = a.c;
    jx_frame_make_scaled(a.w, a.h, c.g.hs, c.g.vs, (uint32_t)scale_denom, &c.s);
    if (pitch < (size_t)c.s.ow * 3) return JPGX_EARG;
    const size_t ny = (size_t)c.g.nb * c.s.m * c.s.m, nc = (size_t)c.g.nbc * c.s.n * c.s.n;
    uint8_t *planes = (uint8_t *)malloc(ny + 2 * nc);
    if (!planes) return JPGX_ENOMEM;
    c.coef = coef;
    c.qt = qt;
    c.plane[0] = planes;
    c.plane[1] = planes + ny;
    c.plane[2] = planes + ny + nc;
    c.rgb = rgb;
    c.pitch = pitch;
    const uint32_t nt = jx_thread_count(nthreads);
    jx_par_run(c.g.cbh, nt, run_samples_scaled, &c);
    jx_par_run(c.g.cbh, nt, run_pixels_scaled, &c);
    free(planes);
    return JPGX_OK;
}

struct GrayScaledCtx {
    GrayCtx c;
    jx_frame_scaled s;
};

/* a thread's block rows */
void run_gray_scaled(void *ctx, uint32_t, uint64_t r0, uint64_t r1)
{
    const GrayScaledCtx &x = *(const GrayScaledCtx *)ctx;
    const GrayCtx &c = x.c;
    const uint32_t ch = c.channels, m = x.s.m;
    for (uint32_t by = (uint32_t)r0; by < (uint32_t)r1; by++)
        for (uint32_t bx = 0; bx < c.g.bw; bx++) {
            uint8_t s[16];
            block_samples_n(c.coef + ((size_t)by * c.g.bw + bx) * 64, c.qt, m, s, m);
            for (uint32_t r = 0; r < m && by * m + r < x.s.oh; r++) {
                uint8_t *row = c.out + (size_t)(by * m + r) * c.pitch;
                for (uint32_t i = 0; i < m && bx * m + i < x.s.ow; i++)
                    for (uint32_t k = 0; k < ch; k++) row[(size_t)ch * (bx * m + i) + k] = s[r * m + i];
            }
        }
}

int pixels_host_gray_scaled(const int16_t *coef, int width, int height, int scale_denom, const uint16_t *qt,
                            uint8_t *out, size_t pitch, int channels, int nthreads)
{
    if (scale_denom == 1) return pixels_host_gray(coef, width, height, qt, out, pitch, channels, nthreads);
    if (!coef || !qt || !out || nthreads < 0 || (channels != 1 && channels != 3) || !jx_scaled_ok(scale_denom))
        return JPGX_EARG;
    GrayScaledCtx x;
    memset(&x, 0, sizeof x);
    const int rc = jx_frame_rc_pixels(jx_frame_make_gray(width, height, &x.c.g));
    if (rc) return rc;
    jx_frame_make_scaled(x.c.g.w, x.c.g.h, 1u, 1u, (uint32_t)scale_denom, &x.s);
    if (pitch < (size_t)x.s.ow * (size_t)channels) return JPGX_EARG;
    x.c.coef = coef;
    x.c.qt = qt;
    x.c.out = out;
    x.c.pitch = pitch;
    x.c.channels = (uint32_t)channels;
    jx_par_run(x.c.g.bh, jx_thread_count(nthreads), run_gray_scaled, &x);
    return JPGX_OK;
}

}  // namespace

extern "C" {

int jpgx_pixels_host_scaled(const int16_t *coef, int width, int height, int sample_ratio, int scale_denom,
                            const uint16_t qt[2][64], uint8_t *rgb, size_t pitch, int nthreads)
{
    return pixels_host_scaled(coef, width, height, sample_ratio, scale_denom, qt, rgb, pitch, nthreads);
}

int jpgx_pixels_host_gray_scaled(const int16_t *coef, int width, int height, int scale_denom, const uint16_t qt[64],
                                 uint8_t *out, size_t pitch, int channels, int nthreads)
{
    return pixels_host_gray_scaled(coef, width, height, scale_denom, qt, out, pitch, channels, nthreads);
}

int jpgx_pixels_host(const int16_t *coef, int width, int height, int sample_ratio, const uint16_t qt[2][64], uint8_t *rgb,
                     size_t pitch, int nthreads)
{
    return pixels_host(false, coef, width, height, sample_ratio, qt, rgb, pitch, nthreads);
}

int jpgx_pixels_host_any(const int16_t *coef, int width, int height, int sample_ratio, const uint16_t qt[2][64],
                         uint8_t *rgb, size_t pitch, int nthreads)
{
    return pixels_host(true, coef, width, height, sample_ratio, qt, rgb, pitch, nthreads);
}

int jpgx_pixels_host_gray(const int16_t *coef, int width, int height, const uint16_t qt[64], uint8_t *out, size_t pitch,
                          int channels, int nthreads)
{
    return pixels_host_gray(coef, width, height, qt, out, pitch, channels, nthreads);
}

}  /* extern "C" */
