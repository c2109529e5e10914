/*
 * pixels_scaled_san.c -- jpgx_pixels_host_scaled and jpgx_pixels_host_gray_scaled
 * (csrc/jpgx_pixels_host.cpp, csrc/jx_idct.h, csrc/jx_frame.h) under AddressSanitizer and
 * UndefinedBehaviorSanitizer: tests/test_pixels_scaled.py builds this program with the host pixel
 * source under -fsanitize=address,undefined -fno-sanitize-recover=undefined and runs it.  The
 * arithmetic is specified to wrap, so every input must run without a report: every coefficient at
 * +-32767 and -32768 under tables of 65535, and 300 random full-range frames under random tables per
 * sampling, at sizes that end inside a block, inside an MCU and on one, for scale_denom 1, 2, 4, 8.
 * The coefficient and output buffers are exactly their sizes, so a write beyond bytes
 * [0, bytes per pixel * ow) of rows [0, oh) is a report.  Ends with "pixels_scaled_san: clean".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

static uint64_t splitmix(uint64_t *s)
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long frames = 0;

/* blocks of the coded frame; sr 3: a one-component frame */
static size_t nblocks(int w, int h, int sr)
{
    const int mw = sr == 1 || sr == 2 ? 16 : 8, mh = sr == 2 ? 16 : 8;
    const size_t nb = (size_t)((w + mw - 1) / mw * (mw / 8)) * (size_t)((h + mh - 1) / mh * (mh / 8));
    return sr == 3 ? nb : nb + 2 * (sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4);
}

/* one frame through the routine at every scale: fresh buffers of exactly the sizes, 1 and 3 threads agree */
static void run(const int16_t *src, int w, int h, int sr, const uint16_t qt[2][64])
{
    static const int scales[4] = {1, 2, 4, 8};
    const size_t n = nblocks(w, h, sr) * 64;
    int16_t *coef = malloc(n * sizeof *coef);
    if (!coef) exit(2);
    memcpy(coef, src, n * sizeof *coef);
    for (int k = 0; k < 4; k++)
        for (int channels = sr == 3 ? 1 : 3; channels <= 3; channels += 2) {
            const int d = scales[k], ow = (w + d - 1) / d, oh = (h + d - 1) / d;
            const size_t pitch = (size_t)ow * (size_t)channels, bytes = pitch * (size_t)oh;
            uint8_t *a = malloc(bytes), *b = malloc(bytes);
            if (!a || !b) exit(2);
            int rc;
            if (sr == 3)
                rc = jpgx_pixels_host_gray_scaled(coef, w, h, d, qt[0], a, pitch, channels, 1) ||
                     jpgx_pixels_host_gray_scaled(coef, w, h, d, qt[0], b, pitch, channels, 3);
            else
                rc = jpgx_pixels_host_scaled(coef, w, h, sr, d, qt, a, pitch, 1) ||
                     jpgx_pixels_host_scaled(coef, w, h, sr, d, qt, b, pitch, 3);
            if (rc) {
                printf("pixels_scaled_san: the routine refused %dx%d mode %d scale %d\n", w, h, sr, d);
                exit(1);
            }
            if (memcmp(a, b, bytes)) {
                printf("pixels_scaled_san: the thread count changed the pixels\n");
                exit(1);
            }
            frames++;
            free(a);
            free(b);
        }
    free(coef);
}

int main(void)
{
    static const int sizes[4][2] = {{1, 1}, {17, 9}, {24, 16}, {53, 37}};
    static const int16_t extreme[3] = {32767, -32767, -32768};
    uint64_t seed = 0x7363616C6564ull;
    uint16_t qt[2][64];
    for (int sr = 0; sr < 4; sr++)
        for (int s = 0; s < 4; s++) {
            const int w = sizes[s][0], h = sizes[s][1];
            const size_t n = nblocks(w, h, sr) * 64;
            int16_t *coef = malloc(n * sizeof *coef);
            if (!coef) return 2;
            for (int e = 0; e < 3; e++) {
                for (size_t i = 0; i < n; i++) coef[i] = extreme[e];
                for (int i = 0; i < 128; i++) qt[i / 64][i % 64] = 65535;
                run(coef, w, h, sr, qt);
            }
            for (int f = 0; f < 300; f++) {
                for (size_t i = 0; i < n; i++) coef[i] = (int16_t)(splitmix(&seed) & 0xFFFF);
                for (int i = 0; i < 128; i++) qt[i / 64][i % 64] = (uint16_t)(splitmix(&seed) >> (f % 3 ? 48 : 58));
                run(coef, w, h, sr, qt);
            }
            free(coef);
        }
    printf("frames %ld\npixels_scaled_san: clean\n", frames);
    return 0;
}
