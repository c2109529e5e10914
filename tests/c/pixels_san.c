/*
 * pixels_san.c -- jpgx_pixels_host (csrc/jpgx_pixels_host.cpp, csrc/jx_idct.h) under
 * AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_pixels.py builds this program with the
 * host pixel source under -fsanitize=address,undefined -fno-sanitize-recover=undefined and runs it.
 * The arithmetic is specified to wrap, so every input must run without a report: hostile values
 * (every coefficient +-32767 under a table of 65535, one extreme coefficient per position under
 * table entries 1, 255 and 65535, an all-zero table) and 2,000 random frames per sample mode at
 * 16x16 and 48x32.  The coefficient and output buffers are exactly their sizes.
 * Ends with "pixels_san: clean".
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

static uint64_t hash = 0xCBF29CE484222325ull;
static long frames = 0;

static size_t nblocks(int w, int h, int sr)
{
    const size_t nb = (size_t)(w / 8) * (size_t)(h / 8);
    return nb + 2 * (sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4);
}

/* one frame through the routine: fresh buffers of exactly the sizes, 1 and 3 threads must agree */
static void run(const int16_t *src, int w, int h, int sr, const uint16_t qt[2][64])
{
    const size_t n = nblocks(w, h, sr) * 64, bytes = (size_t)w * 3 * (size_t)h;
    int16_t *coef = malloc(n * sizeof *coef);
    uint8_t *a = malloc(bytes), *b = malloc(bytes);
    if (!coef || !a || !b) exit(2);
    memcpy(coef, src, n * sizeof *coef);
    if (jpgx_pixels_host(coef, w, h, sr, qt, a, (size_t)w * 3, 1) || jpgx_pixels_host(coef, w, h, sr, qt, b, (size_t)w * 3, 3)) {
        printf("pixels_san: the routine refused %dx%d mode %d\n", w, h, sr);
        exit(1);
    }
    if (memcmp(a, b, bytes)) {
        printf("pixels_san: the thread count changed the pixels\n");
        exit(1);
    }
    for (size_t i = 0; i < bytes; i++) hash = (hash ^ a[i]) * 0x100000001B3ull;
    frames++;
    free(coef);
    free(a);
    free(b);
}

int main(void)
{
    static const int sizes[2][2] = {{16, 16}, {48, 32}};
    static const int16_t extreme[3] = {32767, -32767, -32768};
    static const uint16_t entry[3] = {1, 255, 65535};
    static int16_t coef[(48 / 8) * (32 / 8) * 3 * 64];
    uint16_t qt[2][64];
    for (int sr = 0; sr < 3; sr++)
        for (int z = 0; z < 2; z++) {
            const int w = sizes[z][0], h = sizes[z][1];
            const size_t n = nblocks(w, h, sr) * 64;
            /* every coefficient +-32767, every table entry 65535 */
            for (int sign = 0; sign < 3; sign++) {
                for (size_t i = 0; i < n; i++) coef[i] = sign == 2 ? ((i & 1) ? 32767 : -32767) : extreme[sign];
                for (int i = 0; i < 128; i++) (&qt[0][0])[i] = 65535;
                run(coef, w, h, sr, qt);
            }
            /* one extreme coefficient per position (in every block), table entry 1, 255, 65535 */
            for (int k = 0; k < 64; k++)
                for (int v = 0; v < 3; v++)
                    for (int e = 0; e < 3; e++) {
                        memset(coef, 0, n * sizeof *coef);
                        for (size_t blk = 0; blk < n / 64; blk++) coef[blk * 64 + (size_t)k] = extreme[v];
                        for (int i = 0; i < 128; i++) (&qt[0][0])[i] = entry[e];
                        run(coef, w, h, sr, qt);
                    }
            /* an all-zero table */
            for (size_t i = 0; i < n; i++) coef[i] = (int16_t)(i * 2654435761u >> 16);
            memset(qt, 0, sizeof qt);
            run(coef, w, h, sr, qt);
            /* random frames: full-range coefficients, full-range tables */
            uint64_t s = 0x706978656C73ull + (uint64_t)(sr * 2 + z);
            for (int f = 0; f < 2000; f++) {
                for (size_t i = 0; i < n; i += 4) {
                    const uint64_t r = splitmix(&s);
                    for (int j = 0; j < 4; j++) coef[i + (size_t)j] = (int16_t)(uint16_t)(r >> (16 * j));
                }
                for (int i = 0; i < 128; i += 4) {
                    const uint64_t r = splitmix(&s);
                    for (int j = 0; j < 4; j++) (&qt[0][0])[i + j] = (f & 1) ? (uint16_t)(r >> (16 * j)) : (uint16_t)((r >> (16 * j)) & 255u);
                }
                run(coef, w, h, sr, qt);
            }
        }
    printf("frames %ld hash %016llx\n", frames, (unsigned long long)hash);
    printf("pixels_san: clean\n");
    return 0;
}
