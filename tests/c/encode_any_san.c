/* encode_any_san.c -- TEST INFRASTRUCTURE (tests/test_encode_any.py): the encode side's host routines
 * for images of any width and height (jpgx_pad_edge, jpgx_write_jfif_any) under
 * -fsanitize=address,undefined, as a program of its own.  For every size 1 .. 40 x 1 .. 40 and the
 * sizes of the tests, in the three samplings: an image whose rows are 3 W + 5 bytes apart, in a buffer
 * that ends with its last pixel, is padded into a buffer of exactly the coded frame's bytes and
 * compared with the edge rule; the coded frame's coefficients, in a buffer of exactly their size, are
 * written twice -- into a buffer one byte short, which must report the size needed, and into one of
 * exactly that size -- with restart intervals, tables and thread counts taken in turn; the file is
 * read back (jpgx_read_jfif_any) to the size and the coefficients it was written from, and for a size
 * that is a multiple of the MCU it must be jpgx_write_jfif_opt's.
 * Exit status 0 and "encode_any_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "encode_any_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                        \
        }                                                                    \
    } while (0)

#define SEED 0x656e63616e797331ull

static uint64_t splitmix(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + k * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* coefficient i of case `idx`: inside the writers' clamps, so the reader returns it */
static int16_t coef_at(long idx, size_t i)
{
    const uint64_t r = splitmix(SEED + (uint64_t)idx, i + 1);
    if (i % 64 == 0) return (int16_t)((int)(r % 601) - 300);
    const int t = (int)(r % 64);
    if (t < 40) return 0;
    if (t < 62) return (int16_t)(t - 51);
    return (int16_t)((int)((r >> 8) % 2001) - 1000);
}

static long n_sizes, n_files;

static int one_size(int W, int H, int sr)
{
    const long idx = n_sizes++;
    int cw = 0, ch = 0;
    CHECK(jpgx_coded_size(W, H, sr, &cw, &ch) == 0);

    /* the edge rule */
    const size_t pitch = 3 * (size_t)W + 5, nsrc = pitch * (size_t)(H - 1) + 3 * (size_t)W;
    const size_t ncoded = 3 * (size_t)cw * (size_t)ch;
    uint8_t *rgb = (uint8_t *)malloc(nsrc), *coded = (uint8_t *)malloc(ncoded);
    CHECK(rgb && coded);
    for (size_t i = 0; i < nsrc; i++) rgb[i] = (uint8_t)splitmix(SEED ^ (uint64_t)idx, i);
    CHECK(jpgx_pad_edge(rgb, W, H, pitch, cw, ch, coded) == 0);
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            const size_t sy = (size_t)(y < H ? y : H - 1), sx = (size_t)(x < W ? x : W - 1);
            CHECK(memcmp(coded + ((size_t)y * (size_t)cw + (size_t)x) * 3, rgb + sy * pitch + 3 * sx, 3) == 0);
        }
    free(coded);
    free(rgb);

    /* the file */
    const size_t nb = (size_t)(cw / 8) * (size_t)(ch / 8), nbc = sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4;
    const size_t ncoef = (nb + 2 * nbc) * 64;
    int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t)), *back = (int16_t *)malloc(ncoef * sizeof(int16_t));
    CHECK(coef && back);
    for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(idx, i);
    const int rr = (int)(idx % 4) - 1, threads = 1 + (int)(idx % 3), q = idx % 2 ? 50 : 90;
    const unsigned flags = idx % 5 < 2 ? JPGX_JFIF_OPTIMIZE : 0u;
    size_t need = 0, len = 0;
    uint8_t *probe = (uint8_t *)malloc(1);
    CHECK(probe);
    CHECK(jpgx_write_jfif_any(coef, W, H, q, sr, rr, threads, flags, probe, 0, &need) == JPGX_EARG);
    free(probe);
    CHECK(need > 0 && need <= jpgx_jfif_bound(cw, ch));
    uint8_t *shy = (uint8_t *)malloc(need - 1), *file = (uint8_t *)malloc(need);
    CHECK(shy && file);
    CHECK(jpgx_write_jfif_any(coef, W, H, q, sr, rr, threads, flags, shy, need - 1, &len) == JPGX_EARG && len == need);
    CHECK(jpgx_write_jfif_any(coef, W, H, q, sr, rr, threads, flags, file, need, &len) == 0 && len == need);
    CHECK(memcmp(shy, file, need - 1) == 0);
    free(shy);
    n_files++;
    jpgx_jfif_info info;
    uint16_t qt[2][64];
    CHECK(jpgx_read_jfif_any(file, len, 1, back, ncoef, qt, &info) == 0);
    CHECK(info.width == W && info.height == H && info.sample_ratio == sr && info.nb_y == nb && info.nb_c == nbc);
    CHECK(memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
    if (W == cw && H == ch) {
        uint8_t *plain = (uint8_t *)malloc(need);
        CHECK(plain);
        CHECK(jpgx_write_jfif_opt(coef, W, H, q, sr, rr, threads, flags, plain, need, &len) == 0 && len == need);
        CHECK(memcmp(plain, file, need) == 0);
        free(plain);
    } else {
        CHECK(jpgx_write_jfif_opt(coef, W, H, q, sr, rr, threads, flags, file, need, &len) != 0);
    }
    free(file);
    free(back);
    free(coef);
    return 0;
}

int main(void)
{
    static const int extra[][2] = {{1, 1}, {3, 5}, {8, 8}, {17, 15}, {16, 33}, {33, 16}, {30, 22}, {129, 65},
                                   {263, 21}, {667, 9}};
    for (int sr = 0; sr <= 2; sr++) {
        for (int H = 1; H <= 40; H++)
            for (int W = 1; W <= 40; W++) CHECK(one_size(W, H, sr) == 0);
        for (size_t k = 0; k < sizeof extra / sizeof extra[0]; k++) CHECK(one_size(extra[k][0], extra[k][1], sr) == 0);
    }
    /* argument checks */
    {
        uint8_t px[3] = {1, 2, 3}, out[8 * 8 * 3], f[2048];
        int16_t c[3 * 64] = {0};
        size_t len = 0;
        CHECK(jpgx_pad_edge(px, 1, 1, 3, 8, 8, out) == 0 && out[0] == 1 && out[191] == 3);
        CHECK(jpgx_pad_edge(NULL, 1, 1, 3, 8, 8, out) == JPGX_EARG && jpgx_pad_edge(px, 1, 1, 3, 8, 8, NULL) == JPGX_EARG);
        CHECK(jpgx_pad_edge(px, 1, 1, 2, 8, 8, out) == JPGX_EARG);
        CHECK(jpgx_pad_edge(px, 0, 1, 3, 8, 8, out) == JPGX_EGEOMETRY && jpgx_pad_edge(px, 1, 1, 3, 0, 8, out) == JPGX_EGEOMETRY);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 50, 0, 0, 1, 0u, f, sizeof f, &len) == 0 && len > 0);
        CHECK(jpgx_write_jfif_any(NULL, 1, 1, 50, 0, 0, 1, 0u, f, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 50, 0, 0, 1, 0u, NULL, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_write_jfif_any(c, 0, 1, 50, 0, 0, 1, 0u, f, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_write_jfif_any(c, 1, 65536, 50, 0, 0, 1, 0u, f, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 50, 3, 0, 1, 0u, f, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 0, 0, 0, 1, 0u, f, sizeof f, &len) == JPGX_EQUALITY);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 98, 0, 0, 1, 0u, f, sizeof f, &len) == JPGX_EQUALITY);
        CHECK(jpgx_write_jfif_any(c, 1, 1, 50, 0, 0, 1, 2u, f, sizeof f, &len) == JPGX_EARG);
        CHECK(jpgx_encode_rgb_to_jpeg_any(px, 1, 1, 3, "/nonexistent-directory/x.jpg", 50, 3, 0u, 0) == JPGX_ESAMPLE);
        CHECK(jpgx_encode_rgb_to_jpeg_any(px, 1, 1, 3, "/nonexistent-directory/x.jpg", 50, 0, 0u, 0) == JPGX_ENODEV);
    }
    printf("sizes %ld files %ld\n", n_sizes, n_files);
    puts("encode_any_san: clean");
    return 0;
}
