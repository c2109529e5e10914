/* any_san.c -- TEST INFRASTRUCTURE (tests/test_any_size.py): the decode side's host routines for
 * files of any width and height (jpgx_jfif_info_of_any, jpgx_read_jfif_any, jpgx_read_jfif_sub_any,
 * jpgx_pixels_host_any) under -fsanitize=address,undefined, as a program of
 * its own.  It writes 32 x 32 files with jpgx_write_jfif_opt (4:4:4, 4:2:2, 4:2:0; Annex K.3 and
 * per-image tables; one MCU row per restart interval) and patches the SOF to every size inside the
 * last MCU: each is a valid file of that size whose coded frame is the 32 x 32 one.  Every such file
 * is decoded by both readers, the twin in the kernel's shape and in (16, 2), into buffers of
 * exactly the coded frame's size, back to the coefficients it was written from, and turned into
 * pixels in a buffer of exactly height x 3 width bytes.  Then every truncation and kFlips
 * single-byte corruptions of two of the files: the two readers' statuses must be equal, one of 0,
 * JPGX_EJFIF_HEADER, JPGX_EJFIF_SCAN, and a status-0 frame's coefficients equal; those go through
 * the pixel routine as well.  The caller states the geometry, as the device entry point's caller
 * does: a header that parses to another one counts as a header error.
 * Exit status 0 and "any_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "any_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                 \
        }                                                             \
    } while (0)

enum { kSide = 32, kFlips = 1500 };
#define COEF_SEED 0x616e7973697a6531ull /* + file index */
#define FLIP_SEED 0x616e79666c697073ull /* + file index */

static uint64_t splitmix(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + k * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* coefficient i of file `idx`: inside the writers' clamps, so the decoders return it */
static int16_t coef_at(int idx, size_t i)
{
    const uint64_t r = splitmix(COEF_SEED + (uint64_t)idx, i + 1);
    if (i % 64 == 0) return (int16_t)((int)(r % 601) - 300);
    const int t = (int)(r % 64);
    if (t < 40) return 0;
    if (t < 62) return (int16_t)(t - 51);
    return (int16_t)((int)((r >> 8) % 2001) - 1000);
}

/* the SOF's height and width replaced */
static int patch(uint8_t *f, size_t len, int W, int H)
{
    size_t i = 2;
    while (i + 9 < len && f[i + 1] != 0xc0 && f[i + 1] != 0xc1) i += 2 + ((size_t)f[i + 2] << 8 | f[i + 3]);
    if (i + 9 >= len) return 1;
    f[i + 5] = (uint8_t)(H >> 8), f[i + 6] = (uint8_t)H, f[i + 7] = (uint8_t)(W >> 8), f[i + 8] = (uint8_t)W;
    return 0;
}

static long n_cases, n_ok, n_header, n_scan, n_pixels;

/* the pixels of a decoded frame, into exactly H rows of 3 W bytes */
static int pixels(const int16_t *coef, int W, int H, int sr, const uint16_t qt[2][64], int threads)
{
    uint8_t *rgb = (uint8_t *)malloc((size_t)H * 3 * (size_t)W);
    if (!rgb) return JPGX_ENOMEM;
    const int rc = jpgx_pixels_host_any(coef, W, H, sr, qt, rgb, 3 * (size_t)W, threads);
    free(rgb);
    n_pixels++;
    return rc;
}

/* `n` bytes from a buffer of exactly n bytes, as a caller that expects W x H, sr, by both readers:
 * the statuses must agree; *coef_out: the frame when the status is 0 (the caller frees it) */
static int decode(const uint8_t *bytes, size_t n, int W, int H, int sr, uint32_t sub_bytes, uint32_t tile_subs,
                  int16_t **coef_out, int *rc_out)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);
    CHECK(file);
    if (n) memcpy(file, bytes, n);
    jpgx_jfif_info info;
    int rc = jpgx_jfif_info_of_any(file, n, &info);
    if (!rc && (info.width != W || info.height != H || info.sample_ratio != sr)) rc = JPGX_EJFIF_HEADER;
    if (!rc) {
        int cw = 0, ch = 0;
        CHECK(jpgx_coded_size(W, H, sr, &cw, &ch) == 0);
        CHECK(info.nb_y == (size_t)(cw / 8) * (size_t)(ch / 8));
        CHECK(info.nb_c == info.nb_y / (sr == 0 ? 1u : sr == 1 ? 2u : 4u));
        const size_t ncoef = (info.nb_y + 2 * info.nb_c) * 64;
        int16_t *a = (int16_t *)malloc(ncoef * sizeof(int16_t)), *b = (int16_t *)malloc(ncoef * sizeof(int16_t));
        uint16_t(*qa)[64] = (uint16_t(*)[64])malloc(128 * sizeof(uint16_t));
        uint16_t(*qb)[64] = (uint16_t(*)[64])malloc(128 * sizeof(uint16_t));
        CHECK(a && b && qa && qb);
        jpgx_jfif_info ia, ib;
        rc = jpgx_read_jfif_any(file, n, 1 + (int)(n % 3), a, ncoef, qa, &ia);
        const int rs = jpgx_read_jfif_sub_any(file, n, sub_bytes, tile_subs, b, ncoef, qb, &ib, NULL);
        CHECK(rc == rs);
        CHECK(memcmp(&ia, &info, sizeof info) == 0 && memcmp(&ib, &info, sizeof info) == 0);
        CHECK(memcmp(qa, qb, 128 * sizeof(uint16_t)) == 0);
        if (!rc) {
            CHECK(memcmp(a, b, ncoef * sizeof(int16_t)) == 0);
            CHECK(pixels(a, W, H, sr, (const uint16_t(*)[64])qa, 1 + (int)(n % 2)) == 0);
        }
        free(qa);
        free(qb);
        free(b);
        if (coef_out && !rc) *coef_out = a;
        else free(a);
    }
    free(file);
    n_cases++;
    n_ok += rc == 0;
    n_header += rc == JPGX_EJFIF_HEADER;
    n_scan += rc == JPGX_EJFIF_SCAN;
    *rc_out = rc;
    return 0;
}

int main(void)
{
    int idx = 0, rc = 0;
    for (int sr = 0; sr <= 2; sr++)
        for (int opt = 0; opt <= 1; opt++, idx++) {
            const int mw = sr ? 16 : 8, mh = sr == 2 ? 16 : 8;
            const size_t nb = (size_t)(kSide / 8) * (kSide / 8), nbc = sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4;
            const size_t ncoef = (nb + 2 * nbc) * 64;
            int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t));
            CHECK(coef);
            for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(idx, i);
            const size_t cap = jpgx_jfif_bound(kSide, kSide);
            uint8_t *f = (uint8_t *)malloc(cap), *g = (uint8_t *)malloc(cap);
            size_t len = 0;
            CHECK(f && g);
            CHECK(jpgx_write_jfif_opt(coef, kSide, kSide, 75, sr, 1, 1, opt ? JPGX_JFIF_OPTIMIZE : 0u, f, cap, &len) == 0);

            /* every size inside the last MCU, the whole one included */
            for (int H = kSide - mh + 1; H <= kSide; H++)
                for (int W = kSide - mw + 1; W <= kSide; W++) {
                    CHECK(patch(f, len, W, H) == 0);
                    for (int shape = 0; shape < 2; shape++) {
                        int16_t *back = NULL;
                        CHECK(decode(f, len, W, H, sr, shape ? 16u : 0u, shape ? 2u : 0u, &back, &rc) == 0);
                        CHECK(rc == 0 && back && memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
                        free(back);
                    }
                    /* the plain readers refuse all but the whole one, and agree on that */
                    jpgx_jfif_info info;
                    const int plain = jpgx_jfif_info_of(f, len, &info);
                    CHECK(plain == (W == kSide && H == kSide ? 0 : JPGX_EJFIF_HEADER));
                    /* another stated geometry is a header error */
                    CHECK(decode(f, len, W == 1 ? 2 : W - 1, H, sr, 0u, 0u, NULL, &rc) == 0 && rc == JPGX_EJFIF_HEADER);
                }

            /* truncations and corruptions of two of the files, at a size odd in both directions */
            if (idx == 1 || idx == 4) {
                const int W = kSide - mw + 3, H = kSide - 3;
                CHECK(patch(f, len, W, H) == 0);
                for (size_t n = 0; n < len; n++) {
                    CHECK(decode(f, n, W, H, sr, n % 2 ? 16u : 0u, n % 2 ? 2u : 0u, NULL, &rc) == 0);
                    CHECK(rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN);
                }
                for (int k = 0; k < kFlips; k++) {
                    const size_t pos = (size_t)(splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 1) % len);
                    const uint8_t val = (uint8_t)(f[pos] ^ (1 + splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 2) % 255));
                    memcpy(g, f, len);
                    g[pos] = val;
                    CHECK(decode(g, len, W, H, sr, k % 2 ? 16u : 0u, k % 2 ? 2u : 0u, NULL, &rc) == 0);
                    CHECK(rc == 0 || rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN);
                }
            }
            free(g);
            free(f);
            free(coef);
        }
    /* argument checks */
    {
        uint8_t b[4] = {0xff, 0xd8, 0xff, 0xd9}, px[3];
        int16_t c[3 * 64] = {0};
        uint16_t qt[2][64];
        jpgx_jfif_info info;
        int cw, ch;
        for (int k = 0; k < 128; k++) qt[k / 64][k % 64] = 1;
        CHECK(jpgx_jfif_info_of_any(NULL, 4, &info) == JPGX_EARG && jpgx_jfif_info_of_any(b, 4, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_any(NULL, 4, 1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_any(b, 4, 1, NULL, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_any(b, 4, -1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_any(b, 4, 1, c, 64, NULL, NULL) == JPGX_EJFIF_HEADER);
        CHECK(jpgx_read_jfif_sub_any(b, 4, 15, 2, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub_any(b, 4, 0, 0, c, 64, NULL, NULL, NULL) == JPGX_EJFIF_HEADER);
        CHECK(jpgx_pixels_host_any(c, 1, 1, 0, (const uint16_t(*)[64])qt, px, 3, 1) == 0);
        CHECK(jpgx_pixels_host_any(c, 1, 1, 0, (const uint16_t(*)[64])qt, px, 2, 1) == JPGX_EARG);
        CHECK(jpgx_pixels_host_any(c, 0, 1, 0, (const uint16_t(*)[64])qt, px, 3, 1) == JPGX_EGEOMETRY);
        CHECK(jpgx_pixels_host_any(c, 1, 65536, 0, (const uint16_t(*)[64])qt, px, 3, 1) == JPGX_EGEOMETRY);
        CHECK(jpgx_pixels_host_any(c, 1, 1, 3, (const uint16_t(*)[64])qt, px, 3, 1) == JPGX_ESAMPLE);
        CHECK(jpgx_coded_size(17, 9, 2, &cw, &ch) == 0 && cw == 32 && ch == 16);
        CHECK(jpgx_coded_size(65535, 1, 1, &cw, &ch) == 0 && cw == 65536 && ch == 8);
        CHECK(jpgx_coded_size(0, 1, 0, &cw, &ch) == JPGX_EARG && jpgx_coded_size(1, 1, 3, &cw, &ch) == JPGX_EARG);
        CHECK(jpgx_coded_size(1, 1, 0, NULL, &ch) == JPGX_EARG);
    }
    printf("cases %ld ok %ld header %ld scan %ld pixels %ld\n", n_cases, n_ok, n_header, n_scan, n_pixels);
    CHECK(n_cases >= 8000 && n_ok + n_header + n_scan == n_cases && n_pixels >= n_ok);
    puts("any_san: clean");
    return 0;
}
