/* jfif_header_san.c -- TEST INFRASTRUCTURE (tests/test_jfif_gpu.py): the JFIF writer's shared table
 * and header functions (host/jpgx_jfif.c, declared in csrc/jpgx_internal.h) under
 * -fsanitize=address,undefined, as a program of its own: the header bytes for q = 1, 23, 24, 97 at
 * sample ratios 0 / 1 / 2 with and without DRI, into exact-size, short and empty buffers, checked
 * against jpgx_write_jfif_ex's own leading bytes; the packed code tables; one whole file.
 * Exit status 0 and "jfif_header_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"
#include "../../jpeg-encoder-and-decoder_amd/csrc/jpgx_internal.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "jfif_header_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main(void)
{
    static const int qs[4] = {1, 23, 24, 97};
    const int W = 32, H = 16;
    const size_t ncoef = (size_t)(W / 8) * (H / 8) * 3 * 64;
    int16_t *coef = (int16_t *)calloc(ncoef, sizeof(int16_t));
    CHECK(coef);
    for (size_t i = 0; i < ncoef; i++) coef[i] = (int16_t)((i * 2654435761u >> 20) % 7) - 3;

    for (int qi = 0; qi < 4; qi++)
        for (int sr = 0; sr <= 2; sr++)
            for (int dri = 0; dri <= 1; dri++) {
                const int q = qs[qi];
                const unsigned cpr = (unsigned)W / (sr ? 16 : 8);
                const unsigned ri = dri ? cpr : 0u;
                const size_t n = jx_jfif_header(W, H, q, sr, ri, NULL, 0);      /* length only */
                const size_t want = (size_t)(q <= 23 ? 751 : 623) + (dri ? 6 : 0);
                CHECK(n == want && n <= JX_JFIF_HDR_MAX);
                uint8_t *exact = (uint8_t *)malloc(n);                          /* exact size */
                uint8_t *shrt = (uint8_t *)malloc(n - 5);                       /* too short */
                CHECK(exact && shrt);
                CHECK(jx_jfif_header(W, H, q, sr, ri, exact, n) == n);
                CHECK(jx_jfif_header(W, H, q, sr, ri, shrt, n - 5) == n);
                CHECK(memcmp(exact, shrt, n - 5) == 0);
                CHECK(exact[0] == 0xff && exact[1] == 0xd8 && exact[n - 14] == 0xff && exact[n - 13] == 0xda);
                if (dri) {
                    CHECK(exact[n - 20] == 0xff && exact[n - 19] == 0xdd);
                    CHECK(((unsigned)exact[n - 16] << 8 | exact[n - 15]) == ri);
                }
                if (sr == 0) {      /* the writer's file begins with exactly these bytes */
                    const size_t cap = jpgx_jfif_bound(W, H);
                    uint8_t *file = (uint8_t *)malloc(cap);
                    size_t len = 0;
                    CHECK(file);
                    CHECK(jpgx_write_jfif_ex(coef, W, H, q, 0, dri ? 1 : 0, 1, file, cap, &len) == JPGX_OK);
                    CHECK(len > n + 2 && memcmp(file, exact, n) == 0);
                    CHECK(file[len - 2] == 0xff && file[len - 1] == 0xd9);
                    free(file);
                }
                free(exact);
                free(shrt);
            }
    CHECK(jx_jfif_header(W, H, 0, 0, 0, NULL, 0) == 0 && jx_jfif_header(W, H, 98, 0, 0, NULL, 0) == 0);

    uint32_t (*cl)[256] = (uint32_t (*)[256])malloc(4 * sizeof *cl);           /* exact size */
    CHECK(cl);
    jx_jfif_codes(cl);
    CHECK(cl[0][0] == (0x0u << 8 | 2) && cl[2][0] == (0x0u << 8 | 2));         /* K.3, K.4: category 0 */
    CHECK(cl[1][0x00] == (0xau << 8 | 4) && cl[1][0xf0] == (0x7f9u << 8 | 11)); /* K.5: EOB, ZRL */
    CHECK(cl[3][0x00] == (0x0u << 8 | 2) && cl[3][0xf0] == (0x3fau << 8 | 10)); /* K.6: EOB, ZRL */
    for (int t = 0; t < 4; t++) {
        int used = 0;
        for (int s = 0; s < 256; s++) {
            const uint32_t len = cl[t][s] & 0xff;
            CHECK(len <= 16 && (len == 0 || (cl[t][s] >> 8) < (1u << len)));
            used += len != 0;
        }
        CHECK(used == ((t & 1) ? 162 : 12));
    }
    free(cl);
    free(coef);
    puts("jfif_header_san: clean");
    return 0;
}
