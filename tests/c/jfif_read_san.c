/* jfif_read_san.c -- TEST INFRASTRUCTURE (tests/test_jfif_read.py): the JFIF decoder's shared
 * routines (csrc/jx_jfif_dec.h through jpgx_read_jfif of csrc/jpgx_jfif_read.cpp) under
 * -fsanitize=address,undefined, as a program of its own.  It writes small files (64x64 and 16x16;
 * 4:4:4, 4:2:2, 4:2:0; Annex K.3 and per-image tables; one MCU row per restart interval), decodes
 * each back to the coefficients it was written from, then decodes, from buffers of exactly the
 * input's size: every truncation of each file, every file with one restart marker dropped, and
 * kFlips single-byte corruptions per file drawn from a splitmix64 stream of fixed seed.  Each
 * result must be 0, JPGX_EJFIF_HEADER or JPGX_EJFIF_SCAN.  The caller states the geometry, as the
 * device entry point's caller does: a header that parses to another geometry counts as a header
 * error, otherwise the coefficient buffer has exactly the frame's size.
 * Prints, for tests/test_jfif_read.py and tests/test_jfif_decode_gpu.py, which regenerate them from
 * the same seeds: a line per file (index, geometry, length, FNV-1a hash of its bytes) and its
 * first kShown corruptions with their results.  Exit status 0 and "jfif_read_san: clean" when
 * everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "jfif_read_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                       \
        }                                                                   \
    } while (0)

enum { kFlips = 2000, kShown = 48 };
#define COEF_SEED 0x6a66696672656164ull /* + file index */
#define FLIP_SEED 0x73616e666c697073ull /* + file index */

/* splitmix64: the k-th output (k = 1, 2, ...) of the stream that starts at seed */
static uint64_t splitmix(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + k * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint64_t fnv1a(const uint8_t *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

/* coefficient i of file `idx`: inside the writers' clamps, so the decoder returns it */
static int16_t coef_at(int idx, size_t i)
{
    const uint64_t r = splitmix(COEF_SEED + (uint64_t)idx, i + 1);
    if (i % 64 == 0) return (int16_t)((int)(r % 601) - 300);
    const int t = (int)(r % 64);
    if (t < 40) return 0;
    if (t < 62) return (int16_t)(t - 51);
    return (int16_t)((int)((r >> 8) % 2001) - 1000);
}

static long n_cases, n_ok, n_header, n_scan;

/* decode `n` bytes from a buffer of exactly n bytes, as a caller that expects W x H, sr */
static int decode(const uint8_t *bytes, size_t n, int W, int H, int sr, int threads, int16_t **coef_out)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);
    if (!file) return JPGX_ENOMEM;
    if (n) memcpy(file, bytes, n);
    jpgx_jfif_info info;
    int rc = jpgx_jfif_info_of(file, n, &info);
    if (!rc && (info.width != W || info.height != H || info.sample_ratio != sr)) rc = JPGX_EJFIF_HEADER;
    if (!rc) {
        const size_t ncoef = (info.nb_y + 2 * info.nb_c) * 64;
        int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t));
        uint16_t(*qt)[64] = (uint16_t(*)[64])malloc(2 * 64 * sizeof(uint16_t));
        if (!coef || !qt) return JPGX_ENOMEM;
        rc = jpgx_read_jfif(file, n, threads, coef, ncoef, qt, &info);
        free(qt);
        if (coef_out && !rc) *coef_out = coef;
        else free(coef);
    }
    free(file);
    n_cases++;
    n_ok += rc == 0;
    n_header += rc == JPGX_EJFIF_HEADER;
    n_scan += rc == JPGX_EJFIF_SCAN;
    return rc;
}

static int known(int rc) { return rc == 0 || rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN; }

int main(void)
{
    int idx = 0;
    for (int big = 1; big >= 0; big--)
        for (int sr = 0; sr <= 2; sr++)
            for (int opt = 0; opt <= 1; opt++, idx++) {
                const int W = big ? 64 : 16, H = W;
                const size_t nb = (size_t)(W / 8) * (H / 8), nbc = sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4;
                const size_t ncoef = (nb + 2 * nbc) * 64;
                int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t));
                CHECK(coef);
                for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(idx, i);
                const size_t cap = jpgx_jfif_bound(W, H);
                uint8_t *f = (uint8_t *)malloc(cap);
                size_t len = 0;
                CHECK(f);
                CHECK(jpgx_write_jfif_opt(coef, W, H, 75, sr, 1, 1, opt ? JPGX_JFIF_OPTIMIZE : 0u, f, cap, &len) == 0);
                printf("file %d %d %d %d %d %zu %016llx\n", idx, W, H, sr, opt, len, (unsigned long long)fnv1a(f, len));

                /* the file itself, on 1 and 3 threads */
                for (int threads = 1; threads <= 3; threads += 2) {
                    int16_t *back = NULL;
                    CHECK(decode(f, len, W, H, sr, threads, &back) == 0 && back);
                    CHECK(memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
                    free(back);
                }
                /* another stated geometry is a header error */
                CHECK(decode(f, len, W + 8, H, sr, 1, NULL) == JPGX_EJFIF_HEADER);

                /* every truncation */
                for (size_t n = 0; n < len; n++) {
                    const int rc = decode(f, n, W, H, sr, 1, NULL);
                    CHECK(rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN);
                }
                /* one restart marker dropped, each in turn */
                jpgx_jfif_info info;
                CHECK(jpgx_jfif_info_of(f, len, &info) == 0);
                uint8_t *g = (uint8_t *)malloc(len);
                CHECK(g);
                int dropped = 0;
                for (size_t p = info.scan_offset; p + 1 < len; p++)
                    if (f[p] == 0xff && (f[p + 1] & 0xf8) == 0xd0) {
                        memcpy(g, f, p);
                        memcpy(g + p, f + p + 2, len - p - 2);
                        CHECK(decode(g, len - 2, W, H, sr, 1, NULL) == JPGX_EJFIF_SCAN);
                        dropped++;
                    }
                CHECK(dropped == H / (sr == 2 ? 16 : 8) - 1);
                /* single-byte corruptions */
                for (int k = 0; k < kFlips; k++) {
                    const size_t pos = (size_t)(splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 1) % len);
                    const uint8_t val = (uint8_t)(f[pos] ^ (1 + splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 2) % 255));
                    memcpy(g, f, len);
                    g[pos] = val;
                    const int rc = decode(g, len, W, H, sr, 1 + k % 2, NULL);
                    CHECK(known(rc));
                    if (k < kShown) printf("flip %d %d %zu %u %d\n", idx, k, pos, (unsigned)val, rc);
                }
                free(g);
                free(f);
                free(coef);
            }
    /* no restart intervals: one interval, whatever the thread count */
    for (int sr = 0; sr <= 2; sr++) {
        const int W = 32, H = 32;
        const size_t nb = 16, nbc = sr == 0 ? nb : sr == 1 ? nb / 2 : nb / 4, ncoef = (nb + 2 * nbc) * 64;
        int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t)), *back = NULL;
        const size_t cap = jpgx_jfif_bound(W, H);
        uint8_t *f = (uint8_t *)malloc(cap);
        size_t len = 0;
        CHECK(coef && f);
        for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(100 + sr, i);
        CHECK(jpgx_write_jfif_sub(coef, W, H, 50, sr, f, cap, &len) == 0);
        CHECK(decode(f, len, W, H, sr, 4, &back) == 0 && back && memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
        for (size_t n = 0; n < len; n++) CHECK(decode(f, n, W, H, sr, 1, NULL) != 0);
        free(back);
        free(f);
        free(coef);
    }
    /* argument checks */
    {
        uint8_t b[4] = {0xff, 0xd8, 0xff, 0xd9};
        int16_t c[64];
        jpgx_jfif_info info;
        CHECK(jpgx_jfif_info_of(NULL, 4, &info) == JPGX_EARG && jpgx_jfif_info_of(b, 4, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif(NULL, 4, 1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif(b, 4, 1, NULL, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif(b, 4, -1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif(b, 4, 1, c, 64, NULL, NULL) == JPGX_EJFIF_HEADER);
    }
    printf("cases %ld ok %ld header %ld scan %ld\n", n_cases, n_ok, n_header, n_scan);
    CHECK(n_cases >= 20000 && n_ok + n_header + n_scan == n_cases);
    puts("jfif_read_san: clean");
    return 0;
}
