/* jfif_sub_san.c -- TEST INFRASTRUCTURE (tests/test_jfif_read_sub.py): the routines of the decoder
 * that works inside a restart interval (csrc/jx_jfif_sub.h through jpgx_read_jfif_sub of
 * csrc/jpgx_jfif_read.cpp, the host twin of the kernel k_jd_sub) under -fsanitize=address,undefined,
 * as a program of its own.  It runs tests/c/jfif_read_san.c's sweep over the same generated files
 * (the same seeds: 64x64 and 16x16; 4:4:4, 4:2:2, 4:2:0; Annex K.3 and per-image tables; one MCU row
 * per restart interval): every truncation, every file with one restart marker dropped and kFlips
 * single-byte corruptions per file, each read from a buffer of exactly the input's size, with the
 * shapes (16, 2), (64, 256) and the kernel's own.  For every input the status must be
 * jpgx_read_jfif's and, where that is 0, the coefficients and tables too.
 * One more file has no restart intervals and a scan of more than two tiles of 64 x 256 bytes
 * (kBig: 160x128, 4:4:4): kBigFlips corruptions and a stride of truncations of it.  Its line and
 * its corruptions with their results are printed for tests/jfif_sub_cases.py, which regenerates
 * them from the same seeds and holds the GPU test's input to them.
 * Exit status 0 and "jfif_sub_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "jfif_sub_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                      \
        }                                                                  \
    } while (0)

enum { kFlips = 2000, kBig = 200, kBigFlips = 400, kBigW = 160, kBigH = 128 };
#define COEF_SEED 0x6a66696672656164ull /* + file index: jfif_read_san.c's */
#define FLIP_SEED 0x73616e666c697073ull /* + file index */

static const uint32_t kShapes[3][2] = {{16, 2}, {64, 256}, {0, 0}}; /* 0, 0: the kernel's own */

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
static jpgx_jfif_sub_stats seen;        /* what the sweep made the mechanism do, summed (rounds: the most) */

/* n bytes from a buffer of exactly n bytes, as a caller that expects W x H, sr: jpgx_read_jfif, then
 * jpgx_read_jfif_sub in the three shapes.  Returns the status, -100 where the two disagree */
static int decode(const uint8_t *bytes, size_t n, int W, int H, int sr, int16_t **coef_out)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);
    if (!file) return JPGX_ENOMEM;
    if (n) memcpy(file, bytes, n);
    jpgx_jfif_info info;
    int rc = jpgx_jfif_info_of(file, n, &info);
    if (!rc && (info.width != W || info.height != H || info.sample_ratio != sr)) rc = JPGX_EJFIF_HEADER;
    if (!rc) {
        const size_t ncoef = (info.nb_y + 2 * info.nb_c) * 64;
        int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t)), *sub = (int16_t *)malloc(ncoef * sizeof(int16_t));
        uint16_t(*qt)[64] = (uint16_t(*)[64])malloc(4 * 64 * sizeof(uint16_t));
        if (!coef || !sub || !qt) return JPGX_ENOMEM;
        rc = jpgx_read_jfif(file, n, 1, coef, ncoef, qt, &info);
        for (int s = 0; s < 3; s++) {
            jpgx_jfif_sub_stats st;
            jpgx_jfif_info info2;
            const int rc2 = jpgx_read_jfif_sub(file, n, kShapes[s][0], kShapes[s][1], sub, ncoef, qt + 2, &info2,
                                               (n_cases + s) % 2 ? &st : NULL);
            if (rc2 != rc || (!rc && (memcmp(sub, coef, ncoef * sizeof(int16_t)) || memcmp(qt, qt + 2, 128 * sizeof(uint16_t)) ||
                                      memcmp(&info, &info2, sizeof info)))) {
                fprintf(stderr, "jfif_sub_san: shape (%u, %u): %d, jpgx_read_jfif %d, %zu bytes\n", kShapes[s][0],
                        kShapes[s][1], rc2, rc, n);
                rc = -100;
                break;
            }
            if ((n_cases + s) % 2) {
                seen.tiles += st.tiles;
                seen.redecodes += st.redecodes;
                seen.starts_on_stuffing += st.starts_on_stuffing;
                seen.units_across_tile += st.units_across_tile;
                if (st.rounds_max > seen.rounds_max) seen.rounds_max = st.rounds_max;
            }
        }
        free(qt);
        free(sub);
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
                int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t)), *back = NULL;
                CHECK(coef);
                for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(idx, i);
                const size_t cap = jpgx_jfif_bound(W, H);
                uint8_t *f = (uint8_t *)malloc(cap);
                size_t len = 0;
                CHECK(f);
                CHECK(jpgx_write_jfif_opt(coef, W, H, 75, sr, 1, 1, opt ? JPGX_JFIF_OPTIMIZE : 0u, f, cap, &len) == 0);
                CHECK(decode(f, len, W, H, sr, &back) == 0 && back);
                CHECK(memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
                free(back);
                /* every truncation */
                for (size_t n = 0; n < len; n++) {
                    const int rc = decode(f, n, W, H, sr, NULL);
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
                        CHECK(decode(g, len - 2, W, H, sr, NULL) == JPGX_EJFIF_SCAN);
                        dropped++;
                    }
                CHECK(dropped == H / (sr == 2 ? 16 : 8) - 1);
                /* single-byte corruptions: jfif_read_san.c's */
                for (int k = 0; k < kFlips; k++) {
                    const size_t pos = (size_t)(splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 1) % len);
                    const uint8_t val = (uint8_t)(f[pos] ^ (1 + splitmix(FLIP_SEED + (uint64_t)idx, 2 * (uint64_t)k + 2) % 255));
                    memcpy(g, f, len);
                    g[pos] = val;
                    CHECK(known(decode(g, len, W, H, sr, NULL)));
                }
                free(g);
                free(f);
                free(coef);
            }
    /* no restart intervals, more than two tiles of the kernel's shape */
    {
        const int W = kBigW, H = kBigH;
        const size_t nb = (size_t)(W / 8) * (H / 8), ncoef = 3 * nb * 64;
        int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t)), *back = NULL;
        const size_t cap = jpgx_jfif_bound(W, H);
        uint8_t *f = (uint8_t *)malloc(cap), *g = (uint8_t *)malloc(cap);
        size_t len = 0;
        CHECK(coef && f && g);
        for (size_t i = 0; i < ncoef; i++) coef[i] = coef_at(kBig, i);
        CHECK(jpgx_write_jfif_sub(coef, W, H, 75, 0, f, cap, &len) == 0);
        jpgx_jfif_info info;
        CHECK(jpgx_jfif_info_of(f, len, &info) == 0 && info.restart_interval == 0);
        CHECK(len - 2 - info.scan_offset > 2 * 64 * 256);
        printf("file %d %d %d %d %d %zu %016llx\n", kBig, W, H, 0, 0, len, (unsigned long long)fnv1a(f, len));
        CHECK(decode(f, len, W, H, 0, &back) == 0 && back && memcmp(back, coef, ncoef * sizeof(int16_t)) == 0);
        free(back);
        for (size_t n = 0; n < len; n += n + 64 < len ? 251 : 1) CHECK(decode(f, n, W, H, 0, NULL) != 0);
        for (int k = 0; k < kBigFlips; k++) {
            const size_t pos = (size_t)(splitmix(FLIP_SEED + kBig, 2 * (uint64_t)k + 1) % len);
            const uint8_t val = (uint8_t)(f[pos] ^ (1 + splitmix(FLIP_SEED + kBig, 2 * (uint64_t)k + 2) % 255));
            memcpy(g, f, len);
            g[pos] = val;
            const int rc = decode(g, len, W, H, 0, NULL);
            CHECK(known(rc));
            printf("flip %d %d %zu %u %d\n", kBig, k, pos, (unsigned)val, rc);
        }
        free(g);
        free(f);
        free(coef);
    }
    /* argument checks */
    {
        uint8_t b[4] = {0xff, 0xd8, 0xff, 0xd9};
        int16_t c[64];
        uint32_t S = 0, T = 0;
        jpgx_jfif_decode_sub_shape(&S, &T);
        CHECK(S >= 16 && S % 16 == 0 && T >= 2);
        CHECK(jpgx_read_jfif_sub(NULL, 4, 0, 0, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 0, 0, NULL, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 15, 2, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 16, 1, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 64, 0, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 1u << 16, 1u << 16, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub(b, 4, 0, 0, c, 64, NULL, NULL, NULL) == JPGX_EJFIF_HEADER);
        CHECK(jpgx_read_jfif_sub(b, 4, 16, 2, c, 64, NULL, NULL, NULL) == JPGX_EJFIF_HEADER);
    }
    printf("cases %ld ok %ld header %ld scan %ld\n", n_cases, n_ok, n_header, n_scan);
    printf("seen tiles %llu redecodes %llu rounds_max %llu starts_on_stuffing %llu units_across_tile %llu\n",
           (unsigned long long)seen.tiles, (unsigned long long)seen.redecodes, (unsigned long long)seen.rounds_max,
           (unsigned long long)seen.starts_on_stuffing, (unsigned long long)seen.units_across_tile);
    CHECK(n_cases >= 20000 && n_ok + n_header + n_scan == n_cases);
    CHECK(seen.redecodes && seen.rounds_max >= 3 && seen.starts_on_stuffing && seen.units_across_tile);
    puts("jfif_sub_san: clean");
    return 0;
}
