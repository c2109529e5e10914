/* gray_san.c -- TEST INFRASTRUCTURE (tests/test_gray.py): the decode side's host routines for
 * one-component files (jpgx_jfif_info_of_gray, jpgx_read_jfif_gray, jpgx_read_jfif_sub_gray,
 * jpgx_pixels_host_gray) under -fsanitize=address,undefined, as a program of
 * its own.  It reads the committed files of tests/golden/gray_fixtures/ (found beside this source file) of
 * at most kMaxFile bytes and runs, for each: the file itself, every prefix, and every single byte
 * replaced by 0x00, by 0xFF and with its low bit flipped.  Each input lies in a buffer of exactly its
 * size and is decoded by the reader and by the twin, in the kernel's shape and in (16, 2), into
 * buffers of exactly the frame's size: the three statuses must be equal, one of 0, JPGX_EJFIF_HEADER,
 * JPGX_EJFIF_SCAN, and a status-0 frame's coefficients and tables equal; such a frame then goes
 * through the pixel routine with 1 and 3 channels into buffers of exactly height x channels x width
 * bytes.  The caller states the fixture's geometry, as the device entry point's caller does: a header
 * that parses to another one counts as a header error.  Before the files, threads(): the host twins'
 * thread fan-out (csrc/jx_par.h) on 0, 1, 3, 64 and, in the writer, 200 threads.
 * Exit status 0 and "gray_san: clean" when everything holds. */
#define _POSIX_C_SOURCE 200809L
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "gray_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                  \
        }                                                              \
    } while (0)

enum { kMaxFile = 700 };

static long n_cases, n_ok, n_header, n_scan, n_pixels;

static int pixels(const int16_t *coef, int W, int H, const uint16_t *qt, int channels, int threads)
{
    uint8_t *out = (uint8_t *)malloc((size_t)H * (size_t)channels * (size_t)W);
    if (!out) return JPGX_ENOMEM;
    const int rc = jpgx_pixels_host_gray(coef, W, H, qt, out, (size_t)channels * (size_t)W, channels, threads);
    free(out);
    n_pixels++;
    return rc;
}

/* `n` bytes from a buffer of exactly n bytes, as a caller that expects W x H */
static int decode(const uint8_t *bytes, size_t n, int W, int H, int *rc_out)
{
    uint8_t *file = (uint8_t *)malloc(n ? n : 1);
    CHECK(file);
    if (n) memcpy(file, bytes, n);
    jpgx_jfif_info info;
    int rc = jpgx_jfif_info_of_gray(file, n, &info);
    if (!rc && (info.width != W || info.height != H)) rc = JPGX_EJFIF_HEADER;
    if (!rc) {
        CHECK(info.sample_ratio == 0 && info.nb_c == 0);
        CHECK(info.nb_y == (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8));
        const size_t ncoef = info.nb_y * 64;
        int16_t *c[3];
        uint16_t *q[3];
        jpgx_jfif_info got[3];
        for (int k = 0; k < 3; k++) {
            c[k] = (int16_t *)malloc(ncoef * sizeof(int16_t));
            q[k] = (uint16_t *)malloc(64 * sizeof(uint16_t));
            CHECK(c[k] && q[k]);
        }
        rc = jpgx_read_jfif_gray(file, n, 1 + (int)(n % 3), c[0], ncoef, q[0], &got[0]);
        const int r1 = jpgx_read_jfif_sub_gray(file, n, 0u, 0u, c[1], ncoef, q[1], &got[1], NULL);
        const int r2 = jpgx_read_jfif_sub_gray(file, n, 16u, 2u, c[2], ncoef, q[2], &got[2], NULL);
        CHECK(rc == r1 && rc == r2);
        for (int k = 0; k < 3; k++) {
            CHECK(memcmp(&got[k], &info, sizeof info) == 0);
            CHECK(memcmp(q[k], q[0], 64 * sizeof(uint16_t)) == 0);
        }
        if (!rc) {
            CHECK(memcmp(c[0], c[1], ncoef * sizeof(int16_t)) == 0 && memcmp(c[0], c[2], ncoef * sizeof(int16_t)) == 0);
            CHECK(pixels(c[0], W, H, q[0], 1, 1 + (int)(n % 2)) == 0);
            CHECK(pixels(c[0], W, H, q[0], 3, 2 - (int)(n % 2)) == 0);
        }
        for (int k = 0; k < 3; k++) {
            free(c[k]);
            free(q[k]);
        }
    }
    free(file);
    n_cases++;
    n_ok += rc == 0;
    n_header += rc == JPGX_EJFIF_HEADER;
    n_scan += rc == JPGX_EJFIF_SCAN;
    *rc_out = rc;
    return 0;
}

static int one_file(const char *path, long *used)
{
    FILE *fp = fopen(path, "rb");
    CHECK(fp);
    uint8_t f[kMaxFile + 1], g[kMaxFile];
    const size_t len = fread(f, 1, sizeof f, fp);
    fclose(fp);
    if (len > kMaxFile) return 0;
    int rc = 0;
    jpgx_jfif_info info;
    CHECK(jpgx_jfif_info_of_gray(f, len, &info) == 0);
    const int W = info.width, H = info.height;
    CHECK(decode(f, len, W, H, &rc) == 0 && rc == 0);
    for (size_t n = 0; n < len; n++) {
        CHECK(decode(f, n, W, H, &rc) == 0);
        CHECK(rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN);
    }
    for (int how = 0; how < 3; how++)
        for (size_t p = 0; p < len; p++) {
            memcpy(g, f, len);
            g[p] = how == 0 ? 0x00 : how == 1 ? 0xff : (uint8_t)(f[p] ^ 1);
            CHECK(decode(g, len, W, H, &rc) == 0);
            CHECK(rc == 0 || rc == JPGX_EJFIF_HEADER || rc == JPGX_EJFIF_SCAN);
        }
    ++*used;
    return 0;
}

/* the host twins' thread fan-out (csrc/jx_par.h): a 16 x 16 4:4:4 frame, 2 MCU rows, through the
 * writer, the reader and both pixel routines on 1, 0 (one per CPU), 3 (more threads than rows) and 64
 * (the most) threads, every output equal to the one-thread one; then the writer's 200 jobs, more than
 * the runner keeps on its stack, over the 520 one-MCU rows of an 8 x 4160 frame */
static int threads(void)
{
    static const int nt[4] = {1, 0, 3, 64};
    enum { kCoef = 12 * 64, kCap = 8192 };
    int16_t coef[kCoef], back[2][kCoef];
    uint16_t qt[2][2][64];
    uint8_t *file[2], rgb[2][16 * 48], gray[2][16 * 48], flat[2][16 * 48];    /* flat: one thread's, 1 and 3 channels */
    size_t len[2] = {0, 0};
    uint32_t x = 0x6a785f70u;
    for (int i = 0; i < kCoef; i++) {
        x = x * 1103515245u + 12345u;
        coef[i] = (int16_t)((int)(x >> 16 & 63u) - 32);
    }
    for (int k = 0; k < 2; k++) CHECK((file[k] = (uint8_t *)malloc(kCap)) != NULL);
    for (int i = 0; i < 4; i++) {
        const int k = i != 0;                               /* 0: one thread's, 1: this count's */
        CHECK(jpgx_write_jfif_ex(coef, 16, 16, 75, 0, 1, nt[i], file[k], kCap, &len[k]) == 0);
        CHECK(len[k] == len[0] && memcmp(file[k], file[0], len[0]) == 0);
        CHECK(jpgx_read_jfif(file[0], len[0], nt[i], back[k], kCoef, qt[k], NULL) == 0);
        CHECK(memcmp(back[k], coef, sizeof coef) == 0 && memcmp(qt[k], qt[0], sizeof qt[0]) == 0);
        CHECK(jpgx_pixels_host(coef, 16, 16, 0, (const uint16_t (*)[64])qt[0], rgb[k], 48, nt[i]) == 0);
        CHECK(memcmp(rgb[k], rgb[0], sizeof rgb[0]) == 0);
        for (int ch = 1; ch <= 3; ch += 2) {
            memset(gray[k], 0, sizeof gray[k]);
            CHECK(jpgx_pixels_host_gray(coef, 16, 16, qt[0][0], gray[k], (size_t)ch * 16, ch, nt[i]) == 0);
            if (!k) memcpy(flat[ch / 2], gray[0], sizeof gray[0]);
            CHECK(memcmp(gray[k], flat[ch / 2], sizeof gray[0]) == 0);
        }
    }
    int16_t *zero = (int16_t *)calloc((size_t)3 * 520 * 64, sizeof(int16_t));
    CHECK(zero);
    CHECK(jpgx_write_jfif_ex(zero, 8, 4160, 50, 0, 1, 1, file[0], kCap, &len[0]) == 0);
    CHECK(jpgx_write_jfif_ex(zero, 8, 4160, 50, 0, -1, 200, file[1], kCap, &len[1]) == 0);     /* ceil(520 / 800) = 1 row */
    CHECK(len[1] == len[0] && memcmp(file[1], file[0], len[0]) == 0);
    free(zero);
    free(file[0]);
    free(file[1]);
    return 0;
}

int main(void)
{
    if (threads()) return 1;
    /* tests/c/gray_san.c -> tests/golden/gray_fixtures/ */
    char dir[4096];
    const char *self = __FILE__, *cut = strstr(self, "c/gray_san.c");
    CHECK(cut && (size_t)(cut - self) + sizeof "golden/gray_fixtures/" < sizeof dir - 300);
    memcpy(dir, self, (size_t)(cut - self));
    strcpy(dir + (cut - self), "golden/gray_fixtures/");
    DIR *d = opendir(dir);
    CHECK(d);
    long used = 0;
    for (struct dirent *e; (e = readdir(d)) != NULL;) {
        const size_t l = strlen(e->d_name);
        if (l < 4 || l > 200 || strcmp(e->d_name + l - 4, ".jpg") != 0) continue;
        char path[4400];
        snprintf(path, sizeof path, "%s%s", dir, e->d_name);
        if (one_file(path, &used)) return 1;
    }
    closedir(d);
    /* argument checks */
    {
        uint8_t b[4] = {0xff, 0xd8, 0xff, 0xd9}, px[3];
        int16_t c[64] = {0};
        uint16_t qt[64];
        jpgx_jfif_info info;
        for (int k = 0; k < 64; k++) qt[k] = 1;
        CHECK(jpgx_jfif_info_of_gray(NULL, 4, &info) == JPGX_EARG && jpgx_jfif_info_of_gray(b, 4, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_gray(NULL, 4, 1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_gray(b, 4, 1, NULL, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_gray(b, 4, -1, c, 64, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_gray(b, 4, 1, c, 64, NULL, NULL) == JPGX_EJFIF_HEADER);
        CHECK(jpgx_read_jfif_sub_gray(b, 4, 15, 2, c, 64, NULL, NULL, NULL) == JPGX_EARG);
        CHECK(jpgx_read_jfif_sub_gray(b, 4, 0, 0, c, 64, NULL, NULL, NULL) == JPGX_EJFIF_HEADER);
        CHECK(jpgx_pixels_host_gray(c, 1, 1, qt, px, 1, 1, 1) == 0 && jpgx_pixels_host_gray(c, 1, 1, qt, px, 3, 3, 1) == 0);
        CHECK(jpgx_pixels_host_gray(c, 1, 1, qt, px, 2, 3, 1) == JPGX_EARG);
        CHECK(jpgx_pixels_host_gray(c, 1, 1, qt, px, 3, 2, 1) == JPGX_EARG);
        CHECK(jpgx_pixels_host_gray(c, 0, 1, qt, px, 3, 1, 1) == JPGX_EGEOMETRY);
        CHECK(jpgx_pixels_host_gray(c, 1, 65536, qt, px, 3, 1, 1) == JPGX_EGEOMETRY);
    }
    printf("files %ld cases %ld ok %ld header %ld scan %ld pixels %ld\n", used, n_cases, n_ok, n_header, n_scan, n_pixels);
    CHECK(used >= 30 && n_cases >= 50000 && n_ok + n_header + n_scan == n_cases && n_pixels == 2 * n_ok);
    puts("gray_san: clean");
    return 0;
}
