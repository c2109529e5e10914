/* pad_rule_san.c -- TEST INFRASTRUCTURE (tests/test_pad_rule.py): k_pad_edge's chunk rule on the host
 * (csrc/jx_pad.h through csrc/jpgx_pad_host.cpp's jx_pad_host, plain loads, no trace) under
 * -fsanitize=address,undefined, as a program of its own.  The sweep is tests/pad_cases.py's: every width
 * 1 .. 48 and 681 .. 696, heights 1, 2, 7, 8, 9, rows 3 W + 0 .. 3 bytes apart, the three samplings, four
 * frames a stride of 1 (mod 4) apart.  The source is a heap buffer of exactly the bytes up to the last
 * frame's last pixel, the coded frames go into one of exactly their size, and each frame is compared with
 * jpgx_pad_edge's (host/jpgx_pad.c).
 * Exit status 0 and "pad_rule_san: clean" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpgx_compat.h"

long long jx_pad_host(const uint8_t *buf, size_t len, size_t base_off, int width, int height, size_t in_pitch,
                      size_t in_frame_stride, int nframes, int coded_width, int coded_height, uint8_t *out,
                      uint8_t *touched, uint64_t *stats);

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "pad_rule_san: line %d: %s\n", __LINE__, #c);  \
            return 1;                                                      \
        }                                                                  \
    } while (0)

enum { kFrames = 4, kStats = 17 };

static long n_cases;
static uint64_t total[kStats];

static int one_case(int W, int H, int slack, int sr)
{
    const int mw = sr ? 16 : 8, mh = sr == 2 ? 16 : 8;
    const int cw = (W + mw - 1) / mw * mw, ch = (H + mh - 1) / mh * mh;
    const size_t pitch = 3 * (size_t)W + (size_t)slack, extent = pitch * (size_t)(H - 1) + 3 * (size_t)W;
    const size_t fstride = extent + (5 - extent % 4) % 4, n = (kFrames - 1) * fstride + extent;
    const size_t coded = (size_t)ch * (size_t)cw * 3;
    uint8_t *src = (uint8_t *)malloc(n), *out = (uint8_t *)malloc(kFrames * coded), *ref = (uint8_t *)malloc(coded);
    CHECK(src && out && ref && fstride % 4 == 1);
    uint32_t x = 0x70616431u + (uint32_t)(n_cases * 2654435761u);
    for (size_t i = 0; i < n; i++) {
        x = x * 1103515245u + 12345u;
        src[i] = (uint8_t)(x >> 16);
    }
    CHECK(jx_pad_host(src, n, 0, W, H, pitch, fstride, kFrames, cw, ch, out, NULL, total) == 0);
    for (int f = 0; f < kFrames; f++) {
        CHECK(jpgx_pad_edge(src + (size_t)f * fstride, W, H, pitch, cw, ch, ref) == 0);
        CHECK(memcmp(out + (size_t)f * coded, ref, coded) == 0);
    }
    free(ref);
    free(out);
    free(src);
    n_cases++;
    return 0;
}

int main(void)
{
    static const int heights[5] = {1, 2, 7, 8, 9};
    for (int W = 1; W <= 696; W = W == 48 ? 681 : W + 1)
        for (int h = 0; h < 5; h++)
            for (int slack = 0; slack < 4; slack++)
                for (int sr = 0; sr < 3; sr++) CHECK(one_case(W, heights[h], slack, sr) == 0);
    /* argument checks */
    {
        uint8_t b[64] = {0}, o[8 * 8 * 3];
        CHECK(jx_pad_host(b, sizeof b, 0, 3, 5, 9, 45, 1, 8, 8, o, NULL, NULL) == 0);
        CHECK(jx_pad_host(NULL, sizeof b, 0, 3, 5, 9, 45, 1, 8, 8, o, NULL, NULL) == -1);
        CHECK(jx_pad_host(b, sizeof b, 0, 3, 5, 9, 45, 1, 8, 8, NULL, NULL, NULL) == -1);
        CHECK(jx_pad_host(b, sizeof b, 0, 3, 5, 8, 45, 1, 8, 8, o, NULL, NULL) == -1);
        CHECK(jx_pad_host(b, sizeof b, 0, 3, 5, 9, 45, 0, 8, 8, o, NULL, NULL) == -1);
        CHECK(jx_pad_host(b, sizeof b, 0, 9, 5, 27, 135, 1, 8, 8, o, NULL, NULL) == -1);
    }
    uint64_t fast = 0, slow = 0;
    for (int k = 0; k < 4; k++) {
        CHECK(total[k] > 0 && total[4 + k] > 0);
        fast += total[k];
        slow += total[4 + k];
    }
    CHECK(total[8] > 0);
    printf("cases %ld fast %llu slow %llu high %llu\n", n_cases, (unsigned long long)fast, (unsigned long long)slow,
           (unsigned long long)total[8]);
    puts("pad_rule_san: clean");
    return 0;
}
