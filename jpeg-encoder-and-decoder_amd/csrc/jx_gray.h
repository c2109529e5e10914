/*
 * jx_gray.h -- the forward path for one-channel images, the parts the kernel
 * k_gray (csrc/jpgx_gray.hip) and its host restatement (csrc/jpgx_gray_host.cpp, test-only: the band's
 * self-test, the load trace, jx_gray_host_blocks) run from one source text:
 *   jx_gray_load_block   which bytes a block's 8 x 8 samples are read from, and how
 *   jx_gray_rows / _col  the fp32 fast path: sample = byte - 128 (exact), jx_fdct8<FOps> on rows and
 *                        columns, the magic-number quantiser
 *   jx_gray_exact        one coefficient in the oracle's exact fp64 operation order
 * The contract is this project's own (the reference knows only RGB; parity unpinned): the frame is
 * jx_frame_make_gray's, ceil(W / 8) x ceil(H / 8) blocks in raster order, standard tiling, the pixels
 * beyond the image by the edge rule (last column to the right, last row downwards).
 */
#ifndef JX_GRAY_H
#define JX_GRAY_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "jx_consts.h"
#include "xform_math.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JX_UNROLL _Pragma("unroll")
#else
#define JX_UNROLL
#endif

/*
 * The 8 rows of block (bx, by) of a w x h frame whose row r begins at frame + r * pitch, as two
 * little-endian dwords per row (byte x of the row in bits 8 (x & 3) of dword x >> 2).
 * Nothing is read outside bytes [0, w) of rows 0 .. h - 1, for any pitch and any alignment of frame:
 * rows >= h read row h - 1, columns >= w take byte w - 1.  Row by row, for a block whose 8 columns are
 * inside the image:
 *   the row's 8 bytes begin on a multiple of 8: one aligned 8-byte load; on a multiple of 4: two aligned
 *   4-byte loads;
 *   they begin s = 1 .. 3 bytes past a dword: the three aligned dwords that cover them, funnelled (shifted
 *   right by s bytes), provided those 12 bytes lie inside the row -- the block is not the row's first
 *   (the s bytes in front belong to the block before) and at least 4 - s more bytes of the row follow;
 * every other row is read byte by byte: in the last block column of a width that is no multiple of 8,
 * and, of a row that starts off a dword, in its first block and in a last block with fewer than 4 - s
 * bytes of the row behind it.
 *   mem.u64(p) / mem.u32(p) / mem.u8(p): an aligned 8-byte / 4-byte load, a byte load.
 */
template <class Mem>
JX_HD void jx_gray_load_block(const Mem &mem, const uint8_t *frame, long long pitch, uint32_t w, uint32_t h,
                              uint32_t bx, uint32_t by, uint32_t (&raw)[8][2])
{
    const uint32_t x0 = 8u * bx;
    const bool inside = x0 + 8u <= w;
JX_UNROLL
    for (int y = 0; y < 8; y++) {
        const uint32_t r = 8u * by + (uint32_t)y, ry = r < h ? r : h - 1u;
        const uint8_t *row = frame + (long long)ry * pitch, *p = row + x0;
        const uint32_t s = (uint32_t)((uintptr_t)p & 3u);
        if (inside && s == 0u) {
            if (((uintptr_t)p & 7u) == 0u) {
                const uint64_t v = mem.u64(p);
                raw[y][0] = (uint32_t)v;
                raw[y][1] = (uint32_t)(v >> 32);
            } else {
                raw[y][0] = mem.u32(p);
                raw[y][1] = mem.u32(p + 4);
            }
        } else if (inside && bx > 0u && x0 + 12u - s <= w) {
            const uint32_t d0 = mem.u32(p - s), d1 = mem.u32(p - s + 4), d2 = mem.u32(p - s + 8);
            const uint32_t sh = 8u * s;                        /* 8, 16 or 24 */
            raw[y][0] = d0 >> sh | d1 << (32u - sh);
            raw[y][1] = d1 >> sh | d2 << (32u - sh);
        } else {
            uint32_t d[2] = {0u, 0u};
JX_UNROLL
            for (int x = 0; x < 8; x++) {
                const uint32_t c = x0 + (uint32_t)x, cx = c < w ? c : w - 1u;
                d[x >> 2] |= (uint32_t)mem.u8(row + cx) << (8 * (x & 3));
            }
            raw[y][0] = d[0];
            raw[y][1] = d[1];
        }
    }
}

/* sample (x, y) of a loaded block, 0 .. 255 */
JX_HD int jx_gray_byte(const uint32_t (&raw)[8][2], int x, int y)
{
    return (int)((raw[y][x >> 2] >> (8 * (x & 3))) & 0xffu);
}

#define JX_GRAY_MAGIC 12582912.0f       /* 1.5 * 2^23: x + magic rounds x to an integer */

/* row pass: T[y] = jx_fdct8 of the row's samples byte - 128 (exact in fp32) */
JX_HD void jx_gray_rows(const uint32_t (&raw)[8][2], float (&T)[8][8])
{
JX_UNROLL
    for (int y = 0; y < 8; y++) {
        float px[8];
JX_UNROLL
        for (int x = 0; x < 8; x++) px[x] = (float)jx_gray_byte(raw, x, y) - 128.0f;
        jx_fdct8<FOps>(px, T[y]);
    }
}

/* column u: coefficient (row v, column u) quantised with the scale wu[v]: tm[v] = rint(F w) + magic (its
 * low 16 bits are the int16) and d[v] = F w - rint(F w), exact; the guard band tests |d| */
JX_HD void jx_gray_col(const float (&T)[8][8], int u, const float *wu, float (&tm)[8], float (&d)[8])
{
    float col[8], F[8];
JX_UNROLL
    for (int y = 0; y < 8; y++) col[y] = T[y][u];
    jx_fdct8<FOps>(col, F);
JX_UNROLL
    for (int v = 0; v < 8; v++) {
        tm[v] = __builtin_fmaf(F[v], wu[v], JX_GRAY_MAGIC);
        const float rr = tm[v] - JX_GRAY_MAGIC;            /* exact */
        d[v] = __builtin_fmaf(F[v], wu[v], -rr);
    }
}

/* The exact value of coefficient (row v, column u): the oracle's operations in its order -- the sample
 * (double)g - 128, the 64-term sum x outer / y inner of (X c_u[x]) c_v[y] with the tabulated cosine
 * doubles, ((0.25 a_u) a_v) s, a true double division by the transposed table entry q = Qs[u][v], C
 * round().  px(x, y): the block's sample 0 .. 255; cosT: JX_COS_INIT's table. */
template <class Px>
JX_HD int16_t jx_gray_exact(const Px &px, int u, int v, int q, const double (*cosT)[8])
{
    double s = 0.0;
JX_UNROLL
    for (int x = 0; x < 8; x++) {
        const double cu = cosT[u][x];
JX_UNROLL
        for (int y = 0; y < 8; y++) s += ((double)(px(x, y) - 128) * cu) * cosT[v][y];
    }
    const double F = 0.25 * (u == 0 ? (double)JX_ALPHA0 : 1.0) * (v == 0 ? (double)JX_ALPHA0 : 1.0) * s;
    return (int16_t)(int)round(F / (double)q);
}

/* The host's side (csrc/jpgx_plan.cpp: the tables; csrc/jpgx_gray_host.cpp: the rest).  Declared here
 * and not in jpgx_internal.h, whose text is part of the transform kernels' source hash
 * (tools/pmc_summary.py).
 * jx_plan_tables_gray: k_gray's per-quality tables -- fp32 scale and band limit [v * 8 + u], divisors
 * [u * 8 + v]: the luminance ones, the band from the sample bound [-128, 127].
 * The kernel's restatement on the host, for the tests: the band's self-test over generated or given
 * blocks (returns the unflagged coefficients that differ from the exact value: must be 0), the whole
 * transform of an image, and the load rule with every load checked against a buffer. */
extern "C" {
int jx_plan_tables_gray(int quality, float w[64], float lim[64], int16_t q[64]);
long long jx_selftest_gray(long long nblocks, unsigned long long seed, int quality, long long *flagged);
long long jx_selftest_gray_blocks(const uint8_t *px, long long nblocks, int quality, long long *flagged,
                                  uint64_t *flagmask);
int jx_gray_host_blocks(const uint8_t *img, int width, int height, size_t pitch, int quality, int force,
                        int16_t *out);
long long jx_gray_load_trace(const uint8_t *buf, size_t buflen, size_t base_off, int width, int height,
                             size_t pitch, uint8_t *touched, uint8_t *blocks);
}

#endif
