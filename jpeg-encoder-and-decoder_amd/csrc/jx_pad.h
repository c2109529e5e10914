/*
 * jx_pad.h -- k_pad_edge's chunk rule, the text the kernel (csrc/jpgx_pad.hip) and its
 * host restatement (csrc/jpgx_pad_host.cpp, test-only: every load checked against a buffer) run alike.
 * A row pair of the coded frame, 2 x 3 cw bytes, is pitch / 8 chunks of 16 bytes.  For chunk c of pair
 * `pair`:
 *   jx_pad_chunk   the chunk's byte in the pair, the row of the pair its first byte lies in, its place xb
 *                  in that row, and whether its 16 bytes are image bytes of that one row
 *   jx_pad_load    the source row (beyond H - 1: row H - 1), sh = the address of the chunk's first source
 *                  byte modulo 4, the fast / slow decision and, for a fast chunk, its four or five
 *                  aligned dword loads
 *   JX_PAD_FUNNEL  a fast chunk's 16 bytes from its dwords
 *   JX_PAD_BYTES   a slow chunk byte by byte: beyond 3 W the last pixel's channel (jx_pad_byte)
 * Reads never leave [row start, row start + 3 W) of a row 0 .. H - 1.  A chunk is slow when its aligned
 * dwords would (a row's first chunk when the row starts off a dword; a last one whose fifth dword passes
 * the row's end), when it holds repeated columns, and when it straddles the two rows of a pair (3 cw no
 * multiple of 16): all of the last two have xb + 16 > 3 W.
 *   mem.u32(p) / mem.u8(p): an aligned 4-byte load, a byte load.
 */
#ifndef JX_PAD_H
#define JX_PAD_H

#include <stddef.h>
#include <stdint.h>

#include "xform_math.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JX_PAD_ROLLED _Pragma("unroll 1")
#define JX_PAD_UNROLL _Pragma("unroll")
#else
#define JX_PAD_ROLLED
#define JX_PAD_UNROLL
#endif

struct JxPadChunk {
    uint32_t o;                         /* the chunk's byte in the row pair */
    uint32_t r;                         /* the row of the pair that byte lies in */
    uint32_t xb;                        /* its place in row 2 pair + r */
    bool whole;                         /* 16 image bytes of one row */
};

/* chunk c < pitch / 8 of a row pair; pitch = 3 cw, w3 = 3 W */
JX_HD JxPadChunk jx_pad_chunk(uint32_t c, uint32_t pitch, uint32_t w3)
{
    JxPadChunk k;
    k.o = 16u * c;
    k.r = k.o >= pitch ? 1u : 0u;
    k.xb = k.o - k.r * pitch;
    k.whole = k.xb + 16u <= w3;
    return k;
}

/* The loads of chunk k of row pair `pair` of a frame whose row y begins at src + y * in_pitch.  fast:
 * whether the chunk is fast; then d holds the aligned dwords [p - sh, p - sh + 16), and [.., + 20) when
 * sh != 0, all inside the row; a slow chunk loads nothing here. */
template <class Mem>
JX_HD void jx_pad_load(const Mem &mem, const uint8_t *src, size_t in_pitch, uint32_t w3, uint32_t h,
                       const JxPadChunk &k, uint32_t pair, uint32_t (&d)[5], uint32_t &sh, bool &fast)
{
    const uint32_t yy = 2u * pair + k.r, y = yy < h - 1u ? yy : h - 1u;
    const uint8_t *p = src + (size_t)y * in_pitch + k.xb;
    sh = (uint32_t)((uintptr_t)p & 3u);
    fast = k.whole && k.xb >= sh && (sh == 0u || k.xb - sh + 20u <= w3);
    if (fast) {
        const uint8_t *q = p - sh;
        const uint32_t d0 = mem.u32(q), d1 = mem.u32(q + 4), d2 = mem.u32(q + 8), d3 = mem.u32(q + 12);
        const uint32_t d4 = sh ? mem.u32(q + 16) : 0u;
        d[0] = d0;
        d[1] = d1;
        d[2] = d2;
        d[3] = d3;
        d[4] = d4;
    }
}

/* bytes sh .. sh + 3 of the little-endian pair lo, hi (v_alignbyte_b32) */
JX_HD uint32_t jx_pad_align(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (sh & 3u)));
#endif
}

/* a fast chunk's 16 bytes: uint32_t w[4], little-endian, from its dwords d[5].  This and JX_PAD_BYTES are
 * macros and not functions: with the words handed through a reference the compiler kept the kernel's
 * arrays in another form and k_pad_edge's instructions came out different (profiles/
 * pad_rule_isa_identity.txt holds them equal to the kernel's before this header). */
#define JX_PAD_FUNNEL(w, d, sh)                                                        \
    do {                                                                               \
        JX_PAD_UNROLL                                                                  \
        for (int k_ = 0; k_ < 4; k_++) (w)[k_] = jx_pad_align((d)[k_ + 1], (d)[k_], sh); \
    } while (0)

/* byte xb of a coded row whose source row begins at `row`: beyond 3 W the last pixel's channel */
template <class Mem>
JX_HD uint32_t jx_pad_byte(const Mem &mem, const uint8_t *row, uint32_t xb, uint32_t w3)
{
    return mem.u8(row + (xb < w3 ? xb : w3 - 3u + xb % 3u));
}

/* the 16 bytes at byte o of row pair `pair`, one by one, into uint32_t w[4] (zeros before) */
#define JX_PAD_BYTES(w, mem, src, in_pitch, w3, h, pitch, o, pair)                                         \
    do {                                                                                                   \
        JX_PAD_ROLLED                                                                                      \
        for (uint32_t k_ = 0; k_ < 16u; k_++) {                                                            \
            const uint32_t ob_ = (o) + k_;                      /* below 2 pitch: c < pitch / 8 */         \
            const uint32_t rr_ = ob_ >= (pitch) ? 1u : 0u;                                                 \
            const uint32_t yy_ = 2u * (pair) + rr_, y_ = yy_ < (h) - 1u ? yy_ : (h) - 1u;                  \
            const uint32_t b_ = jx_pad_byte(mem, (src) + (size_t)y_ * (in_pitch), ob_ - rr_ * (pitch), w3) \
                                << (8u * (k_ & 3u));                                                       \
            (w)[0] |= k_ < 4u ? b_ : 0u;                                                                   \
            (w)[1] |= k_ >= 4u && k_ < 8u ? b_ : 0u;                                                       \
            (w)[2] |= k_ >= 8u && k_ < 12u ? b_ : 0u;                                                      \
            (w)[3] |= k_ >= 12u ? b_ : 0u;                                                                 \
        }                                                                                                  \
    } while (0)

/* The host's side (csrc/jpgx_pad_host.cpp, test-only): the rule above chunk by chunk over a batch of
 * nframes frames of width x height whose pixel (0, 0) of frame f is buf[base_off + f * in_frame_stride],
 * into out: the coded frames, rows of 3 coded_width bytes, frames coded_height rows apart.
 * touched NULL: plain loads.  touched [len]: every load is checked against [buf, buf + len) and, a dword
 * load, for alignment, and recorded (|= 1 a byte load, |= 2 a dword load, per byte read); a refused load
 * returns what it has of the buffer, zeros beyond.  stats (may be NULL) [JX_PAD_NSTAT], added to:
 *   [0..3]   fast chunks by sh
 *   [4..7]   slow chunks by reason: a row's first chunk off a dword (xb < sh); repeated columns or a
 *            row's short end (xb + 16 > 3 W, one row); the fifth dword past the row; the straddling chunk
 *   [8]      chunks with an index >= 256 (a second workgroup's)
 *   [9..12]  by sh: chunks otherwise fast with xb - sh + 20 == 3 W (the last that is)
 *   [13..16] by sh: with xb - sh + 20 == 3 W + 1 (the first that is not)
 * Returns the refused loads plus the slow chunks that none of the reasons explains (must be 0), -1 for
 * bad arguments. */
#define JX_PAD_NSTAT 17
extern "C" {
long long jx_pad_host(const uint8_t *buf, size_t len, size_t base_off, int width, int height, size_t in_pitch,
                      size_t in_frame_stride, int nframes, int coded_width, int coded_height, uint8_t *out,
                      uint8_t *touched, uint64_t *stats);
}

#endif
