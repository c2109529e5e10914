/*
 * jx_jfif_sub.h -- decoding inside a restart interval: the routines of the
 * self-synchronising decoder, one source for the device kernel k_jd_sub (csrc/jpgx_jfif_dec.hip)
 * and its host twin jpgx_read_jfif_sub (csrc/jpgx_jfif_read.cpp), beside jx_jfif_dec.h, whose
 * tables and frame they use.
 *
 * An interval's bytes [begin, end) are cut into subsequences of S bytes, counted from begin, and
 * into tiles of T subsequences.  Every position here is relative to the tile's first byte.  A lane
 * decodes one subsequence: the units (a Huffman code and the magnitude bits its symbol calls for)
 * whose first bit lies in it.  A lane that does not know where a unit begins guesses; the lanes'
 * exit states are handed on until they agree with the sequential decoder's (jxs_decode_sub's
 * callers do that, each in its own way: barriers there, loops here).
 *
 * The bytes are untrusted.  The rules of jx_jfif_dec.h hold:
 *   - a byte is read only through the reader, at a position below `lim`, which the caller has
 *     bounded by the interval's end and by what it has loaded (the tile and JXS_HALO bytes);
 *   - a coefficient is written only into a block whose index jxs_block_of has checked against the
 *     frame's and the interval's block counts, at an index 0 .. 63;
 *   - every loop is bounded by the bytes left below `lim`, by the 16 code lengths or by index 63
 *     (the rounds of the callers by T);
 *   - anything else makes the state invalid.
 */
#ifndef JX_JFIF_SUB_H
#define JX_JFIF_SUB_H

#include "jx_jfif_dec.h"

#if defined(__HIPCC__)
#define JXD_FN_M __host__ __device__ inline
#else
#define JXD_FN_M inline
#endif

/* the kernel's shape: bytes per subsequence (a multiple of 16), subsequences per tile (its lanes) */
#ifndef JXS_SUB
#define JXS_SUB 32u
#endif
#define JXS_TILE 256u
/* bytes loaded past a tile for the unit that overruns its last subsequence: such a unit begins at
 * the tile's last byte at the latest and takes at most 7 + 27 bits, five data bytes, each of which
 * may drag a stuffed 00 along.  The window below reads eight */
#define JXS_HALO 16u
#define JXS_INVALID 0xffffffffu

/* where the next unit begins: p = 8 x the data byte that holds its first bit + the bit's index from
 * the top (never a stuffed 00: after the last bit of an FF the position moves on by two bytes),
 * cz = c << 8 | z, the block's place in its MCU and the zig-zag index the unit starts at (0: DC).
 * p == JXS_INVALID: no such place */
struct jxs_state {
    uint32_t p, cz;
};

JXD_FN bool jxs_same(jxs_state a, jxs_state b) { return a.p == b.p && a.cz == b.cz; }

/* the six tables of a frame's three components, and its MCU */
struct jxs_tabs {
    const jxd_tab *dc[3], *ac[3];
    uint32_t lum, bpm;      /* Y blocks per MCU, blocks per MCU */
};

JXD_FN void jxs_tabs_of(const jxd_frame *fr, const jxd_tab *tabs, jxs_tabs *t)
{
    for (int c = 0; c < 3; c++) {
        t->dc[c] = tabs + fr->tdc[c];
        t->ac[c] = tabs + fr->tac[c];
    }
    t->lum = fr->hs * fr->vs;
    t->bpm = t->lum + 2u;
}

/* the one-component frame (jxd_parse_header's GRAY): the MCU is one block, and the unit walk below
 * stays at c = 0.  The header walk has put the component's tables into all three places */
JXD_FN void jxs_tabs_of_gray(const jxd_frame *fr, const jxd_tab *tabs, jxs_tabs *t)
{
    jxs_tabs_of(fr, tabs, t);
    t->lum = t->bpm = 1u;
}

/* the reader of a plain buffer: byte r of the tile that begins at d */
struct jxs_flat {
    const uint8_t *d;
    JXD_FN_M uint32_t byte(uint32_t r) const { return d[r]; }
};

/* up to eight data bytes from byte `pos` on, stuffing removed, left-aligned in w: bit `bit` of the
 * first of them is the next bit */
struct jxs_win {
    uint64_t w;
    uint32_t k;             /* data bytes in w */
    uint32_t pos, bit;
    uint32_t next;          /* the next byte to load; JXS_INVALID after an FF without its 00 */
};

template <class R>
JXD_FN void jxs_fill(jxs_win *b, const R &rd, uint32_t lim)
{
    while (b->k < 8u && b->next < lim) {
        const uint32_t x = rd.byte(b->next);
        if (x == 0xffu) {
            if (b->next + 1u < lim && rd.byte(b->next + 1u) == 0u) {
                b->next += 2u;
            } else {                    /* a marker, the interval's end or the halo's: nothing more */
                b->next = JXS_INVALID;
                return;
            }
        } else {
            b->next++;
        }
        b->w |= (uint64_t)x << (56u - 8u * b->k);
        b->k++;
    }
}

/* n bits (1 .. 27, all in w) are used: pos / bit move on; returns the byte that held the last */
JXD_FN uint32_t jxs_consume(jxs_win *b, uint32_t n)
{
    uint32_t tot = b->bit + n, last = b->pos;
    while (tot >= 8u) {                 /* at most four bytes */
        tot -= 8u;
        b->pos += (uint32_t)(b->w >> 56) == 0xffu ? 2u : 1u;
        b->w <<= 8;
        b->k--;
        if (tot) last = b->pos;
    }
    b->bit = tot;
    return last;
}

/* what a decode does with its coefficients: nothing (a guess, a round) ... */
struct jxs_nowrite {
    JXD_FN_M void put(uint32_t, int) {}
    JXD_FN_M bool next_block() { return true; }
    JXD_FN_M void unit(uint32_t, uint32_t) {}
};

/* block `ord` (in decode order) of the interval that begins at MCU mcu0 and has nblocks blocks: its
 * index in the frame's coefficient array, JXS_INVALID outside the interval or the frame */
JXD_FN uint32_t jxs_block_of(const jxd_frame *fr, uint32_t mcu0, uint32_t nblocks, uint32_t ord)
{
    const uint32_t lum = fr->hs * fr->vs, bpm = lum + 2u;
    if (ord >= nblocks) return JXS_INVALID;
    const uint32_t m = ord / bpm, j = ord - m * bpm, mcu = mcu0 + m;
    if (mcu >= fr->nmcu) return JXS_INVALID;
    const uint32_t my = mcu / fr->cpr, mx = mcu - my * fr->cpr;
    if (j < lum) {
        const uint32_t dy = j / fr->hs, dx = j - dy * fr->hs;
        const uint32_t blk = (my * fr->vs + dy) * fr->bpr + mx * fr->hs + dx;
        return blk < fr->nb ? blk : JXS_INVALID;
    }
    const uint32_t cb = my * fr->cpr + mx;
    return cb < fr->nbc ? fr->nb + (j - lum) * fr->nbc + cb : JXS_INVALID;
}

/* the same of the one-component frame: block `ord` of the interval is block mcu0 + ord of the frame */
JXD_FN uint32_t jxs_block_of_gray(const jxd_frame *fr, uint32_t mcu0, uint32_t nblocks, uint32_t ord)
{
    if (ord >= nblocks || mcu0 >= fr->nmcu || ord >= fr->nmcu - mcu0) return JXS_INVALID;
    const uint32_t blk = mcu0 + ord;
    return blk < fr->nb ? blk : JXS_INVALID;
}

template <int GRAY>
JXD_FN uint32_t jxs_block_of_t(const jxd_frame *fr, uint32_t mcu0, uint32_t nblocks, uint32_t ord)
{
    return GRAY ? jxs_block_of_gray(fr, mcu0, nblocks, ord) : jxs_block_of(fr, mcu0, nblocks, ord);
}

/* ... or the last pass: the nonzero coefficients and the DC difference into the frame, from block
 * `ord` of the interval on, up to its last block.  GRAY: of the one-component frame */
template <int GRAY>
struct jxs_store_t {
    const jxd_frame *fr;
    int16_t *coef;          /* the frame's */
    uint32_t mcu0, nblocks, ord;
    int16_t *cur;           /* block ord, NULL: none */
    JXD_FN_M void open(const jxd_frame *f, int16_t *c, uint32_t m0, uint32_t nb, uint32_t o)
    {
        fr = f, coef = c, mcu0 = m0, nblocks = nb, ord = o;
        seek();
    }
    JXD_FN_M void seek()
    {
        const uint32_t blk = jxs_block_of_t<GRAY>(fr, mcu0, nblocks, ord);
        cur = blk == JXS_INVALID ? NULL : coef + (size_t)blk * 64;
    }
    JXD_FN_M void put(uint32_t k, int v)
    {
        if (cur && k < 64u) cur[k] = (int16_t)v;
    }
    JXD_FN_M bool next_block()
    {
        ord++;
        seek();
        return cur != NULL;
    }
    JXD_FN_M void unit(uint32_t, uint32_t) {}
};
typedef jxs_store_t<0> jxs_store;

JXD_FN int jxs_extend(uint32_t v, uint32_t s) { return v < (1u << (s - 1u)) ? (int)v - (1 << s) + 1 : (int)v; }

/* The units that begin at `in` and in the bytes below sub_end, one after another (T.81 F.2.2.1,
 * F.2.2.2 as jxd_block reads them).  *out: where the first unit begins that does not -- or, when
 * wr says that the interval's last block is complete, where that block ended -- or invalid: a code
 * in no table, an index past 63, a DC size above 11, an AC size above 10, a size-0 symbol with a
 * run other than 0 or 15, or bits that ran out.  *nblk: the blocks completed. */
template <class R, class W>
JXD_FN void jxs_decode_sub(const R &rd, uint32_t lim, uint32_t sub_end, jxs_state in, const jxs_tabs *t, W &wr,
                           jxs_state *out, uint32_t *nblk)
{
    *nblk = 0;
    *out = in;
    if (in.p == JXS_INVALID) return;
    uint32_t c = in.cz >> 8, z = in.cz & 63u;
    jxs_win b;
    b.w = 0;
    b.k = 0;
    b.pos = b.next = in.p >> 3;
    b.bit = in.p & 7u;
    out->p = JXS_INVALID;
    out->cz = 0;
    while (b.pos < sub_end && b.pos < lim) {
        if (8u * b.k < b.bit + 32u) jxs_fill(&b, rd, lim);
        const uint32_t avail = 8u * b.k - b.bit;
        const uint32_t x = (uint32_t)((b.w << b.bit) >> 32);
        const uint32_t comp = c < t->lum ? 0u : c - t->lum + 1u;
        const jxd_tab *tab = z ? (comp == 0 ? t->ac[0] : comp == 1 ? t->ac[1] : t->ac[2])
                               : (comp == 0 ? t->dc[0] : comp == 1 ? t->dc[1] : t->dc[2]);
        const uint32_t peek = x >> 16, e = tab->look[peek >> 8];
        uint32_t l = e >> 8, v = e & 255u;
        if (!e) {
            for (l = 9; l <= 16; l++) {
                const int32_t code = (int32_t)(peek >> (16 - l));
                if (code <= tab->maxcode[l]) {
                    v = tab->vals[(uint32_t)(code + tab->valoff[l]) & 255u];
                    break;
                }
            }
            if (l > 16) return;
        }
        uint32_t n = l, end_of_block = 0;
        if (!z) {
            if (v > 11u || l + v > avail) return;
            n += v;
            if (v) wr.put(0, jxs_extend((x << l) >> (32u - v), v));
            z = 1;
        } else {
            const uint32_t r = v >> 4, sz = v & 15u;
            if (!sz) {
                if (l > avail) return;
                if (r == 0u) {
                    end_of_block = 1;
                } else {
                    if (r != 15u) return;
                    z += 16u;
                    if (z > 64u) return;
                }
            } else {
                z += r;
                if (z > 63u || sz > 10u || l + sz > avail) return;
                n += sz;
                wr.put(z, jxs_extend((x << l) >> (32u - sz), sz));
                z++;
            }
        }
        const uint32_t first = b.pos, last = jxs_consume(&b, n);
        wr.unit(first, last);
        if (end_of_block || z == 64u) {
            z = 0;
            c = c + 1u == t->bpm ? 0u : c + 1u;
            ++*nblk;
            if (!wr.next_block()) break;
        }
    }
    out->p = b.pos * 8u + b.bit;
    out->cz = c << 8 | z;
}

/* where lane i > 0 of a tile starts when nobody has told it: its subsequence's first byte with
 * c = 0, z = 0; one byte later where that byte is a stuffed 00 (the byte before it is in the tile) */
template <class R>
JXD_FN jxs_state jxs_guess(const R &rd, uint32_t i, uint32_t sub_bytes, uint32_t *on_stuffing)
{
    const uint32_t r = i * sub_bytes;
    const uint32_t skip = rd.byte(r) == 0u && rd.byte(r - 1u) == 0xffu;
    if (on_stuffing) *on_stuffing = skip;
    jxs_state s = {(r + skip) * 8u, 0u};
    return s;
}

/* an FF in the bytes [r0, r1) of the tile that its 00 does not follow inside the interval, which
 * ends at end_rel (seen from the tile; above `lim` it only has to be large) */
template <class R>
JXD_FN uint32_t jxs_bare_ff(const R &rd, uint32_t r0, uint32_t r1, uint32_t end_rel)
{
    uint32_t bad = 0;
    for (uint32_t r = r0; r < r1; r++)
        if (rd.byte(r) == 0xffu && !(r + 1u < end_rel && rd.byte(r + 1u) == 0u)) bad = 1;
    return bad;
}

/* after the interval's last unit, at p: fewer than 8 unstuffed bits and no data byte are left */
template <class R>
JXD_FN bool jxs_tail_ok(const R &rd, uint32_t lim, uint32_t end_rel, uint32_t p)
{
    const uint32_t pos = p >> 3;
    if (!(p & 7u)) return pos == end_rel;
    if (pos >= end_rel || pos >= lim) return false;
    return pos + (rd.byte(pos) == 0xffu ? 2u : 1u) == end_rel;
}

/* a tile: its bytes, the bytes loaded for it, and its end as the routines above take it */
struct jxs_tile {
    uint32_t n, lim, end_rel;
};

JXD_FN jxs_tile jxs_tile_of(uint64_t left /* end - the tile's first byte */, uint32_t sub_bytes, uint32_t tile_subs)
{
    const uint32_t full = sub_bytes * tile_subs;
    jxs_tile t;
    t.n = left < full ? (uint32_t)left : full;
    t.lim = left < full + JXS_HALO ? (uint32_t)left : full + JXS_HALO;
    t.end_rel = left <= t.lim ? (uint32_t)left : t.lim + 1u;
    return t;
}

#endif
