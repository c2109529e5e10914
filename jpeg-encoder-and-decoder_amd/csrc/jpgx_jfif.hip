/*
 * jpgx_jfif.hip -- the JFIF writer's scan on the device: the bytes of
 * jpgx_write_jfif_ex (csrc/jpgx_jfif_write.cpp) with restart intervals, for a batch of frames whose
 * coefficients are in device memory.  A block's symbols, the clamps, the scan's geometry and its
 * block order are jx_jfif_enc.h's, the routines the host writer runs; the kernels bring their own
 * sinks for the symbols (BitCount, BitPack, SymCount).
 *
 * A restart interval is self-contained (DC predictors reset, byte aligned), so one workgroup
 * codes one interval, its lanes looping over the interval's blocks in scan order (MCU by MCU:
 * hs x vs luma blocks, Cb, Cr).  Five launches per batch:
 *   k_jf_len    per block the coded bit count (the DC predecessor is the previous block of the
 *               same component in scan order -- a lookup, not a recurrence), a workgroup
 *               exclusive scan -> each block's bit offset within its interval, the interval's bits
 *   k_jf_place  per frame: the intervals' 16-byte-aligned places in the unstuffed stream
 *   k_jf_pack   zeroes the interval's place, then every lane writes its block's codes at its
 *               bit offset (interior words: stores; the partial first and last words, shared
 *               with the neighbouring lanes' blocks, are merged in LDS), the last block also the
 *               1-bit padding; then counts the interval's 0xFF bytes
 *   k_jf_frame  per frame: the intervals' places in the file (uint64 scan of stuffed sizes and
 *               RSTm markers), the frame's length or its overflow report, headers and EOI
 *   k_jf_stuff  per interval: unstuffed bytes -> file bytes with 0xFF 0x00 stuffing, RSTm
 * A lane keeps its block in LDS (its own 33-dword row: conflict-free when the lanes of a wave read
 * the same coefficient) and walks only the nonzero coefficients (a 64-bit mask, ctz: jxe_walk).
 * The code tables and the header bytes come from the host writer's own functions
 * (jx_jfif_codes, jx_jfif_header) as by-value kernel arguments: nothing is copied with a memcpy,
 * the call is asynchronous, capturable and keeps no state.
 *
 * With JPGX_JFIF_OPTIMIZE (jpgx_jfif_gpu_ex; the bytes of jpgx_write_jfif_opt) every frame gets
 * Huffman tables of its own, and three launches come first:
 *   k_jf_zero   the frame's symbol counts to zero
 *   k_jf_count  k_jf_len's walk with a sink that counts the symbols instead of their bits
 *   k_jf_tables per table: T.81 Annex K.2 exactly as jx_jfif_optimal (host/jpgx_jfif.c) -> the
 *               frame's code tables, DHT segments and their lengths in the workspace
 * k_jf_len, k_jf_pack and k_jf_frame are templates over where tables and header come from: the
 * launch's by-value arguments (the standard path, the same code as before) or the frame's workspace.
 *
 * One-component (grayscale) files (jpgx_jfif_gpu_gray) are the same kernels over the
 * one-component frame (jx_frame_make_gray_coded: an MCU is a block), with the one-component header
 * (jx_jfif_header_gray) and, optimised, two tables per frame: k_jf_tables on a grid of 2 and
 * k_jf_frame<JfHdrOptGray>, the one instantiation that is new.
 */
#include <stdint.h>
#include <string.h>

#include "jpgx_internal.h"
#include "jx_hip.h"
#include "jx_jfif_enc.h"
#include "jx_jfif_gray.h"

namespace {

constexpr int kT = 256;                 /* threads per workgroup (4 waves) */
constexpr int kRow = 33;                /* LDS dwords per lane's block (32 + 1: bank = lane + k / 2) */

struct JfTabs {                         /* code << 8 | length */
    uint32_t dc[2][16];                 /* [luma, chroma][category] */
    uint32_t ac[2][256];                /* [luma, chroma][run << 4 | category] */
};

constexpr int kDhtSlot = 192;           /* bytes kept per DHT segment (at most 21 + 162) */
constexpr int kHdrPre = 320;            /* SOI .. SOF: at most 2 + 18 + 2 x 133 + 19 bytes */
constexpr int kHdrSuf = 32;             /* DRI, SOS: 6 + 14 bytes */

struct JfArgs {
    const int16_t *coef;                /* frame f: Y [nb][64] | Cb [nbc][64] | Cr [nbc][64] at f fstride */
    unsigned long long fstride;         /* int16 elements */
    jx_frame g;
    uint32_t rpi, ni;                   /* MCU rows per interval, intervals per frame */
    uint32_t ivblk;                     /* blocks of a full interval */
    uint32_t hdrlen;
    uint32_t *offs;                     /* [nframes][g.nblk] bit offset within the interval (scan order) */
    uint32_t *ibits;                    /* [nframes][ni] coded bits of the interval */
    uint32_t *nff;                      /* [nframes][ni] 0xFF bytes of the interval (padding included) */
    unsigned long long *ustart;         /* [nframes][ni] place in the frame's unstuffed stream */
    unsigned long long *ostart;         /* [nframes][ni] place in the frame's file */
    uint32_t *ovf;                      /* [nframes] the frame does not fit */
    uint8_t *ustream;                   /* [nframes][uarea] */
    unsigned long long uarea;
    uint8_t *out;
    unsigned long long ostride, ocap;
    unsigned long long *len;
};

struct JfHdr {
    uint8_t b[JX_JFIF_HDR_MAX];
    __device__ __forceinline__ uint32_t length(const JfArgs &a, uint32_t) const { return a.hdrlen; }
    __device__ __forceinline__ uint8_t byte(uint32_t, uint32_t i) const { return b[i]; }
};

/* optimised mode: the frame's own DHT segments between the bytes that do not depend on them */
struct JfHdrOpt {
    uint8_t pre[kHdrPre], suf[kHdrSuf];
    uint32_t npre, nsuf;
    const uint8_t *dht;                 /* [nframes][4][kDhtSlot] */
    const uint32_t *dhtlen;             /* [nframes][4] */
    __device__ __forceinline__ uint32_t length(const JfArgs &, uint32_t f) const
    {
        const uint32_t *n = dhtlen + 4 * (size_t)f;
        return npre + n[0] + n[1] + n[2] + n[3] + nsuf;
    }
    __device__ __forceinline__ uint8_t byte(uint32_t f, uint32_t i) const
    {
        if (i < npre) return pre[i];
        i -= npre;
        const uint32_t *n = dhtlen + 4 * (size_t)f;
        for (uint32_t k = 0; k < 4; k++) {
            if (i < n[k]) return dht[((size_t)f * 4 + k) * kDhtSlot + i];
            i -= n[k];
        }
        return suf[i];
    }
};

/* the same for a one-component file (jpgx_jfif_gpu_gray): two DHT segments, DC and AC luminance, in
 * slots 0 and 1 of the frame's four; k_jf_frame's one new instantiation, every other kernel's text is
 * the colour coder's */
struct JfHdrOptGray {
    uint8_t pre[kHdrPre], suf[kHdrSuf];
    uint32_t npre, nsuf;
    const uint8_t *dht;                 /* [nframes][4][kDhtSlot] */
    const uint32_t *dhtlen;             /* [nframes][4] */
    __device__ __forceinline__ uint32_t length(const JfArgs &, uint32_t f) const
    {
        const uint32_t *n = dhtlen + 4 * (size_t)f;
        return npre + n[0] + n[1] + nsuf;
    }
    __device__ __forceinline__ uint8_t byte(uint32_t f, uint32_t i) const
    {
        if (i < npre) return pre[i];
        i -= npre;
        const uint32_t *n = dhtlen + 4 * (size_t)f;
        for (uint32_t k = 0; k < 2; k++) {
            if (i < n[k]) return dht[((size_t)f * 4 + k) * kDhtSlot + i];
            i -= n[k];
        }
        return suf[i];
    }
};

/* the interval's block count */
__device__ __forceinline__ uint32_t jf_nblk(const JfArgs &a, uint32_t iv)
{
    const uint32_t r0 = iv * a.rpi;
    const uint32_t rows = min(a.rpi, a.g.cbh - r0);
    return rows * a.g.cbw * a.g.bpm;
}

typedef uint32_t jf_u4 __attribute__((ext_vector_type(4)));

/* scan-order block i of interval iv of frame f into this lane's LDS row; returns the mask of its
 * nonzero coefficients, the DC difference (jxe_dc_diff) and whether it is a chroma block */
__device__ __forceinline__ uint64_t jf_load(const JfArgs &a, uint32_t f, uint32_t iv, uint32_t i, uint32_t *row,
                                            int &diff, uint32_t &chroma)
{
    const jx_frame &g = a.g;
    const uint32_t m = i / g.bpm, j = i - m * g.bpm;
    const int16_t *base = a.coef + (size_t)f * a.fstride;
    /* position jj of the interval's MCU mm in the frame's coefficient array */
    const auto at = [&](uint32_t mm, uint32_t jj) {
        const uint32_t mr = mm / g.cbw;
        return jx_frame_block(&g, iv * a.rpi + mr, mm - mr * g.cbw, jj) * 64;
    };
    const int16_t *z = base + at(m, j);
    /* the previous block of the same component: the luma block before it in the MCU, else the
     * previous MCU's last luma block / same chroma block; none at the interval's first MCU */
    int pred = 0;
    if (j > 0 && j < g.lum) pred = base[at(m, j - 1)];
    else if (m > 0) pred = base[at(m - 1, j == 0 ? g.lum - 1 : j)];
    uint64_t nz = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        /* plain loads: a lane's eight loads share one 128-byte line, which must stay in L1 between
         * them (nontemporal loads: 427 instead of 335 us per 8 x 4K batch) */
        const jf_u4 x = ((const jf_u4 *)z)[r];
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            row[4 * r + e] = w[e];
            const uint64_t two = ((w[e] & 0xffffu) ? 1u : 0u) | ((w[e] >> 16) ? 2u : 0u);
            nz |= two << (8 * r + 2 * e);
        }
    }
    diff = jxe_dc_diff((int)(int16_t)(row[0] & 0xffffu), pred);
    chroma = j >= g.lum ? 1u : 0u;
    return nz & ~1ull;
}

/* jxe_walk's view of a lane's block: its LDS row of packed pairs */
struct JfRow {
    const uint32_t *row;
    __device__ __forceinline__ uint32_t fetch(uint32_t k) const { return row[k >> 1]; }
    __device__ __forceinline__ int value(uint32_t word, uint32_t k) const
    {
        return (k & 1u) ? (int)word >> 16 : (int)(int16_t)(word & 0xffffu);
    }
};

/* jxe_walk's sinks on the device hold the block's two code tables in LDS (code << 8 | length) */

/* counts bits */
struct BitCount {
    const uint32_t *dct, *act;
    uint32_t n;
    __device__ __forceinline__ void dc(uint32_t s, uint32_t) { n += (dct[s] & 0xffu) + s; }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t s, uint32_t) { n += (act[sym] & 0xffu) + s; }
};

/* writes bits MSB first from a bit offset.  The words a block covers whole are its own (plain
 * stores).  The word it starts in and the word it ends in may be shared with the neighbouring
 * blocks, whose lanes are the neighbouring lanes: those partial words are ORed into the
 * workgroup's LDS slots (one per distinct word a lane of this pass starts in, k_jf_pack) and
 * leave as one store each -- a global atomic per partial word costs more than the whole walk
 * (eight and more blocks share a word).  Only the last lane's last word
 * has no slot: it is shared with the next pass and goes to memory with an atomicOr. */
struct BitPack {
    const uint32_t *dct, *act;
    uint32_t *wp;
    uint32_t *slots;                    /* the workgroup's LDS slots */
    uint32_t head, tail;                /* slots of the first and the last word; tail ~0: none */
    uint64_t acc;                       /* the low nacc bits are pending */
    uint32_t nacc;
    bool first;
    __device__ __forceinline__ void open(uint8_t *area, uint32_t bit, uint32_t *lds_slots, uint32_t head_slot,
                                         uint32_t tail_slot)
    {
        wp = (uint32_t *)area + (bit >> 5);
        slots = lds_slots;
        head = head_slot;
        tail = tail_slot;
        acc = 0;
        nacc = bit & 31u;               /* the bits before ours: zeros, neutral under OR */
        first = true;
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb)   /* v < 2^nb, nb <= 27 */
    {
        acc = (acc << nb) | v;
        nacc += nb;
        if (nacc >= 32u) {
            nacc -= 32u;
            const uint32_t x = __builtin_bswap32((uint32_t)(acc >> nacc));
            if (first) atomicOr(slots + head, x);
            else *wp = x;
            first = false;
            wp++;
        }
    }
    __device__ __forceinline__ void code(uint32_t c, uint32_t s, uint32_t extra) { put((c >> 8) << s | extra, (c & 0xffu) + s); }
    __device__ __forceinline__ void dc(uint32_t s, uint32_t extra) { code(dct[s], s, extra); }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t s, uint32_t extra) { code(act[sym], s, extra); }
    __device__ __forceinline__ void close()
    {
        if (!nacc) return;
        const uint32_t x = __builtin_bswap32((uint32_t)(acc << (32u - nacc)));
        if (first) atomicOr(slots + head, x);   /* the block ends in the word it starts in */
        else if (tail != ~0u) atomicOr(slots + tail, x);
        else atomicOr(wp, x);
    }
};

/* adds 1 to the symbol's bin of the workgroup's LDS histogram */
struct SymCount {
    uint32_t *dct, *act;
    __device__ __forceinline__ void dc(uint32_t s, uint32_t) { atomicAdd(dct + s, 1u); }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t, uint32_t) { atomicAdd(act + sym, 1u); }
};

/* workgroup exclusive scan (kT threads); total = the sum.  wtot: LDS [kT / 64] */
template <class T>
__device__ __forceinline__ T jf_scan(T x, T *wtot, T &total)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(incl, o, 64);
        if (lane >= (unsigned)o) incl += y;
    }
    if (lane == 63u) wtot[wave] = incl;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < kT / 64; w++) {
        const T y = wtot[w];
        if (w < wave) base += y;
        total += y;
    }
    __syncthreads();                    /* wtot is free again */
    return base + incl - x;
}

__device__ __forceinline__ void jf_tabs_to_lds(const JfTabs &t, uint32_t (*dc)[16], uint32_t (*ac)[256])
{
    for (unsigned i = threadIdx.x; i < 512u; i += kT) (&ac[0][0])[i] = (&t.ac[0][0])[i];
    if (threadIdx.x < 32u) (&dc[0][0])[threadIdx.x] = (&t.dc[0][0])[threadIdx.x];
    __syncthreads();
}

/* optimised mode (JPGX_JFIF_OPTIMIZE): what the call's own kernels leave per frame in the workspace */
struct JfOpt {
    unsigned long long *counts;         /* [nframes][4][256] symbol counts: DC luma, AC luma, DC chroma, AC chroma */
    JfTabs *tabs;                       /* [nframes] the frame's code tables */
    uint8_t *dht;                       /* [nframes][4][kDhtSlot] the frame's DHT segments */
    uint32_t *dhtlen;                   /* [nframes][4] their lengths */
};

/* the frame's tables in the workspace instead of the launch's by-value tables */
struct JfTabsOf {
    const JfTabs *p;
};

__device__ __forceinline__ void jf_tabs_to_lds(const JfTabsOf &t, uint32_t (*dc)[16], uint32_t (*ac)[256])
{
    jf_tabs_to_lds(t.p[blockIdx.y], dc, ac);
}

template <class Tabs>                   /* JfTabs: the launch's tables; JfTabsOf: the frame's own */
__global__ __launch_bounds__(kT) void k_jf_len(const JfArgs a, const Tabs tabs)
{
    __shared__ uint32_t tile[kT * kRow];
    __shared__ uint32_t dc[2][16], ac[2][256];
    __shared__ uint32_t wtot[kT / 64];
    const uint32_t iv = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    jf_tabs_to_lds(tabs, dc, ac);
    const uint32_t n = jf_nblk(a, iv);
    uint32_t *offs = a.offs + (size_t)f * a.g.nblk + (size_t)iv * a.ivblk;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += kT) {
        const uint32_t i = i0 + t;
        BitCount w{NULL, NULL, 0};
        if (i < n) {
            int diff;
            uint32_t ch;
            const uint64_t nz = jf_load(a, f, iv, i, tile + t * kRow, diff, ch);
            w.dct = dc[ch], w.act = ac[ch];
            jxe_walk(w, JfRow{tile + t * kRow}, nz, diff);
        }
        uint32_t total;
        const uint32_t ex = jf_scan(w.n, wtot, total);
        if (i < n) offs[i] = carry + ex;
        carry += total;
    }
    if (t == 0) a.ibits[(size_t)f * a.ni + iv] = carry;
}

/* the intervals' places in the frame's unstuffed stream, 16-byte aligned so that no word (and no
 * 16-byte read of k_jf_stuff) is shared by two workgroups; a frame whose places do not fit its
 * area (out_cap + 16 bytes per interval) cannot fit out_cap either */
__global__ __launch_bounds__(kT) void k_jf_place(const JfArgs a)
{
    __shared__ unsigned long long wtot[kT / 64];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t i0 = 0; i0 < a.ni; i0 += kT) {
        const uint32_t iv = i0 + t;
        unsigned long long sz = 0;
        if (iv < a.ni) sz = ((unsigned long long)((a.ibits[(size_t)f * a.ni + iv] + 7u) >> 3) + 15ull) & ~15ull;
        unsigned long long total;
        const unsigned long long ex = jf_scan(sz, wtot, total);
        if (iv < a.ni) a.ustart[(size_t)f * a.ni + iv] = carry + ex;
        carry += total;
    }
    if (t == 0) a.ovf[f] = carry > a.uarea ? 1u : 0u;
}

template <class Tabs>
__global__ __launch_bounds__(kT) void k_jf_pack(const JfArgs a, const Tabs tabs)
{
    __shared__ uint32_t tile[kT * kRow];
    __shared__ uint32_t dc[2][16], ac[2][256];
    __shared__ uint32_t wtot[kT / 64];
    __shared__ uint32_t slot[kT], hws[kT], rk[kT];
    const uint32_t iv = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (a.ovf[f]) return;
    jf_tabs_to_lds(tabs, dc, ac);
    const uint32_t n = jf_nblk(a, iv);
    const uint32_t bits = a.ibits[(size_t)f * a.ni + iv];
    const uint32_t nbytes = (bits + 7u) >> 3, nchunk = (nbytes + 15u) >> 4;
    uint8_t *area = a.ustream + (size_t)f * a.uarea + a.ustart[(size_t)f * a.ni + iv];
    for (uint32_t c = t; c < nchunk; c += kT) ((uint4 *)area)[c] = make_uint4(0, 0, 0, 0);
    __syncthreads();                    /* the interval's place is zero before any lane ORs into it */
    const uint32_t *offs = a.offs + (size_t)f * a.g.nblk + (size_t)iv * a.ivblk;
    for (uint32_t i0 = 0; i0 < n; i0 += kT) {
        const uint32_t i = i0 + t;
        const bool live = i < n;
        const uint32_t off = live ? offs[i] : 0u;
        /* slots: lane t starts in word hw; the distinct hw of this pass, in lane order, are the
         * slots (rank = the number of lanes before t that start a new word) */
        slot[t] = 0;
        hws[t] = live ? off >> 5 : ~0u;
        __syncthreads();
        const uint32_t opens = live && (t == 0 || hws[t - 1] != (off >> 5)) ? 1u : 0u;
        uint32_t nslots;
        const uint32_t rank = jf_scan(opens, wtot, nslots) + opens - 1u;      /* live: lane 0 opens */
        rk[t] = rank;
        __syncthreads();
        if (live) {
            int diff;
            uint32_t ch;
            const uint64_t nz = jf_load(a, f, iv, i, tile + t * kRow, diff, ch);
            const bool last = i + 1 == n || t + 1 == kT;       /* the next block is the next pass's */
            BitPack w;
            w.dct = dc[ch], w.act = ac[ch];
            w.open(area, off, slot, rank, last ? ~0u : rk[t + 1]);
            jxe_walk(w, JfRow{tile + t * kRow}, nz, diff);
            if (i + 1 == n) {           /* the interval's end: 1-bits up to the byte boundary */
                const uint32_t pad = (8u - (bits & 7u)) & 7u;
                if (pad) w.put((1u << pad) - 1u, pad);
            }
            w.close();
        }
        __syncthreads();                /* the slots are complete */
        if (opens) {                    /* lane 0's word may hold the previous pass's last bits */
            if (t == 0) atomicOr((uint32_t *)area + (off >> 5), slot[rank]);
            else ((uint32_t *)area)[off >> 5] = slot[rank];
        }
        __syncthreads();                /* before the next pass clears the slots */
    }
    __syncthreads();                    /* every lane's stores and ORs are done */
    /* the 0xFF bytes; loads at agent scope: the ORs were done in L2 */
    uint32_t cnt = 0;
    for (uint32_t c = t; c < 2u * nchunk; c += kT) {
        const unsigned long long x =
            __hip_atomic_load((const unsigned long long *)area + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int b = 0; b < 8; b++) cnt += ((x >> (8 * b)) & 0xffull) == 0xffull ? 1u : 0u;
    }
    uint32_t total;
    jf_scan(cnt, wtot, total);
    if (t == 0) a.nff[(size_t)f * a.ni + iv] = total;
}

/* per frame: where each interval's stuffed bytes go, the length (or the overflow report: bit 63 and
 * a capacity that suffices whatever the stuffing -- headers + 2 x unstuffed bytes + markers + EOI),
 * the header bytes and EOI */
template <class Hdr>                    /* JfHdr: one header for the batch; JfHdrOpt: the frame's own */
__global__ __launch_bounds__(kT) void k_jf_frame(const JfArgs a, const Hdr hdr)
{
    __shared__ unsigned long long wtot[kT / 64];
    __shared__ uint32_t fits;
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const bool early = a.ovf[f] != 0;
    const uint32_t hdrlen = hdr.length(a, f);
    unsigned long long carry = hdrlen, raw = 0;
    for (uint32_t i0 = 0; i0 < a.ni; i0 += kT) {
        const uint32_t iv = i0 + t;
        unsigned long long sz = 0, un = 0;
        if (iv < a.ni) {
            un = (a.ibits[(size_t)f * a.ni + iv] + 7u) >> 3;
            sz = un + (early ? 0u : a.nff[(size_t)f * a.ni + iv]) + (iv + 1 < a.ni ? 2u : 0u);
        }
        unsigned long long total, rtotal;
        const unsigned long long ex = jf_scan(sz, wtot, total);
        jf_scan(un, wtot, rtotal);
        if (iv < a.ni) a.ostart[(size_t)f * a.ni + iv] = carry + ex;
        carry += total;
        raw += rtotal;
    }
    const unsigned long long len = carry + 2;
    if (t == 0) {
        const bool ok = !early && len <= a.ocap;
        fits = ok ? 1u : 0u;
        a.ovf[f] = ok ? 0u : 1u;
        a.len[f] = ok ? len : (1ull << 63) | (hdrlen + 2 * raw + 2ull * (a.ni - 1) + 2);
    }
    __syncthreads();
    if (!fits) return;
    uint8_t *out = a.out + (size_t)f * a.ostride;
    for (uint32_t i = t; i < hdrlen; i += kT) out[i] = hdr.byte(f, i);
    if (t < 2) out[len - 2 + t] = t ? 0xd9 : 0xff;
}

/* unstuffed bytes -> file bytes: a lane takes 16 bytes, a workgroup scan of the 0xFF counts places
 * them; RSTm (m = interval index mod 8) after every interval but the last */
__global__ __launch_bounds__(kT) void k_jf_stuff(const JfArgs a)
{
    __shared__ uint32_t wtot[kT / 64];
    const uint32_t iv = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (a.ovf[f]) return;
    const uint32_t nbytes = (a.ibits[(size_t)f * a.ni + iv] + 7u) >> 3;
    const uint8_t *area = a.ustream + (size_t)f * a.uarea + a.ustart[(size_t)f * a.ni + iv];
    uint8_t *out = a.out + (size_t)f * a.ostride + a.ostart[(size_t)f * a.ni + iv];
    uint32_t carry = 0;
    for (uint32_t c0 = 0; 16u * c0 < nbytes; c0 += kT) {
        const uint32_t c = c0 + t;
        const uint32_t nv = 16u * c < nbytes ? min(16u, nbytes - 16u * c) : 0u;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (nv) q = ((const uint4 *)area)[c];       /* bytes past nbytes in the place are zero */
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t cnt = 0;
#pragma unroll
        for (int b = 0; b < 16; b++) cnt += ((w[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0xffu ? 1u : 0u;
        uint32_t total;
        uint32_t pos = 16u * c + carry + jf_scan(cnt, wtot, total);
        carry += total;
#pragma unroll
        for (int b = 0; b < 16; b++) {
            if ((uint32_t)b < nv) {
                const uint32_t x = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
                out[pos++] = (uint8_t)x;
                if (x == 0xffu) out[pos++] = 0;
            }
        }
    }
    if (t < 2 && iv + 1 < a.ni) out[nbytes + carry + t] = t ? (uint8_t)(0xd0u + (iv & 7u)) : (uint8_t)0xff;
}

/* ---- optimised mode: the frame's symbol counts and its tables ------------------------------- */

/* the counts start at zero in every call (a kernel, not a memset: capturable, and nothing depends
 * on what the workspace held) */
__global__ __launch_bounds__(kT) void k_jf_zero(const JfOpt o)
{
    unsigned long long *c = o.counts + (size_t)blockIdx.x * 1024;
    for (uint32_t i = threadIdx.x; i < 1024u; i += kT) c[i] = 0;
}

constexpr int kBins = 2 * 16 + 2 * 256;  /* DC luma, DC chroma, AC luma, AC chroma */

/* one workgroup per restart interval, as k_jf_len: the interval's symbols into LDS bins, the bins
 * into the frame's counts with 64-bit atomic adds (integer sums: the order does not show).  One
 * histogram for the workgroup: a copy per wave measured slower */
__global__ __launch_bounds__(kT) void k_jf_count(const JfArgs a, const JfOpt o)
{
    __shared__ uint32_t tile[kT * kRow];
    __shared__ uint32_t h[kBins];
    const uint32_t iv = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    for (uint32_t i = t; i < (uint32_t)kBins; i += kT) h[i] = 0;
    __syncthreads();
    const uint32_t n = jf_nblk(a, iv);
    for (uint32_t i = t; i < n; i += kT) {
        int diff;
        uint32_t ch;
        const uint64_t nz = jf_load(a, f, iv, i, tile + t * kRow, diff, ch);
        SymCount w{h + 16u * ch, h + 32u + 256u * ch};
        jxe_walk(w, JfRow{tile + t * kRow}, nz, diff);
    }
    __syncthreads();
    unsigned long long *counts = o.counts + (size_t)f * 1024;
    for (uint32_t i = t; i < (uint32_t)kBins; i += kT) {
        const uint32_t c = h[i];
        /* bins 0..31: DC [chroma][16] -> tables 0 / 2; then AC [chroma][256] -> tables 1 / 3 */
        const uint32_t at = i < 32u ? (i >> 4) * 512u + (i & 15u) : 256u + ((i - 32u) >> 8) * 512u + ((i - 32u) & 255u);
        if (c) atomicAdd(counts + at, (unsigned long long)c);
    }
}

/* x of the lane a DPP control names (every lane is active where this is used) */
template <int kCtrl>
__device__ __forceinline__ unsigned long long jf_dpp(unsigned long long x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, kCtrl, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), kCtrl, 0xf, 0xf, false);
    return (unsigned long long)hi << 32 | lo;
}

__device__ __forceinline__ unsigned long long jf_lane(unsigned long long x, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
    return (unsigned long long)hi << 32 | lo;
}

__device__ __forceinline__ unsigned long long jf_least(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

/* the wave's least key, the same in every lane (every lane active).  Within a row of 16 lanes the
 * exchange is DPP (neighbours, pairs, the mirrored half row, the mirrored row: after each step the
 * groups exchanged are uniform), the four rows meet through lane reads: no LDS round trip and no
 * barrier, which is what a merge's time was made of */
__device__ __forceinline__ unsigned long long jf_wave_min(unsigned long long key)
{
    key = jf_least(key, jf_dpp<0xb1>(key));                /* quad_perm [1, 0, 3, 2] */
    key = jf_least(key, jf_dpp<0x4e>(key));                /* quad_perm [2, 3, 0, 1] */
    key = jf_least(key, jf_dpp<0x141>(key));               /* row_half_mirror */
    key = jf_least(key, jf_dpp<0x140>(key));               /* row_mirror */
    return jf_least(jf_least(jf_lane(key, 0), jf_lane(key, 16)), jf_least(jf_lane(key, 32), jf_lane(key, 48)));
}

/* jx_jfif_optimal (host/jpgx_jfif.c, csrc/jpgx_internal.h) for table blockIdx.x of frame blockIdx.y,
 * bit for bit.  The merges (Figure K.1) run on the first wave alone, in registers: lane l owns
 * symbols l, l + 64, l + 128 and l + 192, every lane the reserved point 256.  A merge searches the
 * least nonzero frequency twice (a wave reduction of keys freq << 9 | 256 - index: the least
 * frequency, on a tie the largest index; a frame's symbols number below 2^34, so the key holds every
 * sum).  A symbol's `others` chain is the set of symbols of its tree, so a lane keeps the tree each
 * of its symbols is in and the two trees' members take their codesize + 1 at once.  Then the whole
 * workgroup, a lane per symbol: the sizes are counted (Figure K.2), limited by one lane (K.3), the
 * symbols ranked by (codesize, value) (K.4) and coded (Annex C); out go the packed codes, the DHT
 * segment and its length. */
__global__ __launch_bounds__(kT) void k_jf_tables(const JfOpt o)
{
    __shared__ uint32_t nsz[258], csz[kT + 1], first[17], upto[17], deepest;
    __shared__ uint8_t vals[kT];
    const uint32_t tb = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    for (uint32_t i = t; i < 258u; i += kT) nsz[i] = 0;
    if (t == 0) deepest = 0;
    if (t < 64u) {
        constexpr unsigned long long kNone = ~0ull;
        unsigned long long fr[4], fr256 = 1;
        uint32_t tree[4], c[4], tree256 = 256u, c256 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            fr[k] = o.counts[((size_t)f * 4 + tb) * 256 + t + 64u * k];
            tree[k] = t + 64u * k;
            c[k] = 0;
        }
        for (int it = 0; it < 256; it++) {                 /* 257 leaves: at most 256 merges */
            unsigned long long key = fr256 ? fr256 << 9 : kNone;          /* 256 - 256 = 0: wins every tie */
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (fr[k]) key = jf_least(key, fr[k] << 9 | (256u - t - 64u * k));
            const unsigned long long k1 = jf_wave_min(key);
            const uint32_t v1 = 256u - (uint32_t)(k1 & 511u);
            key = fr256 && v1 != 256u ? fr256 << 9 : kNone;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (fr[k] && t + 64u * k != v1) key = jf_least(key, fr[k] << 9 | (256u - t - 64u * k));
            const unsigned long long k2 = jf_wave_min(key);
            if (k2 == kNone) break;                        /* the same for every lane */
            const uint32_t v2 = 256u - (uint32_t)(k2 & 511u);
            const unsigned long long sum = (k1 >> 9) + (k2 >> 9);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                if (t + 64u * k == v1) fr[k] = sum;
                if (t + 64u * k == v2) fr[k] = 0;
                if (tree[k] == v1 || tree[k] == v2) c[k]++, tree[k] = v1;
            }
            if (v1 == 256u) fr256 = sum;
            if (v2 == 256u) fr256 = 0;
            if (tree256 == v1 || tree256 == v2) c256++, tree256 = v1;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) csz[t + 64u * k] = c[k];
        if (t == 0) csz[kT] = c256;
    }
    __syncthreads();                                       /* the code sizes; nsz is zero */
    const uint32_t cs = csz[t];
    if (cs) atomicAdd(nsz + cs, 1u), atomicMax(&deepest, cs);
    if (t == 0 && csz[kT]) atomicAdd(nsz + csz[kT], 1u), atomicMax(&deepest, csz[kT]);
    __syncthreads();
    if (t == 0) {
        for (uint32_t i = deepest; i > 16u; i--)
            while (nsz[i] > 0) {
                uint32_t j = i - 2u;
                while (j > 0 && nsz[j] == 0) j--;
                nsz[i] -= 2u;
                nsz[i - 1u]++;
                nsz[j + 1u] += 2u;
                nsz[j]--;
            }
        uint32_t last = 16;
        while (last > 0 && nsz[last] == 0) last--;
        if (last) nsz[last]--;
        uint32_t code = 0, k = 0;                          /* Annex C: the first code of each length */
        for (uint32_t l = 1; l <= 16u; l++) {
            first[l] = code;
            k += nsz[l];
            upto[l] = k;                                   /* values of length <= l */
            code = (code + nsz[l]) << 1;
        }
    }
    /* rank among the used symbols by (codesize, value) */
    uint32_t rank = 0, used = 0;
    for (uint32_t i = 0; i < (uint32_t)kT; i++) {
        const uint32_t c = csz[i];
        used += c ? 1u : 0u;
        rank += c && (c < cs || (c == cs && i < t)) ? 1u : 0u;
    }
    __syncthreads();                                       /* first, upto and the limited nsz */
    uint32_t cl = 0;
    if (cs) {
        uint32_t l = 1;
        while (l < 16u && rank >= upto[l]) l++;
        cl = (first[l] + rank - (l > 1u ? upto[l - 1u] : 0u)) << 8 | l;
        vals[rank] = (uint8_t)t;
    }
    JfTabs *tabs = o.tabs + f;
    if (tb & 1u) tabs->ac[tb >> 1][t] = cl;
    else if (t < 16u) tabs->dc[tb >> 1][t] = cl;
    __syncthreads();                                       /* vals */
    uint8_t *dht = o.dht + ((size_t)f * 4 + tb) * kDhtSlot;
    const uint32_t seg = 2u + 1u + 16u + used;             /* the segment's length field */
    if (t < 21u) {
        const uint32_t id = (tb & 1u) << 4 | tb >> 1;      /* 0x00, 0x10, 0x01, 0x11 */
        dht[t] = t == 0 ? 0xff : t == 1 ? 0xc4 : t == 2 ? (uint8_t)(seg >> 8) : t == 3 ? (uint8_t)seg
                 : t == 4 ? (uint8_t)id : (uint8_t)nsz[t - 4u];
    }
    if (t < used && 21u + t < (uint32_t)kDhtSlot) dht[21u + t] = vals[t];
    if (t == 0) o.dhtlen[(size_t)f * 4 + tb] = min(2u + seg, (uint32_t)kDhtSlot);
}

/* which frame an entry point codes: whole MCUs only, the coded frame of a width x height file of any
 * size, or a one-component file's blocks (sample_ratio unused; an MCU is a block, an MCU row a block row) */
enum JfKind { kWhole, kAny, kGray };

/* geometry and argument checks shared by the size query and the call; a.hdrlen stays 0.  The
 * device codes with restart intervals only: restart_rows 0 is refused, -1 is one MCU row */
int jf_geometry(JfKind kind, int width, int height, int sample_ratio, int restart_rows, size_t nframes, JfArgs &a)
{
    if (restart_rows == 0 || restart_rows < -1 || !jx_frames_ok(nframes)) return JPGX_EARG;
    jx_frame_any fa;
    const bool any = kind == kAny;
    const int rc = jx_frame_rc_coder(kind == kGray ? jx_frame_make_gray_coded(width, height, &a.g)
                                     : any         ? jx_frame_make_any(width, height, sample_ratio, &fa)
                                                   : jx_frame_make(width, height, sample_ratio, &a.g));
    if (rc) return rc;
    if (any) a.g = fa.c;
    a.rpi = restart_rows > 0 ? (uint32_t)restart_rows : 1u;
    if (a.rpi > jx_frame_max_rows(&a.g)) return JPGX_EARG;
    a.ni = (a.g.cbh + a.rpi - 1) / a.rpi;
    a.ivblk = a.rpi * a.g.cbw * a.g.bpm;
    return JPGX_OK;
}

struct JfLayout {
    size_t offs, ibits, nff, ustart, ostart, ovf, ustream, uarea, total;
    size_t counts, tabs, dht, dhtlen;   /* JPGX_JFIF_OPTIMIZE only */
};

JfLayout jf_layout(const JfArgs &a, size_t nframes, size_t out_cap, unsigned jfif_flags)
{
    JfLayout l;
    jx_carve ws;
    l.offs = ws.take(nframes * a.g.nblk * sizeof(uint32_t));
    l.ibits = ws.take(nframes * a.ni * sizeof(uint32_t));
    l.nff = ws.take(nframes * a.ni * sizeof(uint32_t));
    l.ustart = ws.take(nframes * a.ni * sizeof(unsigned long long));
    l.ostart = ws.take(nframes * a.ni * sizeof(unsigned long long));
    l.ovf = ws.take(nframes * sizeof(uint32_t));
    l.uarea = jx_r16(out_cap) + 16 * (size_t)a.ni;
    l.ustream = ws.take(nframes * l.uarea);
    l.counts = l.tabs = l.dht = l.dhtlen = 0;
    if (jfif_flags & JPGX_JFIF_OPTIMIZE) {
        l.counts = ws.take(nframes * 4 * 256 * sizeof(unsigned long long));
        l.tabs = ws.take(nframes * sizeof(JfTabs));
        l.dht = ws.take(nframes * 4 * kDhtSlot);
        l.dhtlen = ws.take(nframes * 4 * sizeof(uint32_t));
    }
    l.total = ws.at;
    return l;
}

size_t jf_workspace_size(JfKind kind, int width, int height, int sample_ratio, int restart_rows, size_t nframes,
                         size_t out_cap, unsigned jfif_flags)
{
    JfArgs a;
    if (jfif_flags & ~JPGX_JFIF_OPTIMIZE) return 0;
    if (jf_geometry(kind, width, height, sample_ratio, restart_rows, nframes, a)) return 0;
    return jf_layout(a, nframes, out_cap, jfif_flags).total;
}

}  // namespace

extern "C" {

size_t jpgx_jfif_gpu_workspace_size(int width, int height, int sample_ratio, int restart_rows, size_t nframes,
                                    size_t out_cap)
{
    return jpgx_jfif_gpu_workspace_size_ex(width, height, sample_ratio, restart_rows, nframes, out_cap, 0u);
}

size_t jpgx_jfif_gpu_workspace_size_ex(int width, int height, int sample_ratio, int restart_rows, size_t nframes,
                                       size_t out_cap, unsigned jfif_flags)
{
    return jf_workspace_size(kWhole, width, height, sample_ratio, restart_rows, nframes, out_cap, jfif_flags);
}

size_t jpgx_jfif_gpu_any_workspace_size(int width, int height, int sample_ratio, int restart_rows, size_t nframes,
                                        size_t out_cap, unsigned jfif_flags)
{
    return jf_workspace_size(kAny, width, height, sample_ratio, restart_rows, nframes, out_cap, jfif_flags);
}

size_t jpgx_jfif_gpu_gray_workspace_size(int width, int height, int restart_rows, size_t nframes, size_t out_cap,
                                         unsigned jfif_flags)
{
    return jf_workspace_size(kGray, width, height, 0, restart_rows, nframes, out_cap, jfif_flags);
}

int jpgx_jfif_gpu(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                  int quality, int sample_ratio, int restart_rows, uint8_t *d_out, size_t out_frame_stride,
                  size_t out_cap, uint64_t *d_len, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return jpgx_jfif_gpu_ex(d_coef, coef_frame_stride, nframes, width, height, quality, sample_ratio, restart_rows,
                            0u, d_out, out_frame_stride, out_cap, d_len, d_workspace, workspace_bytes, stream);
}

}  /* extern "C" */

namespace {

/* jpgx_jfif_gpu_ex, and with kAny jpgx_jfif_gpu_any: the same kernels over the coded frame of a
 * width x height file; the header states the file's own size, the restart interval counts the coded
 * frame's MCUs.  With kGray jpgx_jfif_gpu_gray: the same kernels over the one-component frame, with the
 * one-component header and, optimised, two tables per frame instead of four */
int jf_code(JfKind kind, const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
            int quality, int sample_ratio, int restart_rows, unsigned jfif_flags, uint8_t *d_out,
            size_t out_frame_stride, size_t out_cap, uint64_t *d_len, void *d_workspace,
            size_t workspace_bytes, void *stream)
{
    JfArgs a;
    memset(&a, 0, sizeof a);
    if (jfif_flags & ~JPGX_JFIF_OPTIMIZE) return JPGX_EARG;
    if (!d_coef || !d_out || !d_len || !d_workspace || ((uintptr_t)d_coef & 15) || ((uintptr_t)d_out & 15) ||
        ((uintptr_t)d_len & 7) || ((uintptr_t)d_workspace & 15))
        return JPGX_EARG;
    const bool gray = kind == kGray;
    int rc = jf_geometry(kind, width, height, sample_ratio, restart_rows, nframes, a);
    if (rc) return rc;
    if (!jx_coef_batch_ok(coef_frame_stride, a.g.nblk) || out_frame_stride < out_cap) return JPGX_EARG;
    JfHdr hdr;
    memset(&hdr, 0, sizeof hdr);
    size_t dht_at = 0;
    const size_t hl = gray ? jx_jfif_header_gray(width, height, quality, a.rpi * a.g.cbw, NULL, NULL, hdr.b,
                                                 sizeof hdr.b, &dht_at)
                           : jx_jfif_header_tabs(width, height, quality, sample_ratio, a.rpi * a.g.cbw, NULL, NULL,
                                                 hdr.b, sizeof hdr.b, &dht_at);
    if (!hl) return JPGX_EQUALITY;
    if (hl > sizeof hdr.b) return JPGX_EARG;
    const JfLayout l = jf_layout(a, nframes, out_cap, jfif_flags);
    if (workspace_bytes < l.total) return JPGX_EWORKSPACE;
    uint32_t cl[4][256];
    jx_jfif_codes(cl);
    JfTabs tabs;
    for (int c = 0; c < 2; c++) {
        memcpy(tabs.dc[c], cl[2 * c], sizeof tabs.dc[c]);
        memcpy(tabs.ac[c], cl[2 * c + 1], sizeof tabs.ac[c]);
    }
    char *ws = (char *)d_workspace;
    a.coef = d_coef;
    a.fstride = coef_frame_stride;
    a.hdrlen = (uint32_t)hl;
    a.offs = (uint32_t *)(ws + l.offs);
    a.ibits = (uint32_t *)(ws + l.ibits);
    a.nff = (uint32_t *)(ws + l.nff);
    a.ustart = (unsigned long long *)(ws + l.ustart);
    a.ostart = (unsigned long long *)(ws + l.ostart);
    a.ovf = (uint32_t *)(ws + l.ovf);
    a.ustream = (uint8_t *)(ws + l.ustream);
    a.uarea = l.uarea;
    a.out = d_out;
    a.ostride = out_frame_stride;
    a.ocap = out_cap;
    a.len = (unsigned long long *)d_len;
    hipStream_t s = (hipStream_t)stream;
    const dim3 per_interval(a.ni, (unsigned)nframes), per_frame((unsigned)nframes);
    if (jfif_flags & JPGX_JFIF_OPTIMIZE) {
        /* the standard header around its DHT segments: what every frame's header shares */
        JfHdrOpt ho;
        memset(&ho, 0, sizeof ho);
        const size_t suf_at = dht_at + (gray ? JX_JFIF_DHT_STD_GRAY : JX_JFIF_DHT_STD);
        if (dht_at > sizeof ho.pre || suf_at > hl || hl - suf_at > sizeof ho.suf) return JPGX_EARG;
        memcpy(ho.pre, hdr.b, dht_at);
        memcpy(ho.suf, hdr.b + suf_at, hl - suf_at);
        ho.npre = (uint32_t)dht_at;
        ho.nsuf = (uint32_t)(hl - suf_at);
        JfOpt o;
        o.counts = (unsigned long long *)(ws + l.counts);
        o.tabs = (JfTabs *)(ws + l.tabs);
        o.dht = (uint8_t *)(ws + l.dht);
        o.dhtlen = (uint32_t *)(ws + l.dhtlen);
        ho.dht = o.dht;
        ho.dhtlen = o.dhtlen;
        const JfTabsOf tof{o.tabs};
        hipLaunchKernelGGL(k_jf_zero, per_frame, dim3(kT), 0, s, o);
        hipLaunchKernelGGL(k_jf_count, per_interval, dim3(kT), 0, s, a, o);
        hipLaunchKernelGGL(k_jf_tables, dim3(gray ? 2 : 4, (unsigned)nframes), dim3(kT), 0, s, o);
        hipLaunchKernelGGL(k_jf_len<JfTabsOf>, per_interval, dim3(kT), 0, s, a, tof);
        hipLaunchKernelGGL(k_jf_place, per_frame, dim3(kT), 0, s, a);
        hipLaunchKernelGGL(k_jf_pack<JfTabsOf>, per_interval, dim3(kT), 0, s, a, tof);
        if (gray) {                                        /* the same bytes around two segments */
            JfHdrOptGray hg;
            memcpy(hg.pre, ho.pre, sizeof hg.pre);
            memcpy(hg.suf, ho.suf, sizeof hg.suf);
            hg.npre = ho.npre, hg.nsuf = ho.nsuf, hg.dht = ho.dht, hg.dhtlen = ho.dhtlen;
            hipLaunchKernelGGL(k_jf_frame<JfHdrOptGray>, per_frame, dim3(kT), 0, s, a, hg);
        } else {
            hipLaunchKernelGGL(k_jf_frame<JfHdrOpt>, per_frame, dim3(kT), 0, s, a, ho);
        }
        hipLaunchKernelGGL(k_jf_stuff, per_interval, dim3(kT), 0, s, a);
        return jx_hip_rc(hipGetLastError());
    }
    hipLaunchKernelGGL(k_jf_len<JfTabs>, per_interval, dim3(kT), 0, s, a, tabs);
    hipLaunchKernelGGL(k_jf_place, per_frame, dim3(kT), 0, s, a);
    hipLaunchKernelGGL(k_jf_pack<JfTabs>, per_interval, dim3(kT), 0, s, a, tabs);
    hipLaunchKernelGGL(k_jf_frame<JfHdr>, per_frame, dim3(kT), 0, s, a, hdr);
    hipLaunchKernelGGL(k_jf_stuff, per_interval, dim3(kT), 0, s, a);
    return jx_hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

int jpgx_jfif_gpu_ex(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                     int quality, int sample_ratio, int restart_rows, unsigned jfif_flags, uint8_t *d_out,
                     size_t out_frame_stride, size_t out_cap, uint64_t *d_len, void *d_workspace,
                     size_t workspace_bytes, void *stream)
{
    return jf_code(kWhole, d_coef, coef_frame_stride, nframes, width, height, quality, sample_ratio, restart_rows,
                   jfif_flags, d_out, out_frame_stride, out_cap, d_len, d_workspace, workspace_bytes, stream);
}

int jpgx_jfif_gpu_any(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                      int quality, int sample_ratio, int restart_rows, unsigned jfif_flags, uint8_t *d_out,
                      size_t out_frame_stride, size_t out_cap, uint64_t *d_len, void *d_workspace,
                      size_t workspace_bytes, void *stream)
{
    return jf_code(kAny, d_coef, coef_frame_stride, nframes, width, height, quality, sample_ratio, restart_rows,
                   jfif_flags, d_out, out_frame_stride, out_cap, d_len, d_workspace, workspace_bytes, stream);
}

int jpgx_jfif_gpu_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                       int quality, int restart_rows, unsigned jfif_flags, uint8_t *d_out, size_t out_frame_stride,
                       size_t out_cap, uint64_t *d_len, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return jf_code(kGray, d_coef, coef_frame_stride, nframes, width, height, quality, 0, restart_rows, jfif_flags,
                   d_out, out_frame_stride, out_cap, d_len, d_workspace, workspace_bytes, stream);
}

}  /* extern "C" */
