/*
 * jpgx_jfif_dec.hip -- baseline JFIF files in device memory back to the coefficient layout
 * (DESIGN.md 4.8): jpgx_jfif_decode_gpu.  Entropy decoding only.  The routines that touch the
 * file's bytes are those of jx_jfif_dec.h, the same source the host decoder (jpgx_jfif_read.cpp)
 * compiles: this file adds where they run.  Five launches per batch, nothing else on the stream:
 *   k_jd_header  per frame: the header walk and the four decode tables into the workspace (one
 *                lane: the walk is serial), the stated geometry checked, d_qt
 *   k_jd_count   per 4 KiB chunk of a file: a lane takes 16 bytes, looks one byte ahead and counts
 *                the restart markers (FF D0 .. D7) that begin in its piece; the chunk's count
 *   k_jd_frame   per frame: the chunks' counts scanned into each chunk's first marker number; the
 *                count must be intervals - 1 and EOI must end the file; d_status
 *   k_jd_place   per chunk: the same search, every marker's place stored at its number, its number
 *                checked against k mod 8
 *   k_jd_scan    one lane per restart interval, one-wave workgroups (so the intervals of a frame
 *                spread over the compute units), the tables in LDS: jxd_decode_interval
 * A lane's interval is a serial bit stream: the lanes of a wave diverge in every loop.  With
 * JPGX_JFIF_DECODE_SUBINTERVAL (jpgx_jfif_decode_gpu_ex) the last launch is instead
 *   k_jd_sub     one workgroup of 256 lanes per restart interval (a bounded grid strides over
 *                them): the interval tile by tile through LDS, a lane per subsequence of JXS_SUB
 *                bytes starting at a guessed place, the exit states handed on in rounds until they
 *                are the sequential decoder's, then placed and written: jx_jfif_sub.h's routines,
 *                which the host twin jpgx_read_jfif_sub runs too
 * jpgx_jfif_decode_gpu_any (files of any width and height) differs in the header kernel's mode alone:
 * the other kernels see the coded frame's counts.
 * The interval's blocks are zeroed and filled by the lanes that decode them; no memset.
 * The call keeps no state and is capturable.
 */
#include <stdint.h>
#include <string.h>

#include "jx_frame.h"
#include "jx_hip.h"
#include "jx_jfif_dec.h"
#include "jx_jfif_sub.h"

namespace {

constexpr int kT = 256;                 /* threads of the search kernels */
constexpr uint32_t kPiece = 16;         /* bytes per lane */
constexpr uint32_t kChunk = kT * kPiece;/* bytes per workgroup */
constexpr int kWave = 64;               /* lanes = intervals per workgroup of k_jd_scan */

struct JdArgs {
    const uint8_t *files;
    unsigned long long fstride;         /* bytes between files */
    const unsigned long long *len;
    uint32_t width, height, hs, vs;     /* the geometry the caller states */
    uint32_t nblk;                      /* blocks per frame of that geometry */
    uint32_t nmcu;                      /* MCUs per frame: the most intervals a file can have */
    uint32_t nchunk;                    /* chunks per file slot */
    int16_t *coef;
    unsigned long long cstride;         /* int16 elements */
    uint16_t *qt;                       /* [nframes][2][64] or NULL */
    int32_t *status;                    /* [nframes] */
    jxd_frame *frames;                  /* [nframes] */
    jxd_tab *tabs;                      /* [nframes][4] */
    int32_t *st;                        /* [nframes] the status before the scan */
    uint32_t *cnt;                      /* [nframes][nchunk] markers of the chunk, then before the chunk */
    uint32_t *mpos;                     /* [nframes][nmcu] the markers' places */
};

/* workgroup exclusive scan (kT threads); total = the sum.  wtot: LDS [kT / 64] */
__device__ __forceinline__ uint32_t jd_scan(uint32_t x, uint32_t *wtot, uint32_t &total)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= (unsigned)o) incl += y;
    }
    if (lane == 63u) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < kT / 64; w++) {
        const uint32_t y = wtot[w];
        if (w < wave) base += y;
        total += y;
    }
    __syncthreads();                    /* wtot is free again */
    return base + incl - x;
}

/* ANY: the header walk's mode (jx_jfif_dec.h) -- the file's width and height are compared as they
 * stand in SOF, its counts are the coded frame's */
template <int ANY>
__global__ __launch_bounds__(kWave) void k_jd_header(const JdArgs a)
{
    __shared__ int32_t rc_s;
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    jxd_frame *fr = a.frames + f;
    if (t == 0) {
        const unsigned long long len = a.len[f];
        int rc = JPGX_EJFIF_HEADER;     /* bit 63 (an overflow report) is above every stride */
        if (len <= a.fstride) rc = jxd_parse_header<ANY>(a.files + (size_t)f * a.fstride, (size_t)len, fr, a.tabs + 4 * (size_t)f);
        if (!rc && (fr->width != a.width || fr->height != a.height || fr->hs != a.hs || fr->vs != a.vs))
            rc = JPGX_EJFIF_HEADER;
        a.st[f] = rc;
        rc_s = rc;
    }
    __syncthreads();                    /* thread 0's stores to *fr are visible to the workgroup */
    if (a.qt)
        for (uint32_t i = t; i < 128u; i += kWave) a.qt[(size_t)f * 128 + i] = rc_s ? (uint16_t)0 : (&fr->qt[0][0])[i];
}

/* the restart markers that begin in this lane's piece of chunk c: a bit per byte */
__device__ __forceinline__ uint32_t jd_piece(const uint8_t *file, size_t len, size_t scan_off, uint32_t c, uint32_t t)
{
    const size_t p0 = (size_t)c * kChunk + (size_t)t * kPiece;
    uint32_t mask = 0;
    if (p0 + kPiece <= scan_off || p0 + 1 >= len) return 0;
    for (uint32_t j = 0; j < kPiece; j++)
        if (jxd_is_rst(file, len, scan_off, p0 + j)) mask |= 1u << j;
    return mask;
}

__global__ __launch_bounds__(kT) void k_jd_count(const JdArgs a)
{
    __shared__ uint32_t wtot[kT / 64];
    const uint32_t c = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    uint32_t mask = 0;
    if (!a.st[f]) mask = jd_piece(a.files + (size_t)f * a.fstride, (size_t)a.len[f], (size_t)a.frames[f].scan_off, c, t);
    uint32_t total;
    jd_scan((uint32_t)__builtin_popcount(mask), wtot, total);
    if (t == 0) a.cnt[(size_t)f * a.nchunk + c] = total;
}

__global__ __launch_bounds__(kT) void k_jd_frame(const JdArgs a)
{
    __shared__ uint32_t wtot[kT / 64];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    uint32_t *cnt = a.cnt + (size_t)f * a.nchunk;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < a.nchunk; c0 += kT) {
        const uint32_t c = c0 + t;
        const uint32_t x = c < a.nchunk ? cnt[c] : 0u;
        uint32_t total;
        const uint32_t ex = jd_scan(x, wtot, total);
        if (c < a.nchunk) cnt[c] = carry + ex;
        carry += total;
    }
    if (t == 0) {
        int rc = a.st[f];
        if (!rc) {
            const jxd_frame *fr = a.frames + f;
            if (carry != fr->ni - 1u ||
                !jxd_has_eoi(a.files + (size_t)f * a.fstride, (size_t)a.len[f], (size_t)fr->scan_off))
                rc = JPGX_EJFIF_SCAN;
        }
        a.st[f] = rc;
        a.status[f] = rc;
    }
}

__global__ __launch_bounds__(kT) void k_jd_place(const JdArgs a)
{
    __shared__ uint32_t wtot[kT / 64];
    const uint32_t c = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (a.st[f]) return;
    const jxd_frame *fr = a.frames + f;
    const uint8_t *file = a.files + (size_t)f * a.fstride;
    uint32_t mask = jd_piece(file, (size_t)a.len[f], (size_t)fr->scan_off, c, t);
    uint32_t total;
    uint32_t k = a.cnt[(size_t)f * a.nchunk + c] + jd_scan((uint32_t)__builtin_popcount(mask), wtot, total);
    const uint32_t nmark = fr->ni - 1u;             /* at most nmcu - 1: inside the frame's mpos */
    const size_t p0 = (size_t)c * kChunk + (size_t)t * kPiece;
    while (mask) {
        const uint32_t j = (uint32_t)__builtin_ctz(mask);
        mask &= mask - 1u;
        if (k < nmark && k < a.nmcu) {
            a.mpos[(size_t)f * a.nmcu + k] = (uint32_t)(p0 + j);
            if ((file[p0 + j + 1] & 7u) != (k & 7u)) a.status[f] = JPGX_EJFIF_SCAN;
        }
        k++;
    }
}

__global__ __launch_bounds__(kWave) void k_jd_scan(const JdArgs a)
{
    __shared__ jxd_tab tabs[4];
    static_assert(sizeof(jxd_tab) % 4 == 0, "tables are copied by dwords");
    const uint32_t f = blockIdx.y, t = threadIdx.x;
    if (a.st[f]) return;                /* the same for the whole workgroup */
    const jxd_frame *fr = a.frames + f;
    const uint32_t ni = fr->ni;
    if (blockIdx.x * kWave >= ni) return;
    const uint32_t *src = (const uint32_t *)(a.tabs + 4 * (size_t)f);
    for (uint32_t i = t; i < 4u * sizeof(jxd_tab) / 4u; i += kWave) ((uint32_t *)tabs)[i] = src[i];
    __syncthreads();
    const uint32_t iv = blockIdx.x * kWave + t;
    if (iv >= ni) return;
    const size_t len = (size_t)a.len[f];
    const uint32_t *mpos = a.mpos + (size_t)f * a.nmcu;
    const size_t begin = iv ? (size_t)mpos[iv - 1] + 2 : (size_t)fr->scan_off;
    const size_t end = iv + 1 < ni ? (size_t)mpos[iv] : len - 2;
    const uint32_t mcu0 = iv * fr->mpi;
    const uint32_t count = min(fr->mpi, fr->nmcu - mcu0);
    /* the header kernel has checked the file's geometry against the stated one, for which the
     * caller's coef_frame_stride was checked: fr->nblk blocks fit the frame's slot */
    if (fr->nblk != a.nblk) return;
    if (jxd_decode_interval(a.files + (size_t)f * a.fstride, len, begin, end, fr, tabs, mcu0, count,
                            a.coef + (size_t)f * a.cstride))
        a.status[f] = JPGX_EJFIF_SCAN;
}

/* ---- inside an interval: jx_jfif_sub.h's routines, a lane per subsequence -------- */
constexpr uint32_t kS = JXS_SUB, kTile = JXS_TILE;
constexpr uint32_t kRow = kS / 4 + 1;   /* dwords of a row of kS bytes: one more, so that lanes kS bytes apart meet other banks */
constexpr uint32_t kSubGrid = 1024;     /* workgroups that stride over a file's intervals, at most */
static_assert(kTile == kT && kS % 16 == 0 && kS >= 16, "a lane per subsequence, whole 16-byte pieces per row");

/* a tile in LDS as it lies in memory from the 16-byte boundary before it on (`shift` bytes before
 * its first byte), kS bytes per row */
struct JdTile {
    const uint8_t *lds;
    uint32_t shift;
    __device__ __forceinline__ uint32_t byte(uint32_t r) const
    {
        const uint32_t q = r + shift;
        return lds[q + 4u * (q / kS)];
    }
};

__global__ __launch_bounds__(kT) void k_jd_sub(const JdArgs a)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    __shared__ jxd_tab tabs[4];
    __shared__ uint32_t tile_s[(kTile + 2) * kRow];
    __shared__ uint32_t ex_p[kT], ex_cz[kT];
    __shared__ uint32_t wtot[kT / 64];
    __shared__ uint32_t first_bad_s;
    const uint32_t f = blockIdx.y, t = threadIdx.x;
    if (a.st[f]) return;                /* the same for the whole workgroup */
    const jxd_frame *fr = a.frames + f;
    const uint32_t ni = fr->ni;
    if (blockIdx.x >= ni || fr->nblk != a.nblk) return;     /* as k_jd_scan: the stated geometry's blocks fit the slot */
    const uint32_t *src = (const uint32_t *)(a.tabs + 4 * (size_t)f);
    for (uint32_t i = t; i < 4u * sizeof(jxd_tab) / 4u; i += kT) ((uint32_t *)tabs)[i] = src[i];
    jxs_tabs tb;
    jxs_tabs_of(fr, tabs, &tb);
    const size_t len = (size_t)a.len[f];
    const uint8_t *file = a.files + (size_t)f * a.fstride;
    int16_t *coef = a.coef + (size_t)f * a.cstride;
    const uint32_t *mpos = a.mpos + (size_t)f * a.nmcu;
    uint32_t err = 0;
    for (uint32_t iv = blockIdx.x; iv < ni; iv += gridDim.x) {
        const size_t begin = iv ? (size_t)mpos[iv - 1] + 2 : (size_t)fr->scan_off;
        const size_t end = iv + 1 < ni ? (size_t)mpos[iv] : len - 2;
        const uint32_t mcu0 = iv * fr->mpi;
        const uint32_t count = min(fr->mpi, fr->nmcu - mcu0);
        const uint32_t nblocks = count * tb.bpm;
        if (begin > end || end > len) {  /* the same for the whole workgroup */
            err = 1;
            continue;
        }
        /* the interval's blocks zeroed, 16 bytes a lane; the stores are complete before a coefficient's */
        for (uint32_t o = t; o < nblocks * 8u; o += kT) {
            const uint32_t blk = jxs_block_of(fr, mcu0, nblocks, o >> 3);
            const u4 zero = {0u, 0u, 0u, 0u};
            if (blk != JXS_INVALID) ((u4 *)(coef + (size_t)blk * 64))[o & 7u] = zero;
            else err = 1;
        }
        __threadfence();
        __syncthreads();                /* also: the tables are in LDS, the last interval's LDS is free */
        jxs_state carry = {0u, 0u};
        uint32_t carry_blocks = 0, done = 0;
        for (size_t tbeg = begin; tbeg < end; tbeg += (size_t)kS * kTile) {
            const jxs_tile tile = jxs_tile_of(end - tbeg, kS, kTile);
            /* load: 16-byte pieces from the boundary before the tile, whole ones by one load */
            const uint8_t *g0 = file + tbeg;
            const uint32_t shift = (uint32_t)((uintptr_t)g0 & 15u);
            const uint32_t npiece = (shift + tile.lim + 15u) / 16u;
            for (uint32_t k = t; k < npiece; k += kT) {
                const uint32_t q = 16u * k;         /* the piece's place in LDS, before the padding */
                u4 v = {0u, 0u, 0u, 0u};
                if (q >= shift && q + 16u - shift <= tile.lim) {
                    v = *(const u4 *)(g0 + (q - shift));
                } else {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (uint32_t j = 0; j < 16u; j++)
                        if (q + j >= shift && q + j - shift < tile.lim) w[j >> 2] |= (uint32_t)g0[q + j - shift] << (8u * (j & 3u));
                    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
                }
                uint32_t *dst = tile_s + (q / kS) * kRow + (q % kS) / 4u;
                dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
            }
            if (t == 0) first_bad_s = kT;
            __syncthreads();
            const JdTile rd = {(const uint8_t *)tile_s, shift};
            const bool active = t * kS < tile.n;
            const uint32_t sub_end = min((t + 1u) * kS, tile.n);
            jxs_state entry = carry, exit = {JXS_INVALID, 0u};
            uint32_t nblk = 0;
            jxs_nowrite nw;
            if (active) {
                err |= jxs_bare_ff(rd, t * kS, sub_end, tile.end_rel);
                if (t) entry = jxs_guess(rd, t, kS, (uint32_t *)nullptr);
                jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, nw, &exit, &nblk);
            }
            /* rounds: at most kT, and after r of them the first r + 1 exits are the sequential decoder's */
            for (uint32_t round = 0; round < kT; round++) {
                ex_p[t] = exit.p;
                ex_cz[t] = exit.cz;
                __syncthreads();
                int changed = 0;
                if (active && t) {
                    const jxs_state prev = {ex_p[t - 1], ex_cz[t - 1]};
                    if (prev.p != JXS_INVALID && !jxs_same(prev, entry)) {
                        entry = prev;
                        jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, nw, &exit, &nblk);
                        changed = 1;
                    }
                }
                if (!__syncthreads_or(changed)) break;
            }
            /* the first lane whose exit is invalid decoded from a true state, as all before it did */
            if (active && exit.p == JXS_INVALID) atomicMin(&first_bad_s, t);
            uint32_t total;
            const uint32_t ord = carry_blocks + jd_scan(active ? nblk : 0u, wtot, total);
            const uint32_t first_bad = first_bad_s;
            int mine = 0;
            if (active && t <= first_bad && entry.p != JXS_INVALID && ord < nblocks) {
                jxs_store wr;
                wr.open(fr, coef, mcu0, nblocks, ord);
                jxs_state out;
                uint32_t nb;
                jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, wr, &out, &nb);
                if (out.p == JXS_INVALID) {
                    err = 1;
                } else if (wr.ord == nblocks) {             /* this lane completed the interval's last block */
                    mine = 1;
                    if (!jxs_tail_ok(rd, tile.lim, tile.end_rel, out.p)) err = 1;
                }
            }
            const uint32_t last_p = ex_p[kT - 1], last_cz = ex_cz[kT - 1];
            done = (uint32_t)__syncthreads_or(mine);        /* and: the tile's LDS is free */
            if (done || first_bad < kT) break;              /* nothing behind an invalid state is true */
            carry.p = last_p - kS * kTile * 8u;             /* seen from the next tile (if there is one) */
            carry.cz = last_cz;
            carry_blocks += total;
        }
        if (!done) err = 1;
        /* the DC predictors: per component a running sum over the interval's blocks in decode order,
         * 256 at a time, each chunk's sums checked against int16 before the carry moves on */
        __threadfence();
        if (__syncthreads_or((int)err)) {
            err = 1;
            continue;
        }
        for (uint32_t comp = 0; comp < 3u; comp++) {
            const uint32_t per = comp ? 1u : tb.lum, nbk = count * per;
            uint32_t pred = 0;
            for (uint32_t i0 = 0; i0 < nbk; i0 += kT) {
                const uint32_t i = i0 + t;
                uint32_t blk = JXS_INVALID;
                if (i < nbk) {
                    const uint32_t m = i / per, j = comp ? tb.lum + comp - 1u : i - m * per;
                    blk = jxs_block_of(fr, mcu0, nblocks, m * tb.bpm + j);
                }
                const uint32_t d = blk != JXS_INVALID ? (uint32_t)(int32_t)coef[(size_t)blk * 64] : 0u;
                uint32_t sum;
                const int32_t dc = (int32_t)(pred + jd_scan(d, wtot, sum) + d);
                const int out_of_range = dc < -32768 || dc > 32767;
                if (blk != JXS_INVALID && !out_of_range) coef[(size_t)blk * 64] = (int16_t)dc;
                if (__syncthreads_or(out_of_range)) {
                    err = 1;
                    break;
                }
                pred += sum;
            }
            if (err) break;
        }
    }
    if (err) a.status[f] = JPGX_EJFIF_SCAN;
}

struct JdLayout {
    size_t frames, tabs, st, cnt, mpos, total;
};

/* geometry and argument checks shared by the size query and the call; every JPGX_EARG comes before
 * JPGX_EGEOMETRY.  The kernels keep the six words of geometry their arguments always had (with the
 * whole jx_frame as argument and in jxd_frame the decoder was 0.9 - 3.1 % slower):
 * the host fills them from the frame */
int jd_geometry(bool any, int width, int height, int sample_ratio, size_t nframes, size_t file_cap, JdArgs &a, JdLayout &l)
{
    jx_frame f;
    jx_frame_any fa;
    const int why = any ? jx_frame_make_any(width, height, sample_ratio, &fa) : jx_frame_make(width, height, sample_ratio, &f);
    const int rc = jx_frame_rc_decoder(why);
    if (any && !why) f = fa.c;          /* the coded frame: what the coefficients and the MCU counts are of */
    if (rc == JPGX_EARG || !jx_frames_ok(nframes) || file_cap == 0 || file_cap > 0xffffffffull - kChunk)
        return JPGX_EARG;
    if (rc) return rc;
    a.width = (uint32_t)width;
    a.height = (uint32_t)height;
    a.hs = f.hs;
    a.vs = f.vs;
    a.nblk = f.nblk;
    a.nmcu = f.nbc;
    a.nchunk = (uint32_t)((file_cap + kChunk - 1) / kChunk);
    jx_carve ws;
    l.frames = ws.take(nframes * sizeof(jxd_frame));
    l.tabs = ws.take(nframes * 4 * sizeof(jxd_tab));
    l.st = ws.take(nframes * sizeof(int32_t));
    l.cnt = ws.take(nframes * a.nchunk * sizeof(uint32_t));
    l.mpos = ws.take(nframes * (size_t)a.nmcu * sizeof(uint32_t));
    l.total = ws.at;
    return JPGX_OK;
}

/* jpgx_jfif_decode_gpu_ex (any = false) and jpgx_jfif_decode_gpu_any: the checks, their order and the
 * launches are the same but for the geometry's rule and the header kernel's mode */
int jd_decode(bool any, const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
              int height, int sample_ratio, unsigned decode_flags, int16_t *d_coef, size_t coef_frame_stride,
              uint16_t *d_qt, int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    JdArgs a;
    JdLayout l;
    memset(&a, 0, sizeof a);
    if (!d_files || !d_len || !d_coef || !d_status || !d_workspace || ((uintptr_t)d_len & 7) ||
        ((uintptr_t)d_coef & 15) || ((uintptr_t)d_status & 3) || ((uintptr_t)d_qt & 1) || ((uintptr_t)d_workspace & 15) ||
        (decode_flags & ~JPGX_JFIF_DECODE_SUBINTERVAL))
        return JPGX_EARG;
    const int rc = jd_geometry(any, width, height, sample_ratio, nframes, file_stride, a, l);
    if (rc) return rc;
    if (!jx_coef_batch_ok(coef_frame_stride, a.nblk)) return JPGX_EARG;
    if (workspace_bytes < l.total) return JPGX_EWORKSPACE;
    char *ws = (char *)d_workspace;
    a.files = d_files;
    a.fstride = file_stride;
    a.len = (const unsigned long long *)d_len;
    a.coef = d_coef;
    a.cstride = coef_frame_stride;
    a.qt = d_qt;
    a.status = d_status;
    a.frames = (jxd_frame *)(ws + l.frames);
    a.tabs = (jxd_tab *)(ws + l.tabs);
    a.st = (int32_t *)(ws + l.st);
    a.cnt = (uint32_t *)(ws + l.cnt);
    a.mpos = (uint32_t *)(ws + l.mpos);
    hipStream_t s = (hipStream_t)stream;
    const dim3 per_frame((unsigned)nframes), per_chunk(a.nchunk, (unsigned)nframes);
    if (any) hipLaunchKernelGGL(k_jd_header<1>, per_frame, dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(k_jd_header<0>, per_frame, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(k_jd_count, per_chunk, dim3(kT), 0, s, a);
    hipLaunchKernelGGL(k_jd_frame, per_frame, dim3(kT), 0, s, a);
    hipLaunchKernelGGL(k_jd_place, per_chunk, dim3(kT), 0, s, a);
    if (decode_flags & JPGX_JFIF_DECODE_SUBINTERVAL)
        hipLaunchKernelGGL(k_jd_sub, dim3(min(a.nmcu, kSubGrid), (unsigned)nframes), dim3(kT), 0, s, a);
    else
        hipLaunchKernelGGL(k_jd_scan, dim3((a.nmcu + kWave - 1) / kWave, (unsigned)nframes), dim3(kWave), 0, s, a);
    return jx_hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

size_t jpgx_jfif_decode_gpu_workspace_size_ex(int width, int height, int sample_ratio, size_t nframes, size_t file_cap,
                                              unsigned decode_flags)
{
    JdArgs a;
    JdLayout l;
    if (decode_flags & ~JPGX_JFIF_DECODE_SUBINTERVAL) return 0;
    if (jd_geometry(false, width, height, sample_ratio, nframes, file_cap, a, l)) return 0;
    return l.total;
}

size_t jpgx_jfif_decode_gpu_workspace_size(int width, int height, int sample_ratio, size_t nframes, size_t file_cap)
{
    return jpgx_jfif_decode_gpu_workspace_size_ex(width, height, sample_ratio, nframes, file_cap, 0u);
}

int jpgx_jfif_decode_gpu_ex(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
                            int height, int sample_ratio, unsigned decode_flags, int16_t *d_coef,
                            size_t coef_frame_stride, uint16_t *d_qt, int32_t *d_status, void *d_workspace,
                            size_t workspace_bytes, void *stream)
{
    return jd_decode(false, d_files, file_stride, d_len, nframes, width, height, sample_ratio, decode_flags, d_coef,
                     coef_frame_stride, d_qt, d_status, d_workspace, workspace_bytes, stream);
}

size_t jpgx_jfif_decode_gpu_any_workspace_size(int width, int height, int sample_ratio, size_t nframes, size_t file_cap,
                                               unsigned decode_flags)
{
    JdArgs a;
    JdLayout l;
    if (decode_flags & ~JPGX_JFIF_DECODE_SUBINTERVAL) return 0;
    if (jd_geometry(true, width, height, sample_ratio, nframes, file_cap, a, l)) return 0;
    return l.total;
}

int jpgx_jfif_decode_gpu_any(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
                             int height, int sample_ratio, unsigned decode_flags, int16_t *d_coef,
                             size_t coef_frame_stride, uint16_t *d_qt, int32_t *d_status, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    return jd_decode(true, d_files, file_stride, d_len, nframes, width, height, sample_ratio, decode_flags, d_coef,
                     coef_frame_stride, d_qt, d_status, d_workspace, workspace_bytes, stream);
}

int jpgx_jfif_decode_gpu(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
                         int height, int sample_ratio, int16_t *d_coef, size_t coef_frame_stride, uint16_t *d_qt,
                         int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return jpgx_jfif_decode_gpu_ex(d_files, file_stride, d_len, nframes, width, height, sample_ratio, 0u, d_coef,
                                   coef_frame_stride, d_qt, d_status, d_workspace, workspace_bytes, stream);
}

}  /* extern "C" */
