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
 * jpgx_jfif_decode_gpu_gray (one-component files) launches k_jd_header_gray and
 * k_jd_scan_gray or k_jd_sub_gray: the header walk in its one-component mode and the scan kernels' own
 * bodies in their one-component forms (jd_scan_body<1>, jx_jd_sub_body.h): an MCU is a block, DRI
 * counts blocks, one predictor.  k_jd_count, k_jd_frame and k_jd_place do not look at components and
 * serve as they are.  The plain kernels are instruction for instruction what they were before the
 * one-component ones came (profiles/gray_isa_identity.txt), which decided how the bodies are shared.
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

/* k_jd_header for the one-component frame: the walk's GRAY mode, the stated width and height compared
 * (hs = vs = 1 on both sides), and ONE table per frame in d_qt */
__global__ __launch_bounds__(kWave) void k_jd_header_gray(const JdArgs a)
{
    __shared__ int32_t rc_s;
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    jxd_frame *fr = a.frames + f;
    if (t == 0) {
        const unsigned long long len = a.len[f];
        int rc = JPGX_EJFIF_HEADER;
        if (len <= a.fstride) rc = jxd_parse_header<1, 1>(a.files + (size_t)f * a.fstride, (size_t)len, fr, a.tabs + 4 * (size_t)f);
        if (!rc && (fr->width != a.width || fr->height != a.height)) rc = JPGX_EJFIF_HEADER;
        a.st[f] = rc;
        rc_s = rc;
    }
    __syncthreads();                    /* thread 0's stores to *fr are visible to the workgroup */
    if (a.qt)
        for (uint32_t i = t; i < 64u; i += kWave) a.qt[(size_t)f * 64 + i] = rc_s ? (uint16_t)0 : fr->qt[0][i];
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

template <int GRAY>
__device__ __forceinline__ void jd_scan_body(const JdArgs &a)
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
    const int rc = GRAY ? jxd_decode_interval_gray(a.files + (size_t)f * a.fstride, len, begin, end, fr, tabs, mcu0,
                                                   count, a.coef + (size_t)f * a.cstride)
                        : jxd_decode_interval(a.files + (size_t)f * a.fstride, len, begin, end, fr, tabs, mcu0, count,
                                              a.coef + (size_t)f * a.cstride);
    if (rc) a.status[f] = JPGX_EJFIF_SCAN;
}

__global__ __launch_bounds__(kWave) void k_jd_scan(const JdArgs a) { jd_scan_body<0>(a); }

__global__ __launch_bounds__(kWave) void k_jd_scan_gray(const JdArgs a) { jd_scan_body<1>(a); }

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

/* the kernel's body, once per frame family (jx_jd_sub_body.h says why it is included and no template) */
#define JD_SUB_KERNEL k_jd_sub
#define JD_SUB_TABS_OF jxs_tabs_of
#define JD_SUB_BLOCK_OF jxs_block_of
#define JD_SUB_STORE jxs_store
#define JD_SUB_COMPONENTS 3u
#include "jx_jd_sub_body.h"
#undef JD_SUB_KERNEL
#undef JD_SUB_TABS_OF
#undef JD_SUB_BLOCK_OF
#undef JD_SUB_STORE
#undef JD_SUB_COMPONENTS

/* the one-component frame: jx_jfif_sub.h's one-component block walk, one DC predictor */
#define JD_SUB_KERNEL k_jd_sub_gray
#define JD_SUB_TABS_OF jxs_tabs_of_gray
#define JD_SUB_BLOCK_OF jxs_block_of_gray
#define JD_SUB_STORE jxs_store_t<1>
#define JD_SUB_COMPONENTS 1u
#include "jx_jd_sub_body.h"
#undef JD_SUB_KERNEL
#undef JD_SUB_TABS_OF
#undef JD_SUB_BLOCK_OF
#undef JD_SUB_STORE
#undef JD_SUB_COMPONENTS

struct JdLayout {
    size_t frames, tabs, st, cnt, mpos, total;
};

/* geometry and argument checks shared by the size query and the call; every JPGX_EARG comes before
 * JPGX_EGEOMETRY.  The kernels keep the six words of geometry their arguments always had (with the
 * whole jx_frame as argument and in jxd_frame the decoder was 0.9 - 3.1 % slower):
 * the host fills them from the frame */
enum { kPlain, kAny, kGray };           /* the entry points' families */

int jd_geometry(int mode, int width, int height, int sample_ratio, size_t nframes, size_t file_cap, JdArgs &a, JdLayout &l)
{
    jx_frame f;
    jx_frame_any fa;
    jx_frame_gray fg;
    const int why = mode == kGray ? jx_frame_make_gray(width, height, &fg)
                    : mode == kAny ? jx_frame_make_any(width, height, sample_ratio, &fa)
                                   : jx_frame_make(width, height, sample_ratio, &f);
    const int rc = jx_frame_rc_decoder(why);
    if (mode == kAny && !why) f = fa.c; /* the coded frame: what the coefficients and the MCU counts are of */
    if (mode == kGray && !why) {        /* one block per MCU: the words the kernels compare and size by */
        f.hs = f.vs = 1;
        f.nblk = f.nbc = fg.nb;
    }
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

/* jpgx_jfif_decode_gpu_ex (kPlain), jpgx_jfif_decode_gpu_any and jpgx_jfif_decode_gpu_gray: the checks,
 * their order and the launches are the same but for the geometry's rule, the header kernel's mode and,
 * for kGray, the scan kernel's */
int jd_decode(int mode, const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
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
    const int rc = jd_geometry(mode, width, height, sample_ratio, nframes, file_stride, a, l);
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
    if (mode == kGray) hipLaunchKernelGGL(k_jd_header_gray, per_frame, dim3(kWave), 0, s, a);
    else if (mode == kAny) hipLaunchKernelGGL(k_jd_header<1>, per_frame, dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(k_jd_header<0>, per_frame, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(k_jd_count, per_chunk, dim3(kT), 0, s, a);
    hipLaunchKernelGGL(k_jd_frame, per_frame, dim3(kT), 0, s, a);
    hipLaunchKernelGGL(k_jd_place, per_chunk, dim3(kT), 0, s, a);
    const dim3 sub_grid(min(a.nmcu, kSubGrid), (unsigned)nframes), scan_grid((a.nmcu + kWave - 1) / kWave, (unsigned)nframes);
    if (decode_flags & JPGX_JFIF_DECODE_SUBINTERVAL) {
        if (mode == kGray) hipLaunchKernelGGL(k_jd_sub_gray, sub_grid, dim3(kT), 0, s, a);
        else hipLaunchKernelGGL(k_jd_sub, sub_grid, dim3(kT), 0, s, a);
    } else {
        if (mode == kGray) hipLaunchKernelGGL(k_jd_scan_gray, scan_grid, dim3(kWave), 0, s, a);
        else hipLaunchKernelGGL(k_jd_scan, scan_grid, dim3(kWave), 0, s, a);
    }
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
    if (jd_geometry(kPlain, width, height, sample_ratio, nframes, file_cap, a, l)) return 0;
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
    return jd_decode(kPlain, d_files, file_stride, d_len, nframes, width, height, sample_ratio, decode_flags, d_coef,
                     coef_frame_stride, d_qt, d_status, d_workspace, workspace_bytes, stream);
}

size_t jpgx_jfif_decode_gpu_any_workspace_size(int width, int height, int sample_ratio, size_t nframes, size_t file_cap,
                                               unsigned decode_flags)
{
    JdArgs a;
    JdLayout l;
    if (decode_flags & ~JPGX_JFIF_DECODE_SUBINTERVAL) return 0;
    if (jd_geometry(kAny, width, height, sample_ratio, nframes, file_cap, a, l)) return 0;
    return l.total;
}

int jpgx_jfif_decode_gpu_any(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
                             int height, int sample_ratio, unsigned decode_flags, int16_t *d_coef,
                             size_t coef_frame_stride, uint16_t *d_qt, int32_t *d_status, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    return jd_decode(kAny, d_files, file_stride, d_len, nframes, width, height, sample_ratio, decode_flags, d_coef,
                     coef_frame_stride, d_qt, d_status, d_workspace, workspace_bytes, stream);
}

size_t jpgx_jfif_decode_gpu_gray_workspace_size(int width, int height, size_t nframes, size_t file_cap, unsigned decode_flags)
{
    JdArgs a;
    JdLayout l;
    if (decode_flags & ~JPGX_JFIF_DECODE_SUBINTERVAL) return 0;
    if (jd_geometry(kGray, width, height, 0, nframes, file_cap, a, l)) return 0;
    return l.total;
}

int jpgx_jfif_decode_gpu_gray(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len, size_t nframes, int width,
                              int height, unsigned decode_flags, int16_t *d_coef, size_t coef_frame_stride, uint16_t *d_qt,
                              int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return jd_decode(kGray, d_files, file_stride, d_len, nframes, width, height, 0, decode_flags, d_coef,
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
