/*
 * jpgx_pixels.hip -- coefficients to pixels on the device: jpgx_pixels_gpu.
 * Dequantisation, the fixed-point inverse DCT, the chroma upsampling and the colour conversion of
 * libjpeg's default decoder; the arithmetic is jx_idct.h's, the source the host twin
 * (jpgx_pixels_host.cpp) compiles.  Integer VALU only.
 *
 *   k_px444      4:4:4, fused: coefficients in, RGB out
 *   k_px_chroma  4:2:2 / 4:2:0: Cb and Cr to uint8 sample planes in the workspace
 *   k_px_sub     4:2:2 / 4:2:0: Y transformed, the chroma samples read with their clamped halo
 *                from the workspace, upsampled, converted
 *
 * One-wave workgroups.  A wave takes runs of 8 consecutive blocks of a block row: a block is 128
 * contiguous bytes, so the run is one 16-byte load per lane and channel, lane = (block, 8 zig-zag
 * positions).  The lane dequantises its 8 coefficients (its 8 table entries per table stay in its
 * registers for all its runs) and scatters them to their natural places in LDS; pass 1 runs with
 * lane = (block, column) in place, pass 2 with lane = (block, row), which then holds 8 samples of
 * every channel, converts them and stages its 24 bytes in LDS, from where each pixel row of the
 * run (192 contiguous bytes) leaves in 8-byte stores.
 *
 * LDS image of a channel (dwords): A(b, r, c) = 64 b + 8 (r ^ (b & 3)) + (c ^ 2 (b & 2)).
 *   pass 1, ds_read_b32 / ds_write_b32 (32 banks, 32-lane groups; a group is 4 blocks x 8 columns of
 *     one r): bank = 8 ((r ^ b) & 3) + (c ^ ...): the 4 blocks take the 4 different r ^ b, the 8
 *     columns the 8 different c: no conflict;
 *   pass 2, 2 x ds_read_b128 (64 banks, the 16-lane groups {0-3, 12-15, 20-27} ... of the hardware: two
 *     blocks' rows 0-3 and two blocks' rows 4-7, whose r ^ (b & 3) coincide pairwise): the pair
 *     differs in b & 2 and so reads opposite halves of the 8-dword row: no conflict.
 * Every global index comes from the checked geometry, blockIdx and the lane: the data only ever
 * become values.  No global state, no memset; capturable.
 *
 * jpgx_pixels_gpu_any (a frame of any width and height) launches the instantiations ANY = 1 of
 * k_px444 and k_px_sub, the plain call ANY = 0; k_px_chroma serves both.
 *
 * jpgx_pixels_gpu_gray (a one-component frame, Y [nb][64] and one table) launches k_px_gray<CHANNELS>:
 * px_transform<1> on the same runs and the same LDS image, then 1 byte per pixel through a staging
 * buffer of its own (px_store_gray1) or 3 equal bytes through px_store<1> with Cb = Cr = 128, for
 * which jxi_rgb returns the sample three times.  No workspace.
 *
 * jpgx_pixels_gpu_scaled / jpgx_pixels_gpu_gray_scaled (1/2, 1/4, 1/8 of the size) launch
 * k_pxs, k_pxs_chroma and k_pxs_dc, which stand below the kernels above and share their runs, their LDS
 * image and their lane constants; scale_denom 1 is the _any / _gray call.
 */
#include <stdint.h>
#include <string.h>

#include "jx_frame.h"
#include "jx_hip.h"
#include "jx_idct.h"

namespace {

constexpr int kWave = 64;
constexpr uint32_t kRunsPerWave = 4;    /* a wave takes this many consecutive runs: its tables and addresses serve them
                                           all, and a pixel row's 4 x 192 bytes are whole 128-byte lines from one wave */
constexpr uint32_t kStageRow = 208;     /* bytes between the staged pixel rows of a run: 192 + 16, which
                                           puts the 8 rows' first dwords on 8 different groups of 4 banks */

__constant__ uint8_t kZZ[64] = JXI_ZZ_INIT;

/* The kernels' view of the frame (jx_frame.h): the eight words they read, in the order their
 * arguments had when they were measured.  With the whole jx_frame by value two of the 4:2:x figures
 * lay 0.2 - 0.4 % above the parent's range, so the host fills these from the frame. */
struct PxGeom {
    uint32_t bw, bh, cbw, cbh, hs, vs, nb, nbc;
};

struct PxArgs {
    const int16_t *coef;
    unsigned long long cstride;         /* int16 elements between frames */
    const uint16_t *qt;
    unsigned long long qstride;         /* uint16 elements between the frames' table pairs, 0: one pair */
    const int32_t *status;              /* NULL, or [nframes]: nonzero = skip the frame */
    uint8_t *rgb;
    unsigned long long pitch, ostride;
    uint8_t *planes;                    /* workspace [nframes][2][8 cbh][8 cbw] (4:2:x) */
    PxGeom g;
};

/* the _any entry points' arguments (jpgx_pixels_gpu_any): g is the coded frame's, and with it come the
 * visible frame and a chroma plane's real extent (jx_frame_any).  A type of its own, so that the plain
 * kernels' arguments stay what they were */
struct PxArgsAny : PxArgs {
    uint32_t w, h, wc, hc;
};

/* jpgx_pixels_gpu_gray's: g.bw x g.bh blocks, g.nb of them, no chroma; the visible frame */
struct PxArgsGray : PxArgs {
    uint32_t w, h;
};

template <int ANY>
struct PxA {
    typedef PxArgs type;
};
template <>
struct PxA<1> {
    typedef PxArgsAny type;
};

union V4 {
    uint4 v;
    uint16_t h[8];
};

/* what a lane keeps for all its runs */
struct Lane {
    uint32_t b, j;                      /* lane = (block of the run, 8 zig-zag positions / column / row) */
    uint32_t at[8];                     /* dword index in a channel's image of zig-zag position 8 j + i */
    V4 q[2];                            /* its 8 entries of the two tables */
    bool fast;                          /* the same for the whole wave: no entry of the frame's tables above 63, so
                                           every |coefficient * entry| <= 2^15 * 63 < 2^21 (jxi_idct8's M24) */
};

__device__ __forceinline__ uint32_t px_at(uint32_t b, uint32_t r, uint32_t c)
{
    return 64u * b + 8u * (r ^ (b & 3u)) + (c ^ ((b & 2u) << 1));
}

__device__ __forceinline__ void px_lane(const PxArgs &a, uint32_t f, Lane &L)
{
    L.b = threadIdx.x >> 3;
    L.j = threadIdx.x & 7u;
    const uint16_t *qt = a.qt + (size_t)f * a.qstride;
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int i = 0; i < 8; i++) L.q[t].h[i] = qt[t * 64 + L.j * 8 + i];
    uint32_t qor = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) qor |= (uint32_t)L.q[0].h[i] | (uint32_t)L.q[1].h[i];
    L.fast = __all(qor < 64u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t nat = kZZ[L.j * 8 + i];
        L.at[i] = px_at(L.b, nat >> 3, nat & 7u);
    }
}

/* px_lane for the one-component frame: a.qt has ONE table per frame, a.qstride apart, which takes
 * both places (only the first is used) */
__device__ __forceinline__ void px_lane_gray(const PxArgs &a, uint32_t f, Lane &L)
{
    L.b = threadIdx.x >> 3;
    L.j = threadIdx.x & 7u;
    const uint16_t *qt = a.qt + (size_t)f * a.qstride;
    uint32_t qor = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        L.q[0].h[i] = L.q[1].h[i] = qt[L.j * 8 + i];
        qor |= (uint32_t)L.q[0].h[i];
    }
    L.fast = __all(qor < 64u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t nat = kZZ[L.j * 8 + i];
        L.at[i] = px_at(L.b, nat >> 3, nat & 7u);
    }
}

/* NCH channels of a run of n <= 8 blocks: src[ch] points at the run's first block.  Leaves
 * s[ch][0..7], the 0..255 samples of row L.j of block L.b.  img: NCH x 512 dwords of LDS. */
template <int NCH>
__device__ __forceinline__ void px_transform(const int16_t *const (&src)[NCH], const int (&tab)[NCH], uint32_t n,
                                             const Lane &L, uint32_t *img, uint32_t (&s)[NCH][8])
{
    const bool live = L.b < n;
    V4 in[NCH];
    if (live) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) in[ch].v = *(const uint4 *)(src[ch] + (size_t)threadIdx.x * 8);
#pragma unroll
        for (int ch = 0; ch < NCH; ch++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                img[ch * 512 + L.at[i]] = jxi_dequant((int16_t)in[ch].h[i], L.q[tab[ch]].h[i]);
    }
    /* the 24-bit multiplier serves pass 1 where the tables are small (quality 75 and better) or, with
     * larger entries, where every coefficient of the run is: every file that was coded from an image.
     * Either way the same for the whole wave. */
    bool small = L.fast;
    if (!small) {
        uint32_t big = 0;               /* the OR of d + 2^15: below 2^16 while every d of this lane is JXI_SMALL */
        if (live) {
#pragma unroll
            for (int ch = 0; ch < NCH; ch++)
#pragma unroll
                for (int i = 0; i < 8; i++) big |= jxi_dequant((int16_t)in[ch].h[i], L.q[tab[ch]].h[i]) + 0x8000u;
        }
        small = __all(big < 0x10000u);
    }
    __syncthreads();
    /* pass 1: lane = (block, column j), in place */
    const uint32_t col = px_at(L.b, 0, L.j);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        uint32_t v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = img[ch * 512 + (col ^ (8u * r))];
        if (small) jxi_idct8<1>(v, JXI_PASS1_SHIFT);
        else jxi_idct8<0>(v, JXI_PASS1_SHIFT);
#pragma unroll
        for (int r = 0; r < 8; r++) img[ch * 512 + (col ^ (8u * r))] = v[r];
    }
    __syncthreads();
    /* pass 2: lane = (block, row j); the halves of its row are swapped where b & 2 */
    const uint32_t row = px_at(L.b, L.j, 0);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        const uint4 lo = *(const uint4 *)(img + ch * 512 + row), hi = *(const uint4 *)(img + ch * 512 + (row ^ 4u));
        uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        jxi_idct8<1>(v, JXI_PASS2_SHIFT);       /* inputs inside +-2^20 whatever the data (jx_idct.h) */
#pragma unroll
        for (int c = 0; c < 8; c++) s[ch][c] = jxi_range(v[c]);
    }
    __syncthreads();                    /* the image is free: the staging buffer lies in it */
}

/* lane (b, row j) has the 8 pixels of its row: 24 bytes to the staging buffer, then pixel row r of
 * the run, 24 n bytes at out + r * pitch, leaves in 8-byte pieces; lanes beyond the run store nothing.
 * ANY: only rows r < rows and bytes [0, nbytes) of a row are the frame's (both the same for the whole
 * wave; 8 and 24 n everywhere but in a row's last run and the last block row): no row beyond, and
 * where the bytes end inside a piece, lane r writes that piece of row r as 4 + 2 + 1 bytes */
template <int ANY>
__device__ __forceinline__ void px_store(const uint32_t (&y)[8], const uint32_t (&cb)[8], const uint32_t (&cr)[8],
                                         uint32_t n, const Lane &L, uint8_t *stage, uint8_t *out, size_t pitch,
                                         uint32_t rows = 8u, uint32_t nbytes = 192u)
{
    uint32_t px[24];
#pragma unroll
    for (int x = 0; x < 8; x++) jxi_rgb(y[x], cb[x], cr[x], &px[3 * x], &px[3 * x + 1], &px[3 * x + 2]);
    uint2 *dst = (uint2 *)(stage + L.j * kStageRow + L.b * 24u);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint2 w;
        w.x = px[8 * k] | px[8 * k + 1] << 8 | px[8 * k + 2] << 16 | px[8 * k + 3] << 24;
        w.y = px[8 * k + 4] | px[8 * k + 5] << 8 | px[8 * k + 6] << 16 | px[8 * k + 7] << 24;
        dst[k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t piece = threadIdx.x + 64u * k, r = piece / 24u, c = piece % 24u;
        const bool whole = ANY ? r < rows && c * 8u + 8u <= nbytes : c < 3u * n;     /* nbytes <= 24 n */
        if (whole) *(uint2 *)(out + (size_t)r * pitch + c * 8u) = *(const uint2 *)(stage + r * kStageRow + c * 8u);
    }
    if (ANY && (nbytes & 7u)) {         /* the same for the whole wave: lane r finishes row r */
        const uint32_t r = threadIdx.x, at = nbytes & ~7u;
        if (r < rows) {
            const uint2 w = *(const uint2 *)(stage + r * kStageRow + at);
            uint8_t *tail = out + (size_t)r * pitch + at;           /* 8-byte aligned */
            uint32_t v = w.x;
            if (nbytes & 4u) {
                *(uint32_t *)tail = v;
                tail += 4;
                v = w.y;
            }
            if (nbytes & 2u) {
                *(uint16_t *)tail = (uint16_t)v;
                tail += 2;
                v >>= 16;
            }
            if (nbytes & 1u) *tail = (uint8_t)v;
        }
    }
    __syncthreads();                    /* the staging buffer is free for the next run's image */
}

/* One byte per pixel: lane (b, row j) has the 8 samples of its row, 8 bytes of pixel row j of the run.
 * Stored from there, consecutive lanes would write to 8 different rows; through the staging buffer
 * lane t writes piece t & 7 of row t >> 3, so 8 consecutive lanes write 64 contiguous bytes, and the
 * 4 runs of a wave whole 128-byte lines.  kStageRowGray = 80 bytes between the staged rows: the 32
 * lanes of a ds_write_b64 group (4 blocks x 8 rows) then take every one of the 32 banks exactly twice,
 * the fewest 64 dwords can; the ds_read_b64 (64 banks) meets 12 of them twice, where 64 bytes between
 * rows would read without a conflict and write four lanes to a bank.  rows, nbytes: as px_store<1>'s,
 * nbytes <= 8 n; the row's last partial piece leaves as 4 + 2 + 1 bytes from lane r */
constexpr uint32_t kStageRowGray = 80;

__device__ __forceinline__ void px_store_gray1(const uint32_t (&y)[8], const Lane &L, uint8_t *stage, uint8_t *out,
                                               size_t pitch, uint32_t rows, uint32_t nbytes)
{
    uint2 w;
    w.x = y[0] | y[1] << 8 | y[2] << 16 | y[3] << 24;
    w.y = y[4] | y[5] << 8 | y[6] << 16 | y[7] << 24;
    *(uint2 *)(stage + L.j * kStageRowGray + L.b * 8u) = w;
    __syncthreads();
    {
        const uint32_t r = threadIdx.x >> 3, c = threadIdx.x & 7u;
        if (r < rows && c * 8u + 8u <= nbytes)
            *(uint2 *)(out + (size_t)r * pitch + c * 8u) = *(const uint2 *)(stage + r * kStageRowGray + c * 8u);
    }
    if (nbytes & 7u) {                  /* the same for the whole wave: lane r finishes row r */
        const uint32_t r = threadIdx.x, at = nbytes & ~7u;
        if (r < rows) {
            const uint2 v2 = *(const uint2 *)(stage + r * kStageRowGray + at);
            uint8_t *tail = out + (size_t)r * pitch + at;           /* 8-byte aligned */
            uint32_t v = v2.x;
            if (nbytes & 4u) {
                *(uint32_t *)tail = v;
                tail += 4;
                v = v2.y;
            }
            if (nbytes & 2u) {
                *(uint16_t *)tail = (uint16_t)v;
                tail += 2;
                v >>= 16;
            }
            if (nbytes & 1u) *tail = (uint8_t)v;
        }
    }
    __syncthreads();                    /* the staging buffer is free for the next run's image */
}

__device__ __forceinline__ bool px_skip(const PxArgs &a, uint32_t f) { return a.status && a.status[f] != 0; }

/* five waves per SIMD: 82 VGPRs without a spill, where the allocator left to itself takes 99 (four waves) */
template <int ANY>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(5))) void k_px444(const typename PxA<ANY>::type a)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[3 * 512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;
    if (px_skip(a, f)) return;          /* the same for the whole workgroup */
    Lane L;
    px_lane(a, f, L);
    const uint32_t nruns = (a.g.bw + 7u) / 8u;
    const int16_t *frame = a.coef + (size_t)f * a.cstride;
    uint8_t *out = a.rgb + (size_t)f * a.ostride + (size_t)by * 8u * a.pitch;
    const int tab[3] = {0, 1, 1};
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.bw - run * 8u);
        const size_t blk = (size_t)by * a.g.bw + (size_t)run * 8u;
        const int16_t *const src[3] = {frame + blk * 64, frame + ((size_t)a.g.nb + blk) * 64,
                                       frame + (2 * (size_t)a.g.nb + blk) * 64};
        uint32_t s[3][8];
        px_transform<3>(src, tab, n, L, img, s);
        if constexpr (ANY) {            /* the grid has the visible block rows only: by * 8 < h, run * 64 < w */
            px_store<1>(s[0], s[1], s[2], n, L, (uint8_t *)img, out + (size_t)run * 192u, (size_t)a.pitch,
                        min(8u, a.h - by * 8u), min(24u * n, 3u * a.w - run * 192u));
        } else {
            px_store<0>(s[0], s[1], s[2], n, L, (uint8_t *)img, out + (size_t)run * 192u, (size_t)a.pitch);
        }
    }
}

__global__ __launch_bounds__(kWave) void k_px_chroma(const PxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[2 * 512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;     /* a chroma block row */
    if (px_skip(a, f)) return;
    Lane L;
    px_lane(a, f, L);
    const uint32_t nruns = (a.g.cbw + 7u) / 8u;
    const size_t wc = (size_t)a.g.cbw * 8u, plane = wc * a.g.cbh * 8u;
    const int16_t *frame = a.coef + (size_t)f * a.cstride + (size_t)a.g.nb * 64;
    uint8_t *out = a.planes + (size_t)f * 2u * plane + ((size_t)by * 8u + L.j) * wc;
    const int tab[2] = {1, 1};
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.cbw - run * 8u);
        const size_t blk = (size_t)by * a.g.cbw + (size_t)run * 8u;
        const int16_t *const src[2] = {frame + blk * 64, frame + ((size_t)a.g.nbc + blk) * 64};
        uint32_t s[2][8];
        px_transform<2>(src, tab, n, L, img, s);
        if (L.b < n) {
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                uint2 w;
                w.x = s[ch][0] | s[ch][1] << 8 | s[ch][2] << 16 | s[ch][3] << 24;
                w.y = s[ch][4] | s[ch][5] << 8 | s[ch][6] << 16 | s[ch][7] << 24;
                *(uint2 *)(out + ch * plane + (size_t)run * 64u + L.b * 8u) = w;
            }
        }
    }
}

/* samples i0 - 1 .. i0 + 4 of a plane row, the two outer indices clamped to the row */
__device__ __forceinline__ void px_row6(const uint8_t *row, uint32_t i0, uint32_t wc, uint32_t (&p)[6])
{
    const uint32_t w = *(const uint32_t *)(row + i0);   /* i0 is a multiple of 4, as are wc and the plane's base */
    p[0] = row[i0 ? i0 - 1u : 0u];
    p[1] = w & 255u;
    p[2] = w >> 8 & 255u;
    p[3] = w >> 16 & 255u;
    p[4] = w >> 24;
    p[5] = row[i0 + 4u < wc ? i0 + 4u : wc - 1u];
}

/* px_row6 where the row really ends at wc, before the plane's pitch (the last run of a row): every
 * index clamps to wc - 1, those inside the dword included.  p[5] is clamped already */
__device__ __forceinline__ void px_row6_edge(const uint8_t *row, uint32_t i0, uint32_t wc, uint32_t (&p)[6])
{
    const uint32_t last = row[wc - 1u];
#pragma unroll
    for (uint32_t k = 0; k < 5u; k++)
        if (i0 + k > wc) p[k] = last;   /* sample i0 + k - 1 is beyond wc - 1 */
}

/* ANY: the planes keep the coded frame's pitch and rows; the clamps are at the chroma's real extent
 * a.wc x a.hc, and a row of two samples or fewer is replicated, not filtered */
template <int V2, int ANY>
__global__ __launch_bounds__(kWave) void k_px_sub(const typename PxA<ANY>::type a)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;     /* a Y block row */
    if (px_skip(a, f)) return;
    Lane L;
    px_lane(a, f, L);
    const uint32_t nruns = (a.g.bw + 7u) / 8u;
    const uint32_t pc = a.g.cbw * 8u;   /* bytes between a plane's rows */
    uint32_t wc = pc, hc = a.g.cbh * 8u;
    const size_t plane = (size_t)pc * hc;
    if constexpr (ANY) wc = a.wc, hc = a.hc;
    const int16_t *frame = a.coef + (size_t)f * a.cstride;
    const uint8_t *planes = a.planes + (size_t)f * 2u * plane;
    uint8_t *out = a.rgb + (size_t)f * a.ostride + (size_t)by * 8u * a.pitch;
    /* the chroma rows of this lane's pixel row: the near one and, for 4:2:0, the far one, clamped */
    const uint32_t y = by * 8u + L.j;
    const uint32_t cy = V2 ? y >> 1 : y;
    const uint32_t far = !V2 ? cy : (y & 1u) ? (cy + 1u < hc ? cy + 1u : cy) : (cy ? cy - 1u : 0u);
    const int tab[1] = {0};
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.bw - run * 8u);
        const int16_t *const src[1] = {frame + ((size_t)by * a.g.bw + (size_t)run * 8u) * 64};
        uint32_t s[1][8], up[2][8];
        px_transform<1>(src, tab, n, L, img, s);
        const uint32_t i0 = run * 32u + L.b * 4u;       /* the lane's 4 chroma samples; below pc while L.b < n */
        /* the same for the whole wave: this run's samples or their right neighbour lie beyond wc - 1 */
        const bool edge = ANY && run * 32u + 32u >= wc;
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            uint32_t p[6] = {0, 0, 0, 0, 0, 0};
            if (L.b < n) {
                /* both rows' loads first, as in the plain kernel; the edge's corrections after them */
                uint32_t q[6];
                px_row6(planes + ch * plane + (size_t)cy * pc, i0, wc, p);
                if (V2) px_row6(planes + ch * plane + (size_t)far * pc, i0, wc, q);
                if (edge) {
                    px_row6_edge(planes + ch * plane + (size_t)cy * pc, i0, wc, p);
                    if (V2) px_row6_edge(planes + ch * plane + (size_t)far * pc, i0, wc, q);
                }
                if (V2 && !(ANY && wc <= 2u)) {
#pragma unroll
                    for (int i = 0; i < 6; i++) p[i] = jxi_vsum(p[i], q[i]);
                }
            }
            if (ANY && wc <= 2u) {      /* replication: the near row's sample for both pixels */
#pragma unroll
                for (int i = 0; i < 4; i++) up[ch][2 * i] = up[ch][2 * i + 1] = p[i + 1];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    up[ch][2 * i] = jxi_up_even(p[i + 1], p[i], V2);
                    up[ch][2 * i + 1] = jxi_up_odd(p[i + 1], p[i + 2], V2);
                }
            }
        }
        if constexpr (ANY) {            /* the grid has the visible block rows only: by * 8 < h, run * 64 < w */
            px_store<1>(s[0], up[0], up[1], n, L, (uint8_t *)img, out + (size_t)run * 192u, (size_t)a.pitch,
                        min(8u, a.h - by * 8u), min(24u * n, 3u * a.w - run * 192u));
        } else {
            px_store<0>(s[0], up[0], up[1], n, L, (uint8_t *)img, out + (size_t)run * 192u, (size_t)a.pitch);
        }
    }
}

/* The one-component frame: Y alone, CHANNELS (1 or 3) equal bytes per pixel.  The grid has the block
 * rows that hold a visible pixel row: by * 8 < h, and run * 64 < w for every run of a row */
template <int CHANNELS>
__global__ __launch_bounds__(kWave) void k_px_gray(const PxArgsGray a)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;
    if (px_skip(a, f)) return;          /* the same for the whole workgroup */
    Lane L;
    px_lane_gray(a, f, L);
    const uint32_t nruns = (a.g.bw + 7u) / 8u;
    const int16_t *frame = a.coef + (size_t)f * a.cstride;
    uint8_t *out = a.rgb + (size_t)f * a.ostride + (size_t)by * 8u * a.pitch;
    const uint32_t rows = min(8u, a.h - by * 8u);
    const int tab[1] = {0};
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.bw - run * 8u);
        const int16_t *const src[1] = {frame + ((size_t)by * a.g.bw + (size_t)run * 8u) * 64};
        uint32_t s[1][8];
        px_transform<1>(src, tab, n, L, img, s);
        if constexpr (CHANNELS == 1) {
            px_store_gray1(s[0], L, (uint8_t *)img, out + (size_t)run * 64u, (size_t)a.pitch, rows,
                           min(8u * n, a.w - run * 64u));
        } else {
            const uint32_t c128[8] = {128u, 128u, 128u, 128u, 128u, 128u, 128u, 128u};
            px_store<1>(s[0], c128, c128, n, L, (uint8_t *)img, out + (size_t)run * 192u, (size_t)a.pitch, rows,
                        min(24u * n, 3u * a.w - run * 192u));
        }
    }
}

/* ---- 1/2, 1/4 and 1/8 of the size ------------------------------------------------
 *   k_pxs<N, MODE>     a luma block to N x N samples, N = 4 or 2, on the runs and the LDS image above:
 *                      one-component frames (1 or 3 bytes per pixel) and 4:4:4 fused, 4:2:x with the
 *                      chroma samples read from the workspace (as they are, replicated 2 x 1 or through
 *                      the triangle filter: a.up)
 *   k_pxs_chroma<N>    Cb and Cr to N x N samples per block in the workspace (8 x 8: k_px_chroma)
 *   k_pxs_dc<MODE>     1/8 of the size: lane = block, one DC per channel, one pixel per lane */
struct PxArgsScaled : PxArgs {
    uint32_t ow, oh;                    /* the output */
    uint32_t wc;                        /* a chroma row's real samples: the triangle filter clamps there */
    uint32_t pc;                        /* bytes between a chroma plane's rows in the workspace */
    uint32_t up;                        /* the chroma samples of a pixel row: 0 as they are, 1 replicated 2 x 1,
                                           2 through the h2v1 triangle filter */
    unsigned long long plane;           /* bytes of a chroma plane */
};

/* px_transform at N = 4 or 2: lane (b, row j < N) gets s[ch][0..N-1], the other lanes zeros.  Pass 1
 * takes the 24-bit multiplier under px_transform's rule (every input inside +-2^21 then), pass 2 always */
template <int NCH, int N>
__device__ __forceinline__ void pxs_transform(const int16_t *const (&src)[NCH], const int (&tab)[NCH], uint32_t n,
                                              const Lane &L, uint32_t *img, uint32_t (&s)[NCH][N])
{
    const bool live = L.b < n;
    V4 in[NCH];
    if (live) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) in[ch].v = *(const uint4 *)(src[ch] + (size_t)threadIdx.x * 8);
#pragma unroll
        for (int ch = 0; ch < NCH; ch++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                img[ch * 512 + L.at[i]] = jxi_dequant((int16_t)in[ch].h[i], L.q[tab[ch]].h[i]);
    }
    bool small = L.fast;
    if (!small) {
        uint32_t big = 0;
        if (live) {
#pragma unroll
            for (int ch = 0; ch < NCH; ch++)
#pragma unroll
                for (int i = 0; i < 8; i++) big |= jxi_dequant((int16_t)in[ch].h[i], L.q[tab[ch]].h[i]) + 0x8000u;
        }
        small = __all(big < 0x10000u);
    }
    __syncthreads();
    /* pass 1: lane = (block, column j), rows 0 .. N - 1 in place */
    const uint32_t col = px_at(L.b, 0, L.j);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        uint32_t v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = img[ch * 512 + (col ^ (8u * r))];
        if (small) jxi_idctn<N, 1>(v, 1);
        else jxi_idctn<N, 0>(v, 1);
#pragma unroll
        for (int r = 0; r < N; r++) img[ch * 512 + (col ^ (8u * r))] = v[r];
    }
    __syncthreads();
    /* pass 2: lane = (block, row j < N) */
    const uint32_t row = px_at(L.b, L.j & (uint32_t)(N - 1), 0);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        const uint4 lo = *(const uint4 *)(img + ch * 512 + row), hi = *(const uint4 *)(img + ch * 512 + (row ^ 4u));
        uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        jxi_idctn<N, 1>(v, 2);
#pragma unroll
        for (int c = 0; c < N; c++) s[ch][c] = L.j < (uint32_t)N ? jxi_range(v[c]) : 0u;
    }
    __syncthreads();                    /* the image is free: the staging buffer lies in it */
}

/* lane (b, row j < N) has the NB = bytes per pixel x N bytes of its piece of pixel row j of the run; a
 * row of the run is 8 NB bytes, NB pieces of 8 bytes, and N rows are at most 48 pieces: lane t stores
 * piece t % NB of row t / NB.  rows, nbytes and the row's last partial piece: as px_store<1>'s */
template <int NB, int N>
__device__ __forceinline__ void pxs_store(const uint32_t (&px)[NB], const Lane &L, uint8_t *stage, uint8_t *out,
                                          size_t pitch, uint32_t rows, uint32_t nbytes)
{
    constexpr uint32_t kRow = 8u * NB + 16u;    /* bytes between the staged rows */
    if (L.j < (uint32_t)N) {
        uint8_t *dst = stage + L.j * kRow + L.b * (uint32_t)NB;
        if constexpr (NB % 4 == 0) {
#pragma unroll
            for (int k = 0; k < NB / 4; k++)
                ((uint32_t *)dst)[k] = px[4 * k] | px[4 * k + 1] << 8 | px[4 * k + 2] << 16 | px[4 * k + 3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < NB / 2; k++) ((uint16_t *)dst)[k] = (uint16_t)(px[2 * k] | px[2 * k + 1] << 8);
        }
    }
    __syncthreads();
    {
        const uint32_t r = threadIdx.x / (uint32_t)NB, c = threadIdx.x % (uint32_t)NB;
        if (r < rows && c * 8u + 8u <= nbytes)      /* rows <= N, nbytes <= 8 NB */
            *(uint2 *)(out + (size_t)r * pitch + c * 8u) = *(const uint2 *)(stage + r * kRow + c * 8u);
    }
    if (nbytes & 7u) {                  /* the same for the whole wave: lane r finishes row r */
        const uint32_t r = threadIdx.x, at = nbytes & ~7u;
        if (r < rows) {
            const uint2 w = *(const uint2 *)(stage + r * kRow + at);
            uint8_t *tail = out + (size_t)r * pitch + at;           /* 8-byte aligned */
            uint32_t v = w.x;
            if (nbytes & 4u) {
                *(uint32_t *)tail = v;
                tail += 4;
                v = w.y;
            }
            if (nbytes & 2u) {
                *(uint16_t *)tail = (uint16_t)v;
                tail += 2;
                v >>= 16;
            }
            if (nbytes & 1u) *tail = (uint8_t)v;
        }
    }
    __syncthreads();                    /* the staging buffer is free for the next run's image */
}

enum { PXS_GRAY1, PXS_GRAY3, PXS_444, PXS_PLANES };

/* The grid has the block rows that hold a visible output row: by * N < oh; run * 8 N < ow for every run
 * of a row, as in the any-size kernels.  PXS_PLANES: the chroma plane's rows are the output's rows; its
 * samples are N per block (a.up 0: 4:2:0, the plane has the luma's size) or N / 2 with their two clamped
 * neighbours (4:2:2); every index is below a.wc <= a.pc or, for a.up 0, below bw N = a.pc */
template <int N, int MODE>
__global__ __launch_bounds__(kWave) void k_pxs(const PxArgsScaled a)
{
    constexpr int NCH = MODE == PXS_444 ? 3 : 1, BPP = MODE == PXS_GRAY1 ? 1 : 3;
    __shared__ __attribute__((aligned(16))) uint32_t img[NCH * 512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;
    if (px_skip(a, f)) return;          /* the same for the whole workgroup */
    Lane L;
    if constexpr (MODE == PXS_GRAY1 || MODE == PXS_GRAY3) px_lane_gray(a, f, L);
    else px_lane(a, f, L);
    const uint32_t nruns = (a.g.bw + 7u) / 8u;
    const int16_t *frame = a.coef + (size_t)f * a.cstride;
    uint8_t *out = a.rgb + (size_t)f * a.ostride + (size_t)by * N * a.pitch;
    const uint32_t y0 = by * N, rows = y0 < a.oh ? min((uint32_t)N, a.oh - y0) : 0u;
    const uint8_t *crow = nullptr;      /* this lane's row of the Cb plane */
    if constexpr (MODE == PXS_PLANES)
        crow = a.planes + (size_t)f * 2u * a.plane + (size_t)(y0 + (L.j & (uint32_t)(N - 1))) * a.pc;
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.bw - run * 8u);
        const size_t blk = (size_t)by * a.g.bw + (size_t)run * 8u;
        uint32_t s[NCH][N], px[BPP * N];
        if constexpr (NCH == 3) {
            const int16_t *const src[3] = {frame + blk * 64, frame + ((size_t)a.g.nb + blk) * 64,
                                           frame + (2 * (size_t)a.g.nb + blk) * 64};
            const int tab[3] = {0, 1, 1};
            pxs_transform<3, N>(src, tab, n, L, img, s);
        } else {
            const int16_t *const src[1] = {frame + blk * 64};
            const int tab1[1] = {0};
            pxs_transform<1, N>(src, tab1, n, L, img, s);
        }
        if constexpr (MODE == PXS_GRAY1) {
#pragma unroll
            for (int c = 0; c < N; c++) px[c] = s[0][c];
        } else {
            uint32_t cb[N], cr[N];
#pragma unroll
            for (int c = 0; c < N; c++) cb[c] = cr[c] = 128u;
            if constexpr (MODE == PXS_444) {
#pragma unroll
                for (int c = 0; c < N; c++) cb[c] = s[1][c], cr[c] = s[2][c];
            }
            if constexpr (MODE == PXS_PLANES) {
                if (L.b < n && L.j < (uint32_t)N) {
                    const uint32_t x0 = (run * 8u + L.b) * N;       /* below bw N */
                    if (a.up == 0u) {
                        uint32_t w0, w1;
                        if constexpr (N == 4) {
                            w0 = *(const uint32_t *)(crow + x0);
                            w1 = *(const uint32_t *)(crow + a.plane + x0);
                        } else {
                            w0 = *(const uint16_t *)(crow + x0);
                            w1 = *(const uint16_t *)(crow + a.plane + x0);
                        }
#pragma unroll
                        for (int c = 0; c < N; c++) cb[c] = w0 >> (8 * c) & 255u, cr[c] = w1 >> (8 * c) & 255u;
                    } else {
                        /* samples i0 - 1 .. i0 + N / 2 of the row, every index clamped to [0, wc - 1] */
                        const uint32_t i0 = x0 >> 1, last = a.wc - 1u;
                        uint32_t p[2][N / 2 + 2];
#pragma unroll
                        for (int k = 0; k < N / 2 + 2; k++) {
                            const uint32_t i = min(max(i0 + k, 1u) - 1u, last);
                            p[0][k] = crow[i];
                            p[1][k] = crow[a.plane + i];
                        }
#pragma unroll
                        for (int i = 0; i < N / 2; i++) {
                            if (a.up == 1u) {
                                cb[2 * i] = cb[2 * i + 1] = p[0][i + 1];
                                cr[2 * i] = cr[2 * i + 1] = p[1][i + 1];
                            } else {
                                cb[2 * i] = jxi_up_even(p[0][i + 1], p[0][i], 0);
                                cb[2 * i + 1] = jxi_up_odd(p[0][i + 1], p[0][i + 2], 0);
                                cr[2 * i] = jxi_up_even(p[1][i + 1], p[1][i], 0);
                                cr[2 * i + 1] = jxi_up_odd(p[1][i + 1], p[1][i + 2], 0);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < N; c++) jxi_rgb(s[0][c], cb[c], cr[c], &px[3 * c], &px[3 * c + 1], &px[3 * c + 2]);
        }
        const uint32_t at = run * 8u * BPP * N, end = BPP * a.ow;   /* the run's first byte of a row; the row's end */
        pxs_store<BPP * N, N>(px, L, (uint8_t *)img, out + at, (size_t)a.pitch, rows,
                              at < end ? min(BPP * N * n, end - at) : 0u);
    }
}

/* Cb and Cr at N x N samples per block to the workspace: planes [2][N cbh][N cbw] per frame */
template <int N>
__global__ __launch_bounds__(kWave) void k_pxs_chroma(const PxArgsScaled a)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[2 * 512];
    const uint32_t f = blockIdx.z, by = blockIdx.y;     /* a chroma block row */
    if (px_skip(a, f)) return;
    Lane L;
    px_lane(a, f, L);
    const uint32_t nruns = (a.g.cbw + 7u) / 8u;
    const int16_t *frame = a.coef + (size_t)f * a.cstride + (size_t)a.g.nb * 64;
    uint8_t *out = a.planes + (size_t)f * 2u * a.plane + ((size_t)by * N + (L.j & (uint32_t)(N - 1))) * a.pc;
    const int tab[2] = {1, 1};
    for (uint32_t run = blockIdx.x * kRunsPerWave; run < min(nruns, (blockIdx.x + 1u) * kRunsPerWave); run++) {
        const uint32_t n = min(8u, a.g.cbw - run * 8u);
        const size_t blk = (size_t)by * a.g.cbw + (size_t)run * 8u;
        const int16_t *const src[2] = {frame + blk * 64, frame + ((size_t)a.g.nbc + blk) * 64};
        uint32_t s[2][N];
        pxs_transform<2, N>(src, tab, n, L, img, s);
        if (L.b < n && L.j < (uint32_t)N) {
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                uint8_t *dst = out + ch * a.plane + ((size_t)run * 8u + L.b) * N;
                if constexpr (N == 4) *(uint32_t *)dst = s[ch][0] | s[ch][1] << 8 | s[ch][2] << 16 | s[ch][3] << 24;
                else *(uint16_t *)dst = (uint16_t)(s[ch][0] | s[ch][1] << 8);
            }
        }
    }
}

enum { PXD_GRAY1, PXD_GRAY3, PXD_444, PXD_422, PXD_420 };

/* 1/8 of the size: a block is one pixel, the range-limited DESCALE(DC, 3).  Lane = block: a wave takes
 * 64 consecutive blocks of a block row and reads one int16 of each channel's block; 4:2:2 takes the
 * chroma block of its pair (replication), 4:2:0 its 2 x 2 samples from the workspace (k_pxs_chroma<2>).
 * The grid has the visible blocks only: blockIdx.y < oh <= bh and x < ow <= bw */
template <int MODE>
__global__ __launch_bounds__(kWave) void k_pxs_dc(const PxArgsScaled a)
{
    constexpr uint32_t BPP = MODE == PXD_GRAY1 ? 1u : 3u;
    __shared__ __attribute__((aligned(8))) uint8_t stage[64 * BPP];
    const uint32_t f = blockIdx.z, by = blockIdx.y, x0 = blockIdx.x * 64u, x = x0 + threadIdx.x;
    if (px_skip(a, f)) return;          /* the same for the whole workgroup */
    if (by >= a.oh || x0 >= a.ow) return;
    const uint16_t *qt = a.qt + (size_t)f * a.qstride;
    const int16_t *frame = a.coef + (size_t)f * a.cstride;
    if (x < a.ow) {
        const size_t blk = (size_t)by * a.g.bw + x;
        const uint32_t y = jxi_range(jxi_idct1(jxi_dequant(frame[blk * 64], qt[0])));
        if constexpr (MODE == PXD_GRAY1) {
            stage[threadIdx.x] = (uint8_t)y;
        } else {
            uint32_t cb = 128u, cr = 128u, r, g, b;
            if constexpr (MODE == PXD_444 || MODE == PXD_422) {
                const size_t cblk = MODE == PXD_444 ? blk : (size_t)by * a.g.cbw + (x >> 1);
                const uint16_t qc = qt[64];
                cb = jxi_range(jxi_idct1(jxi_dequant(frame[((size_t)a.g.nb + cblk) * 64], qc)));
                cr = jxi_range(jxi_idct1(jxi_dequant(frame[((size_t)a.g.nb + a.g.nbc + cblk) * 64], qc)));
            }
            if constexpr (MODE == PXD_420) {
                const uint8_t *p = a.planes + (size_t)f * 2u * a.plane + (size_t)by * a.pc + x;
                cb = p[0];
                cr = p[a.plane];
            }
            jxi_rgb(y, cb, cr, &r, &g, &b);
            stage[3u * threadIdx.x] = (uint8_t)r;
            stage[3u * threadIdx.x + 1u] = (uint8_t)g;
            stage[3u * threadIdx.x + 2u] = (uint8_t)b;
        }
    }
    __syncthreads();
    const uint32_t nbytes = BPP * min(64u, a.ow - x0);
    uint8_t *out = a.rgb + (size_t)f * a.ostride + (size_t)by * a.pitch + (size_t)x0 * BPP;  /* 8-byte aligned */
    if (threadIdx.x * 8u + 8u <= nbytes) *(uint2 *)(out + threadIdx.x * 8u) = *(const uint2 *)(stage + threadIdx.x * 8u);
    if ((nbytes & 7u) && threadIdx.x == 0u) {
        const uint32_t at = nbytes & ~7u;
        const uint2 w = *(const uint2 *)(stage + at);
        uint8_t *tail = out + at;
        uint32_t v = w.x;
        if (nbytes & 4u) {
            *(uint32_t *)tail = v;
            tail += 4;
            v = w.y;
        }
        if (nbytes & 2u) {
            *(uint16_t *)tail = (uint16_t)v;
            tail += 2;
            v >>= 16;
        }
        if (nbytes & 1u) *tail = (uint8_t)v;
    }
}

/* the chroma sample planes (4:2:x): the workspace's one part */
size_t px_workspace(const jx_frame &g, size_t nframes)
{
    jx_carve ws;
    if (g.hs > 1) ws.take(nframes * 2 * (size_t)g.nbc * 64);
    return ws.at;
}

unsigned px_grid_x(uint32_t blocks_per_row)
{
    const uint32_t nruns = (blocks_per_row + 7u) / 8u;
    return (nruns + kRunsPerWave - 1) / kRunsPerWave;
}

/* jpgx_pixels_gpu (ANY = 0) and jpgx_pixels_gpu_any: the checks and their order are the same but for
 * the geometry's rule.  ANY: the Y grid has the block rows that hold a visible pixel row; the chroma
 * kernel fills the coded planes whole, as it does for the plain call */
template <int ANY>
int px_run(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height, int sample_ratio,
           const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_rgb, size_t out_pitch,
           size_t out_frame_stride, void *d_workspace, size_t workspace_bytes, void *stream)
{
    typename PxA<ANY>::type a;
    memset(&a, 0, sizeof a);
    if (!d_coef || !d_qt || !d_rgb || ((uintptr_t)d_coef & 15) || ((uintptr_t)d_qt & 1) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_rgb & 7) || !jx_frames_ok(nframes))
        return JPGX_EARG;
    jx_frame f;
    unsigned yrows;
    if constexpr (ANY) {
        jx_frame_any fa;
        const int rc = jx_frame_rc_pixels(jx_frame_make_any(width, height, sample_ratio, &fa));
        if (rc) return rc;
        f = fa.c;
        a.w = fa.w, a.h = fa.h, a.wc = fa.wc, a.hc = fa.hc;
        yrows = (fa.h + 7u) / 8u;
    } else {
        const int rc = jx_frame_rc_pixels(jx_frame_make(width, height, sample_ratio, &f));
        if (rc) return rc;
        yrows = f.bh;
    }
    a.g = PxGeom{f.bw, f.bh, f.cbw, f.cbh, f.hs, f.vs, f.nb, f.nbc};
    if (!jx_coef_batch_ok(coef_frame_stride, f.nblk)) return JPGX_EARG;
    if (qt_frame_stride != 0 && qt_frame_stride < 128) return JPGX_EARG;
    if (out_pitch < (size_t)width * 3 || out_pitch % 8) return JPGX_EARG;
    if (out_frame_stride < out_pitch * (size_t)height || out_frame_stride % 8) return JPGX_EARG;
    const size_t need = px_workspace(f, nframes);
    if (workspace_bytes < need) return JPGX_EWORKSPACE;
    if (need && (!d_workspace || ((uintptr_t)d_workspace & 15))) return JPGX_EARG;
    a.coef = d_coef;
    a.cstride = coef_frame_stride;
    a.qt = d_qt;
    a.qstride = qt_frame_stride;
    a.status = d_status;
    a.rgb = d_rgb;
    a.pitch = out_pitch;
    a.ostride = out_frame_stride;
    a.planes = (uint8_t *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 ygrid(px_grid_x(a.g.bw), yrows, (unsigned)nframes);
    if (sample_ratio == 0) {
        hipLaunchKernelGGL(k_px444<ANY>, ygrid, dim3(kWave), 0, s, a);
    } else {
        const PxArgs &plain = a;
        hipLaunchKernelGGL(k_px_chroma, dim3(px_grid_x(a.g.cbw), a.g.cbh, (unsigned)nframes), dim3(kWave), 0, s, plain);
        if (sample_ratio == 2) hipLaunchKernelGGL((k_px_sub<1, ANY>), ygrid, dim3(kWave), 0, s, a);
        else hipLaunchKernelGGL((k_px_sub<0, ANY>), ygrid, dim3(kWave), 0, s, a);
    }
    return jx_hip_rc(hipGetLastError());
}

/* jpgx_pixels_gpu_gray: jpgx_pixels_gpu_any's checks in their order, with one table per frame, the
 * channel count and no workspace */
int px_run_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_out, size_t out_pitch,
                size_t out_frame_stride, int channels, void *stream)
{
    PxArgsGray a;
    memset(&a, 0, sizeof a);
    if (!d_coef || !d_qt || !d_out || ((uintptr_t)d_coef & 15) || ((uintptr_t)d_qt & 1) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_out & 7) || !jx_frames_ok(nframes) || (channels != 1 && channels != 3))
        return JPGX_EARG;
    jx_frame_gray g;
    const int rc = jx_frame_rc_pixels(jx_frame_make_gray(width, height, &g));
    if (rc) return rc;
    a.g = PxGeom{g.bw, g.bh, 0u, 0u, 1u, 1u, g.nb, 0u};
    a.w = g.w, a.h = g.h;
    if (!jx_coef_batch_ok(coef_frame_stride, g.nb)) return JPGX_EARG;
    if (qt_frame_stride != 0 && qt_frame_stride < 64) return JPGX_EARG;
    if (out_pitch < (size_t)width * (size_t)channels || out_pitch % 8) return JPGX_EARG;
    if (out_frame_stride < out_pitch * (size_t)height || out_frame_stride % 8) return JPGX_EARG;
    a.coef = d_coef;
    a.cstride = coef_frame_stride;
    a.qt = d_qt;
    a.qstride = qt_frame_stride;
    a.status = d_status;
    a.rgb = d_out;
    a.pitch = out_pitch;
    a.ostride = out_frame_stride;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(px_grid_x(g.bw), g.bh, (unsigned)nframes);
    if (channels == 1) hipLaunchKernelGGL(k_px_gray<1>, grid, dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(k_px_gray<3>, grid, dim3(kWave), 0, s, a);
    return jx_hip_rc(hipGetLastError());
}

/* 1 / d of the size: which sampling keeps its chroma samples in the workspace (4:2:0 always; 4:2:2 but
 * at 1/8, where a pixel pair takes its chroma block's DC), and the bytes of the two planes of a batch */
bool pxs_planes(const jx_frame &g, const jx_frame_scaled &s) { return g.vs > 1 || (g.hs > 1 && s.m > 1); }

size_t pxs_workspace(const jx_frame &g, const jx_frame_scaled &s, size_t nframes)
{
    jx_carve ws;
    if (pxs_planes(g, s)) ws.take(nframes * 2 * (size_t)g.nbc * s.n * s.n);
    return ws.at;
}

template <int MODE>
void pxs_launch(uint32_t m, dim3 grid, hipStream_t s, const PxArgsScaled &a)
{
    if (m == 4) hipLaunchKernelGGL((k_pxs<4, MODE>), grid, dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL((k_pxs<2, MODE>), grid, dim3(kWave), 0, s, a);
}

/* jpgx_pixels_gpu_scaled, d = 2, 4, 8: px_run<1>'s checks in their order, the output's size in the
 * place of the frame's */
int pxs_run(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height, int sample_ratio,
            int scale_denom, const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_rgb,
            size_t out_pitch, size_t out_frame_stride, void *d_workspace, size_t workspace_bytes, void *stream)
{
    PxArgsScaled a;
    memset(&a, 0, sizeof a);
    if (!d_coef || !d_qt || !d_rgb || ((uintptr_t)d_coef & 15) || ((uintptr_t)d_qt & 1) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_rgb & 7) || !jx_frames_ok(nframes) || !jx_scaled_ok(scale_denom))
        return JPGX_EARG;
    jx_frame_any fa;
    const int rc = jx_frame_rc_pixels(jx_frame_make_any(width, height, sample_ratio, &fa));
    if (rc) return rc;
    const jx_frame &f = fa.c;
    jx_frame_scaled sc;
    jx_frame_make_scaled(fa.w, fa.h, f.hs, f.vs, (uint32_t)scale_denom, &sc);
    a.g = PxGeom{f.bw, f.bh, f.cbw, f.cbh, f.hs, f.vs, f.nb, f.nbc};
    if (!jx_coef_batch_ok(coef_frame_stride, f.nblk)) return JPGX_EARG;
    if (qt_frame_stride != 0 && qt_frame_stride < 128) return JPGX_EARG;
    if (out_pitch < (size_t)sc.ow * 3 || out_pitch % 8) return JPGX_EARG;
    if (out_frame_stride < out_pitch * (size_t)sc.oh || out_frame_stride % 8) return JPGX_EARG;
    const size_t need = pxs_workspace(f, sc, nframes);
    if (workspace_bytes < need) return JPGX_EWORKSPACE;
    if (need && (!d_workspace || ((uintptr_t)d_workspace & 15))) return JPGX_EARG;
    a.coef = d_coef;
    a.cstride = coef_frame_stride;
    a.qt = d_qt;
    a.qstride = qt_frame_stride;
    a.status = d_status;
    a.rgb = d_rgb;
    a.pitch = out_pitch;
    a.ostride = out_frame_stride;
    a.planes = (uint8_t *)d_workspace;
    a.ow = sc.ow, a.oh = sc.oh, a.wc = sc.wc;
    a.pc = f.cbw * sc.n;
    a.plane = (unsigned long long)a.pc * f.cbh * sc.n;
    a.up = sc.hfac == 1 ? 0u : (sc.wc <= 2 || sc.m == 1) ? 1u : 2u;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nf = (unsigned)nframes;
    if (pxs_planes(f, sc)) {
        const dim3 cgrid(px_grid_x(f.cbw), f.cbh, nf);
        if (sc.n == 8) {
            const PxArgs &plain = a;
            hipLaunchKernelGGL(k_px_chroma, cgrid, dim3(kWave), 0, s, plain);
        } else if (sc.n == 4) {
            hipLaunchKernelGGL(k_pxs_chroma<4>, cgrid, dim3(kWave), 0, s, a);
        } else {
            hipLaunchKernelGGL(k_pxs_chroma<2>, cgrid, dim3(kWave), 0, s, a);
        }
    }
    if (sc.m == 1) {
        const dim3 grid((sc.ow + 63u) / 64u, sc.oh, nf);
        if (sample_ratio == 0) hipLaunchKernelGGL(k_pxs_dc<PXD_444>, grid, dim3(kWave), 0, s, a);
        else if (sample_ratio == 1) hipLaunchKernelGGL(k_pxs_dc<PXD_422>, grid, dim3(kWave), 0, s, a);
        else hipLaunchKernelGGL(k_pxs_dc<PXD_420>, grid, dim3(kWave), 0, s, a);
    } else {
        const dim3 grid(px_grid_x(f.bw), (sc.oh + sc.m - 1u) / sc.m, nf);
        if (sample_ratio == 0) pxs_launch<PXS_444>(sc.m, grid, s, a);
        else pxs_launch<PXS_PLANES>(sc.m, grid, s, a);
    }
    return jx_hip_rc(hipGetLastError());
}

/* jpgx_pixels_gpu_gray_scaled, d = 2, 4, 8: px_run_gray's checks in their order */
int pxs_run_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                 int scale_denom, const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_out,
                 size_t out_pitch, size_t out_frame_stride, int channels, void *stream)
{
    PxArgsScaled a;
    memset(&a, 0, sizeof a);
    if (!d_coef || !d_qt || !d_out || ((uintptr_t)d_coef & 15) || ((uintptr_t)d_qt & 1) || ((uintptr_t)d_status & 3) ||
        ((uintptr_t)d_out & 7) || !jx_frames_ok(nframes) || (channels != 1 && channels != 3) ||
        !jx_scaled_ok(scale_denom))
        return JPGX_EARG;
    jx_frame_gray g;
    const int rc = jx_frame_rc_pixels(jx_frame_make_gray(width, height, &g));
    if (rc) return rc;
    jx_frame_scaled sc;
    jx_frame_make_scaled(g.w, g.h, 1u, 1u, (uint32_t)scale_denom, &sc);
    a.g = PxGeom{g.bw, g.bh, 0u, 0u, 1u, 1u, g.nb, 0u};
    if (!jx_coef_batch_ok(coef_frame_stride, g.nb)) return JPGX_EARG;
    if (qt_frame_stride != 0 && qt_frame_stride < 64) return JPGX_EARG;
    if (out_pitch < (size_t)sc.ow * (size_t)channels || out_pitch % 8) return JPGX_EARG;
    if (out_frame_stride < out_pitch * (size_t)sc.oh || out_frame_stride % 8) return JPGX_EARG;
    a.coef = d_coef;
    a.cstride = coef_frame_stride;
    a.qt = d_qt;
    a.qstride = qt_frame_stride;
    a.status = d_status;
    a.rgb = d_out;
    a.pitch = out_pitch;
    a.ostride = out_frame_stride;
    a.ow = sc.ow, a.oh = sc.oh;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nf = (unsigned)nframes;
    if (sc.m == 1) {
        const dim3 grid((sc.ow + 63u) / 64u, sc.oh, nf);
        if (channels == 1) hipLaunchKernelGGL(k_pxs_dc<PXD_GRAY1>, grid, dim3(kWave), 0, s, a);
        else hipLaunchKernelGGL(k_pxs_dc<PXD_GRAY3>, grid, dim3(kWave), 0, s, a);
    } else {
        const dim3 grid(px_grid_x(g.bw), (sc.oh + sc.m - 1u) / sc.m, nf);
        if (channels == 1) pxs_launch<PXS_GRAY1>(sc.m, grid, s, a);
        else pxs_launch<PXS_GRAY3>(sc.m, grid, s, a);
    }
    return jx_hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

int jpgx_scaled_size(int width, int height, int scale_denom, int *out_width, int *out_height)
{
    if (!out_width || !out_height || width <= 0 || height <= 0 || width > 65535 || height > 65535 ||
        (scale_denom != 1 && !jx_scaled_ok(scale_denom)))
        return JPGX_EARG;
    *out_width = (width + scale_denom - 1) / scale_denom;
    *out_height = (height + scale_denom - 1) / scale_denom;
    return JPGX_OK;
}

size_t jpgx_pixels_gpu_scaled_workspace_size(int width, int height, int sample_ratio, int scale_denom, size_t nframes)
{
    if (scale_denom == 1) return jpgx_pixels_gpu_any_workspace_size(width, height, sample_ratio, nframes);
    jx_frame_any g;
    if (!jx_frames_ok(nframes) || !jx_scaled_ok(scale_denom) || jx_frame_make_any(width, height, sample_ratio, &g)) return 0;
    jx_frame_scaled sc;
    jx_frame_make_scaled(g.w, g.h, g.c.hs, g.c.vs, (uint32_t)scale_denom, &sc);
    return pxs_workspace(g.c, sc, nframes);
}

int jpgx_pixels_gpu_scaled(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                           int sample_ratio, int scale_denom, const uint16_t *d_qt, size_t qt_frame_stride,
                           const int32_t *d_status, uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride,
                           void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (scale_denom == 1)
        return px_run<1>(d_coef, coef_frame_stride, nframes, width, height, sample_ratio, d_qt, qt_frame_stride, d_status,
                         d_rgb, out_pitch, out_frame_stride, d_workspace, workspace_bytes, stream);
    return pxs_run(d_coef, coef_frame_stride, nframes, width, height, sample_ratio, scale_denom, d_qt, qt_frame_stride,
                   d_status, d_rgb, out_pitch, out_frame_stride, d_workspace, workspace_bytes, stream);
}

int jpgx_pixels_gpu_gray_scaled(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                                int scale_denom, const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                                uint8_t *d_out, size_t out_pitch, size_t out_frame_stride, int channels, void *stream)
{
    if (scale_denom == 1)
        return px_run_gray(d_coef, coef_frame_stride, nframes, width, height, d_qt, qt_frame_stride, d_status, d_out,
                           out_pitch, out_frame_stride, channels, stream);
    return pxs_run_gray(d_coef, coef_frame_stride, nframes, width, height, scale_denom, d_qt, qt_frame_stride, d_status,
                        d_out, out_pitch, out_frame_stride, channels, stream);
}

size_t jpgx_pixels_gpu_workspace_size(int width, int height, int sample_ratio, size_t nframes)
{
    jx_frame g;
    if (!jx_frames_ok(nframes) || jx_frame_make(width, height, sample_ratio, &g)) return 0;
    return px_workspace(g, nframes);
}

int jpgx_pixels_gpu(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                    int sample_ratio, const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                    uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride, void *d_workspace,
                    size_t workspace_bytes, void *stream)
{
    return px_run<0>(d_coef, coef_frame_stride, nframes, width, height, sample_ratio, d_qt, qt_frame_stride, d_status,
                     d_rgb, out_pitch, out_frame_stride, d_workspace, workspace_bytes, stream);
}

size_t jpgx_pixels_gpu_any_workspace_size(int width, int height, int sample_ratio, size_t nframes)
{
    jx_frame_any g;
    if (!jx_frames_ok(nframes) || jx_frame_make_any(width, height, sample_ratio, &g)) return 0;
    return px_workspace(g.c, nframes);
}

int jpgx_pixels_gpu_any(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                        int sample_ratio, const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                        uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride, void *d_workspace,
                        size_t workspace_bytes, void *stream)
{
    return px_run<1>(d_coef, coef_frame_stride, nframes, width, height, sample_ratio, d_qt, qt_frame_stride, d_status,
                     d_rgb, out_pitch, out_frame_stride, d_workspace, workspace_bytes, stream);
}

int jpgx_pixels_gpu_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                         const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_out,
                         size_t out_pitch, size_t out_frame_stride, int channels, void *stream)
{
    return px_run_gray(d_coef, coef_frame_stride, nframes, width, height, d_qt, qt_frame_stride, d_status, d_out,
                       out_pitch, out_frame_stride, channels, stream);
}

}  /* extern "C" */
