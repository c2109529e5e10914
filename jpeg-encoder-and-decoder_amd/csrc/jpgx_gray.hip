/*
 * jpgx_gray.hip -- k_gray, the forward path for one-channel images, and its entry point
 * jpgx_blocks_gpu_gray (include/jpgx.h).  Linked into both libraries; it has no
 * second implementation.  The contract is this project's own (the reference knows only RGB): the frame
 * is jx_frame_make_gray's, ceil(W / 8) x ceil(H / 8) blocks in raster order with standard tiling, the
 * pixels beyond the image by the edge rule, the sample byte - 128, then the reference's dct_block,
 * quantise_lum (the scaled luminance table applied transposed), C round() and zig-zag.
 *
 * k_gray (all-VALU; one lane = one 8x8 block, one wave = a tile of 64 consecutive blocks of the batch)
 *   HBM -> VGPR: the lane's 8 rows of 8 bytes (jx_gray_load_block, csrc/jx_gray.h: nothing is read
 *   outside the image, whatever the pitch and the alignment; aligned 8- or 4-byte loads where the rows
 *   allow them, bytes at the right edge and for rows that start off a dword).
 *   In the lane's registers: byte -> f32 - 128 (exact), row DCT then column DCT (jx_fdct8<FOps>), one
 *   FMA per coefficient with the fp32 scale that also rounds (+1.5 * 2^23); each int16 to the wave's
 *   LDS stage at its zig-zag position.
 *   Exactness: integer samples put four coefficients per block on exact rounding ties often (DESIGN.md
 *   4.11), so the exact pass is no rare path: every coefficient inside the guard band (jpgx_plan.cpp,
 *   jx_plan_tables_gray) becomes a task (block lane << 6 | u * 8 + v) in the wave's LDS queue, and the
 *   queue is drained 64 tasks at a time, one per lane: the lane fetches the block's 16 pixel dwords from
 *   the owning lane's registers (ds_bpermute, no LDS copy of the pixels) and runs jx_gray_exact, the
 *   oracle's 64 ordered fp64 terms, division and round(); the result replaces the fp32 one in the stage.
 *   LDS -> HBM: the wave's 64 blocks x 128 B leave as 8 KiB of 16-byte nontemporal stores, after the
 *   exact pass: a coefficient is written to memory once.
 * No workspace, no memset, no state but the per-quality tables, which are built once per device.
 *
 * Compiled with FP contraction off; the fast path uses explicit fmaf.
 */
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "jx_hip.h"             /* the HIP runtime first: jx_gray.h's functions are __host__ __device__ */

#include "jpgx_internal.h"
#include "jx_frame.h"
#include "jx_gray.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWG = 256;                /* threads per workgroup (4 waves) */
constexpr int kQueue = 1024;            /* tasks the wave's queue holds; a column adds at most 512 */

/* scan position of natural (row v, column u) */
__host__ __device__ constexpr int zz_of(int v, int u)
{
    constexpr int t[8][8] = JX_SCAN_ORDER_INIT;
    return t[v][u];
}
__constant__ int kScan[8][8] = JX_SCAN_ORDER_INIT;
__constant__ double kCos[8][8] = JX_COS_INIT;

/* Per-quality tables (index 0 unused), constant address space so that wave-uniform reads become scalar
 * loads.  Column-major ([u][v]): one column's 8 entries are one scalar load. */
struct GrayTab {
    float w[8][8];          /* fp32 scale of coefficient (row v, column u), 1/Q folded              */
    float lim[2][8][8];     /* |t - rint(t)| >= lim -> exact path; [1]: FORCE_EXACT, every entry -1 */
    int16_t q[64];          /* q[u * 8 + v] = Qs[u][v], the divisor of coefficient (row v, column u) */
};
__constant__ GrayTab g_gray[JX_MAXQ + 1];

struct GrayArgs {
    const uint8_t *src;     /* byte (0, 0) of frame 0 */
    int16_t *out;           /* frame 0's Y [nb][64] */
    long long in_pitch, in_fstride;     /* bytes */
    long long out_fstride;              /* int16 elements */
    uint32_t w, h, bw, nb;
    uint32_t total;         /* nb * nframes */
    jx_udiv dnb, dbw;
    int quality, force;
};

__device__ __forceinline__ uint32_t udiv(uint32_t n, const jx_udiv &d)
{
    const uint32_t t = __umulhi(d.m, n);
    return (t + ((n - t) >> d.s1)) >> d.s2;
}

struct DevMem {
    __device__ __forceinline__ uint64_t u64(const uint8_t *p) const { return *(const uint64_t *)p; }
    __device__ __forceinline__ uint32_t u32(const uint8_t *p) const { return *(const uint32_t *)p; }
    __device__ __forceinline__ uint8_t u8(const uint8_t *p) const { return *p; }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct WaveLds {
    uint32_t stage[64 * 33];            /* block k at dwords 33k.. (odd stride: the 16-bit writes of 64
                                           lanes hit 64 different banks) */
    uint16_t task[kQueue];              /* block lane << 6 | u * 8 + v */
};

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* number of set bits of m below this lane */
__device__ __forceinline__ unsigned lane_rank(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

/* The exact pass over the queue's n tasks (n wave-uniform), 64 at a time, one per lane; every lane
 * runs every step (the pixel fetch reads other lanes' registers).  raw: this lane's own block. */
__device__ __forceinline__ void drain(WaveLds &W, unsigned n, const uint32_t (&raw)[8][2], const GrayTab &tab,
                                      unsigned lane)
{
    wave_sync_lds();                    /* the tasks, and the fp32 values the exact ones replace */
    for (unsigned t0 = 0; t0 < n; t0 += 64u) {
        const unsigned ti = t0 + lane;
        const bool live = ti < n;
        const unsigned tk = live ? (unsigned)W.task[ti] : 0u, src = tk >> 6;
        const int u = (int)((tk >> 3) & 7u), v = (int)(tk & 7u);
        uint32_t blk[8][2];
#pragma unroll
        for (int y = 0; y < 8; y++)
#pragma unroll
            for (int k = 0; k < 2; k++)
                blk[y][k] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)raw[y][k]);
        const auto px = [&](int x, int y) { return jx_gray_byte(blk, x, y); };
        const int16_t val = jx_gray_exact(px, u, v, (int)tab.q[u * 8 + v], kCos);
        if (live) ((uint16_t *)W.stage)[src * 66u + (unsigned)kScan[v][u]] = (uint16_t)val;
    }
    wave_sync_lds();
}

__global__ __launch_bounds__(kWG, 3) void k_gray(const GrayArgs a)
{
    __shared__ WaveLds s_wave[kWG / 64];
    const unsigned lane = threadIdx.x & 63u;
    /* wave-uniform (readfirstlane: the compiler cannot see that threadIdx.x >> 6 is) */
    const unsigned wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned t = blockIdx.x * (kWG / 64) + wv;
    if (t >= (a.total + 63u) / 64u) return;
    WaveLds &W = s_wave[wv];
    const GrayTab &tab = g_gray[a.quality];
    const int fe = a.force ? 1 : 0;

    /* lanes past the batch's end compute its last block again and neither queue nor store */
    const unsigned b0 = t * 64u;
    const bool active = b0 + lane < a.total;
    const unsigned b = active ? b0 + lane : a.total - 1u;
    const unsigned f = udiv(b, a.dnb), bi = b - f * a.nb, by = udiv(bi, a.dbw), bx = bi - by * a.bw;
    uint32_t raw[8][2];
    jx_gray_load_block(DevMem{}, a.src + (long long)f * a.in_fstride, a.in_pitch, a.w, a.h, bx, by, raw);
    const uint64_t act = __ballot(active);

    float T[8][8];
    jx_gray_rows(raw, T);

    /* The columns in turn, each coefficient to the stage and the flagged ones to the queue; the queue
     * is drained once after the last column, and earlier only where another column might not fit
     * (FORCE_EXACT, or nearly every coefficient inside the band).  The form -- an endless loop around
     * the unrolled columns, each guarded by `u >= next && !stop` -- exists so that the compiler emits
     * each column's code and the exact pass once (u stays a compile-time index into T, so T stays in
     * registers; a drain inlined after every column would be eight copies of its 64 unrolled fp64
     * terms).  `next`, `stop` and `qn` are wave-uniform, so the guards are scalar branches: the usual
     * trip is eight columns, one drain, out. */
    unsigned next = 0, qn = 0;
    for (;;) {
        bool stop = false;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (!stop && (unsigned)u >= next) {
                float wu[8], lu[8], tm[8], d[8];
#pragma unroll
                for (int v = 0; v < 8; v++) {
                    wu[v] = tab.w[u][v];
                    lu[v] = tab.lim[fe][u][v];
                }
                jx_gray_col(T, u, wu, tm, d);
                uint64_t m[8], any = 0;
#pragma unroll
                for (int v = 0; v < 8; v++) {
                    ((uint16_t *)W.stage)[lane * 66u + (unsigned)zz_of(v, u)] = (uint16_t)__float_as_uint(tm[v]);
                    m[v] = __ballot(__builtin_fabsf(d[v]) >= lu[v]) & act;
                    any |= m[v];
                }
                if (any) {
#pragma unroll
                    for (int v = 0; v < 8; v++) {
                        if (m[v]) {
                            if ((m[v] >> lane) & 1u)
                                W.task[qn + lane_rank(m[v])] = (uint16_t)(lane << 6 | (unsigned)(u * 8 + v));
                            qn += (unsigned)__popcll(m[v]);
                        }
                    }
                }
                next = (unsigned)u + 1u;
                stop = qn > (unsigned)kQueue - 512u;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        drain(W, qn, raw, tab, lane);
        qn = 0;
        if (next >= 8u) break;
    }

    /* the staged tile leaves as coalesced stores: unit e = 64 j + lane is the 16 bytes (block e / 8,
     * zig-zag chunk e % 8) */
    const unsigned last = b0 + 63u < a.total ? b0 + 63u : a.total - 1u;
    const unsigned f0 = udiv(b0, a.dnb);
    if (b0 + 63u < a.total && udiv(last, a.dnb) == f0) {
        u32x4 *dst = (u32x4 *)(a.out + (long long)f0 * a.out_fstride + (long long)(b0 - f0 * a.nb) * 64);
        const unsigned o0 = (lane >> 3) * 33u + (lane & 7u) * 4u;
        u32x4 unit[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned o = o0 + 264u * (unsigned)j;
            unit[j] = u32x4{W.stage[o], W.stage[o + 1], W.stage[o + 2], W.stage[o + 3]};
        }
#pragma unroll
        for (int j = 0; j < 8; j++) __builtin_nontemporal_store(unit[j], dst + (unsigned)j * 64u + lane);
    } else {                            /* the tile crosses a frame's end, or is the batch's last */
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned e = (unsigned)j * 64u + lane, bb = b0 + (e >> 3);
            if (bb < a.total) {
                const unsigned ff = udiv(bb, a.dnb);
                const unsigned o = (e >> 3) * 33u + (e & 7u) * 4u;
                const u32x4 unit{W.stage[o], W.stage[o + 1], W.stage[o + 2], W.stage[o + 3]};
                __builtin_nontemporal_store(unit, (u32x4 *)(a.out + (long long)ff * a.out_fstride +
                                                            (long long)(bb - ff * a.nb) * 64 + (e & 7u) * 8u));
            }
        }
    }
}

std::once_flag g_tab_once[JX_MAX_DEV];
int g_tab_rc[JX_MAX_DEV];

int tables_for_current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= JX_MAX_DEV) return JPGX_ENODEV;
    std::call_once(g_tab_once[dev], [dev]() {
        std::vector<GrayTab> host(JX_MAXQ + 1);
        memset(host.data(), 0, host.size() * sizeof(GrayTab));
        for (int q = 1; q <= JX_MAXQ; q++) {
            float w[64], lim[64];
            jx_plan_tables_gray(q, w, lim, host[q].q);
            for (int u = 0; u < 8; u++)
                for (int v = 0; v < 8; v++) {
                    host[q].w[u][v] = w[v * 8 + u];
                    host[q].lim[0][u][v] = lim[v * 8 + u];
                    host[q].lim[1][u][v] = -1.0f;           /* FORCE_EXACT */
                }
        }
        g_tab_rc[dev] = jx_hip_rc(hipMemcpyToSymbol(HIP_SYMBOL(g_gray), host.data(), host.size() * sizeof(GrayTab)));
    });
    return g_tab_rc[dev];
}

}  // namespace

extern "C" int jpgx_blocks_gpu_gray(const uint8_t *d_gray, size_t in_pitch, size_t in_frame_stride, size_t nframes,
                                    int width, int height, int quality, unsigned flags, int16_t *d_out,
                                    size_t out_frame_stride, void *stream)
{
    if (quality < 1 || quality > JX_MAXQ) return JPGX_EQUALITY;
    jx_frame_gray g;
    if (jx_frame_make_gray(width, height, &g)) return JPGX_EGEOMETRY;
    if (!d_gray || !d_out || (flags & ~(unsigned)JPGX_FLAG_FORCE_EXACT) || in_pitch < (size_t)width ||
        !jx_frames_ok(nframes))
        return JPGX_EARG;
    if (((uintptr_t)d_out & 15) || !jx_coef_batch_ok(out_frame_stride, g.nb)) return JPGX_EARG;
    /* block indices are 32-bit: no batch of 2^32 blocks (512 GiB of coefficients) fits a device */
    if ((unsigned long long)g.nb * nframes > 0xffffffc0ull) return JPGX_EARG;
    const int rc = tables_for_current_device();
    if (rc) return rc;
    GrayArgs a;
    memset(&a, 0, sizeof a);
    a.src = d_gray;
    a.out = d_out;
    a.in_pitch = (long long)in_pitch;
    a.in_fstride = (long long)in_frame_stride;
    a.out_fstride = (long long)out_frame_stride;
    a.w = g.w;
    a.h = g.h;
    a.bw = g.bw;
    a.nb = g.nb;
    a.total = g.nb * (uint32_t)nframes;
    a.dnb = jx_udiv_make(g.nb);
    a.dbw = jx_udiv_make(g.bw);
    a.quality = quality;
    a.force = (flags & JPGX_FLAG_FORCE_EXACT) ? 1 : 0;
    const unsigned ntiles = (a.total + 63u) / 64u;
    hipLaunchKernelGGL(k_gray, dim3((ntiles + kWG / 64 - 1) / (kWG / 64)), dim3(kWG), 0, (hipStream_t)stream, a);
    return jx_hip_rc(hipGetLastError());
}
