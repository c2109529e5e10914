/*
 * jpgx_device.hip -- the device C ABI of include/jpgx.h: jpgx_blocks_gpu and its _ev / _timed
 * forms (argument checks, the launch arguments, one launcher), jpgx_blocks_gpu_any (k_pad_edge of
 * csrc/jpgx_pad.hip into the workspace, then the same launch), the on-device input generators
 * and jpgx_device_count.  Compiled twice; the launcher is the only difference.  The product
 * (libjpgx.so) runs one kernel per mode on the matrix cores (jx_launch_mx, csrc/jpgx_mx.hip):
 * k_mxs for 4:4:4, k_mxs422 / k_mxs420 for true 4:2:2 / 4:2:0.  The test-only cross-check library
 * (libjpgx_alt.so, -DJPGX_ALT_DISPATCH) runs the second implementation instead (jx_launch_alt,
 * csrc/jpgx_kernels.hip): k_xform for 4:4:4 and k_xform (Y) + k_chroma<1|2> for true 4:2:x.
 */
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "jpgx_internal.h"
#include "jx_frame.h"
#include "jx_hip.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint8_t splitmix_byte(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint8_t)(z >> 56);
}

__global__ void k_gen_splitmix(uint8_t *dst, size_t n, uint64_t seed)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x * 16;
    for (size_t k0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; k0 < n; k0 += stride) {
        if (k0 + 16 <= n && (((uintptr_t)(dst + k0)) & 15) == 0) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = 0;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    w[j] |= (uint32_t)splitmix_byte(seed, k0 + 4 * j + i) << (8 * i);
            }
            *(u32x4 *)(dst + k0) = u32x4{w[0], w[1], w[2], w[3]};
        } else {
            for (size_t k = k0; k < k0 + 16 && k < n; k++) dst[k] = splitmix_byte(seed, k);
        }
    }
}

__global__ void k_gen_tie(uint8_t *dst, int W, int H)
{
    const size_t npx = (size_t)W * H;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += stride) {
        const size_t y = i / W, x = i - y * W;
        const size_t bi = (y / 8) * (W / 8) + x / 8;
        const uint8_t v = (uint8_t)(97 + 2 * (bi % 40));
        dst[3 * i] = v;
        dst[3 * i + 1] = v;
        dst[3 * i + 2] = v;
    }
}

constexpr size_t kMaxPitch = (size_t)1 << 27;     /* 16 rows x pitch + 256 < 2^32 */

/* what a checked call launches; empty: a stripe of no rows, nothing to do */
struct BlocksPlan {
    jx_xform_args xa;
    int sr;                 /* the kernel's mode: 0, or the ratio of true subsampling */
    size_t nbc;
    bool empty;
};

/* every argument check of jpgx_blocks_gpu, and the launch arguments; no device call */
int blocks_plan(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb, int16_t *d_out,
                void *d_workspace, size_t workspace_bytes, BlocksPlan &pl)
{
    pl.empty = true;
    if (!fr || !p) return JPGX_EARG;
    int rc = jpgx_validate(fr->width, fr->height, p);
    if (rc) return rc;
    if (fr->row_begin < 0 || fr->row_end > fr->height / 8 || fr->row_begin > fr->row_end ||
        fr->nframes < 1)
        return JPGX_EARG;
    const bool sub = (p->flags & JPGX_FLAG_SUBSAMPLE) != 0;
    if (sub && p->sample_ratio == 0) return JPGX_ESAMPLE;
    if (sub && p->sample_ratio == 2 && ((fr->row_begin | fr->row_end) & 1)) return JPGX_EARG;
    if (fr->row_begin == fr->row_end) return JPGX_OK;
    if (!d_rgb || !d_out) return JPGX_EARG;
    if (fr->in_pitch < (size_t)fr->width * 3 || fr->in_pitch % 8 || fr->in_frame_stride % 8 ||
        ((uintptr_t)d_rgb & 7) || ((uintptr_t)d_out & 15) || fr->out_frame_stride % 8)
        return JPGX_EARG;
    /* the MFMA kernels address a step's pixel rows (up to 16 of them) with 32-bit lane offsets */
    if (fr->in_pitch > kMaxPitch) return JPGX_EARG;
    const int bpr = fr->width / 8;
    const size_t nb = (size_t)(fr->row_end - fr->row_begin) * bpr;
    const size_t total = nb * fr->nframes;
    if (total + 64 >= (1ull << 32)) return JPGX_EARG;
    const size_t nbc = sub ? jpgx_chroma_blocks(fr->width, fr->row_begin, fr->row_end,
                                                p->sample_ratio, p->flags)
                           : nb;
    if (fr->nframes > 1 && fr->out_frame_stride < (nb + 2 * nbc) * 64) return JPGX_EARG;
    if (fr->nframes > 1 && fr->in_frame_stride < fr->in_pitch * (size_t)(fr->row_end - fr->row_begin) * 8)
        return JPGX_EARG;
    if (workspace_bytes < jpgx_workspace_size(fr) || ((uintptr_t)d_workspace & 15))
        return JPGX_EWORKSPACE;

    jx_xform_args &xa = pl.xa;
    memset(&xa, 0, sizeof xa);
    jx_geom &g = xa.g;
    g.rgb = d_rgb;
    g.out = d_out;
    g.in_pitch = (long long)fr->in_pitch;
    g.in_fstride = (long long)fr->in_frame_stride;
    g.out_fstride = (long long)fr->out_frame_stride;
    g.bpr = bpr;
    g.nb = (int)nb;
    g.nframes = fr->nframes;
    g.row0 = fr->row_begin;
    g.dnb = jx_udiv_make((uint32_t)nb);
    g.dbpr = jx_udiv_make((uint32_t)bpr);
    g.mpr = (uint32_t)bpr / 2u;
    g.nmcu = (uint32_t)(nb / (size_t)bpr / 2u) * g.mpr;
    g.dmpr = jx_udiv_make(g.mpr ? g.mpr : 1u);
    g.dnmcu = jx_udiv_make(g.nmcu ? g.nmcu : 1u);
    jx_under_dwords(p->underflow, g.under);
    xa.quality = p->quality;
    xa.force_exact = (p->flags & JPGX_FLAG_FORCE_EXACT) ? 1 : 0;
    xa.luma_only = sub ? 1 : 0;
    pl.sr = sub ? p->sample_ratio : 0;
    pl.nbc = nbc;
    pl.empty = false;
    return JPGX_OK;
}

int blocks_launch(const BlocksPlan &pl, void *stream, void *event_after, void *ev_start, void *ev_stop)
{
#if JPGX_ALT_DISPATCH
    int rc = jx_launch_alt(&pl.xa, pl.sr, pl.nbc, stream, ev_start, ev_stop);
#else
    int rc = jx_launch_mx(&pl.xa, pl.sr, stream, ev_start, ev_stop);
#endif
    if (!rc && event_after) rc = jx_hip_rc(hipEventRecord((hipEvent_t)event_after, (hipStream_t)stream));
    return rc;
}

int blocks_gpu(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb, int16_t *d_out,
               void *d_workspace, size_t workspace_bytes, void *stream, void *event_after, void *ev_start,
               void *ev_stop)
{
    BlocksPlan pl;
    const int rc = blocks_plan(fr, p, d_rgb, d_out, d_workspace, workspace_bytes, pl);
    if (rc || pl.empty) return rc;
    return blocks_launch(pl, stream, event_after, ev_start, ev_stop);
}

/* ---- images of any width and height ------------------------------------------ */
struct AnyLayout {
    jpgx_frames cf;         /* the padded batch as the plain entry point takes it */
    jpgx_params cp;         /* the caller's parameters, for the coded size */
    size_t padded, inner, total;
};

/* the refusals of the table in include/jpgx.h but for the pointers and the workspace; no device call */
int any_layout(const jpgx_frames *fr, const jpgx_params *p, AnyLayout &l)
{
    if (!fr || !p) return JPGX_EARG;
    if (p->sample_ratio < 0 || p->sample_ratio > 2) return JPGX_ESAMPLE;
    if (p->quality < 1 || p->quality > JX_MAXQ) return JPGX_EQUALITY;
    jx_frame_any a;
    if (jx_frame_make_any(fr->width, fr->height, p->sample_ratio, &a)) return JPGX_EGEOMETRY;
    const int cw = (int)a.c.bw * 8, ch = (int)a.c.bh * 8;
    if (fr->nframes < 1 || fr->row_begin != 0 || fr->row_end != ch / 8) return JPGX_EARG;
    if (fr->in_pitch < (size_t)fr->width * 3) return JPGX_EARG;
    if (fr->nframes > 1 && fr->in_frame_stride < fr->in_pitch * (size_t)(fr->height - 1) + (size_t)fr->width * 3)
        return JPGX_EARG;
    l.cf = *fr;
    l.cf.width = cw;
    l.cf.height = ch;
    l.cf.in_pitch = (size_t)cw * 3;
    l.cf.in_frame_stride = l.cf.in_pitch * (size_t)ch;
    /* the underflow bytes depend on the size: the caller's defaults become the coded size's, bytes
     * the caller chose stay */
    jpgx_params dv, dc;
    jpgx_default_params(&dv, fr->width, fr->height, p->quality, p->sample_ratio);
    jpgx_default_params(&dc, cw, ch, p->quality, p->sample_ratio);
    l.cp = *p;
    if (!memcmp(p->underflow, dv.underflow, sizeof dv.underflow)) memcpy(l.cp.underflow, dc.underflow, sizeof dc.underflow);
    jx_carve ws;
    l.padded = ws.take(l.cf.in_frame_stride * (size_t)fr->nframes);
    l.inner = ws.take(jpgx_workspace_size(&l.cf));
    l.total = ws.at;
    return JPGX_OK;
}

}  // namespace

extern "C" {

int jpgx_blocks_gpu(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                    int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return jpgx_blocks_gpu_ev(fr, p, d_rgb, d_out, d_workspace, workspace_bytes, stream, nullptr);
}

int jpgx_blocks_gpu_ev(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                       int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream,
                       void *event_after)
{
    return blocks_gpu(fr, p, d_rgb, d_out, d_workspace, workspace_bytes, stream, event_after, nullptr, nullptr);
}

int jpgx_blocks_gpu_timed(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                          int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream,
                          void *ev_start, void *ev_stop)
{
    if (!ev_start || !ev_stop) return JPGX_EARG;
    return blocks_gpu(fr, p, d_rgb, d_out, d_workspace, workspace_bytes, stream, nullptr, ev_start, ev_stop);
}

size_t jpgx_workspace_size_any(const jpgx_frames *fr, const jpgx_params *p)
{
    AnyLayout l;
    return any_layout(fr, p, l) ? 0 : l.total;
}

int jpgx_blocks_gpu_any(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                        int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    AnyLayout l;
    int rc = any_layout(fr, p, l);
    if (rc) return rc;
    if (!d_rgb || !d_out || !d_workspace) return JPGX_EARG;
    if (workspace_bytes < l.total || ((uintptr_t)d_workspace & 15)) return JPGX_EWORKSPACE;
    uint8_t *padded = (uint8_t *)d_workspace + l.padded;
    BlocksPlan pl;
    rc = blocks_plan(&l.cf, &l.cp, padded, d_out, (uint8_t *)d_workspace + l.inner, workspace_bytes - l.inner, pl);
    if (rc || pl.empty) return rc;
    rc = jx_launch_pad(d_rgb, padded, fr->width, fr->height, l.cf.width, l.cf.height, fr->nframes, fr->in_pitch,
                       fr->in_frame_stride, stream);
    if (rc) return rc;
    return blocks_launch(pl, stream, nullptr, nullptr, nullptr);
}

int jpgx_gen_splitmix_gpu(uint8_t *d_dst, size_t nbytes, uint64_t seed, void *stream)
{
    if (!d_dst) return JPGX_EARG;
    if (!nbytes) return JPGX_OK;
    const size_t threads = (nbytes + 15) / 16;
    const unsigned grid = (unsigned)std::min<size_t>((threads + 255) / 256, 65536);
    hipLaunchKernelGGL(k_gen_splitmix, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_dst,
                       nbytes, seed);
    return jx_hip_rc(hipGetLastError());
}

int jpgx_gen_tie_gpu(uint8_t *d_dst, int width, int height, void *stream)
{
    if (!d_dst || width <= 0 || height <= 0 || width % 8 || height % 8) return JPGX_EARG;
    const size_t npx = (size_t)width * height;
    const unsigned grid = (unsigned)std::min<size_t>((npx + 255) / 256, 65536);
    hipLaunchKernelGGL(k_gen_tie, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_dst, width,
                       height);
    return jx_hip_rc(hipGetLastError());
}

int jpgx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  /* extern "C" */
