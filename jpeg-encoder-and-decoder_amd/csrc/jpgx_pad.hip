/*
 * jpgx_pad.hip -- k_pad_edge: the coded frames of a batch of images of any width
 * and height, for the forward path's _any entry point (jpgx_blocks_gpu_any, jpgx_device.hip).  The
 * coded frame is the image with its last column repeated to the right and its last row repeated
 * downwards, up to the MCU (jx_frame_coded): np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)), "edge").
 *
 * A pure data mover, 3 B read and 3 B written per pixel.  The destination is ours: rows of 3 cw bytes
 * (a multiple of 24) from a 16-byte aligned base, so two rows together are a whole number of 16-byte
 * chunks and a lane stores one chunk with one dwordx4.  The source is the caller's: any pitch >= 3 W,
 * any base alignment (a torch tensor 667 pixels wide has rows of 2001 bytes).  A lane reads the four
 * or five aligned dwords that hold its chunk's 16 source bytes and funnels them (v_alignbyte_b32).
 * Reads never leave [row start, row start + 3 W) of a row 0 .. H - 1: a chunk whose aligned dwords
 * would (a row's first chunk when the row starts off a dword, its last one or two), a chunk that
 * holds repeated columns, and the chunk that straddles the two rows of a pair when 3 cw is no
 * multiple of 16, are put together byte by byte instead -- about three chunks of a row.  That rule is
 * csrc/jx_pad.h's, one text for this kernel and for its host restatement (csrc/jpgx_pad_host.cpp), which
 * runs it with every load checked.  A lane takes the same chunk of kPadPairs row pairs and issues all
 * their loads before the first store.  No LDS.
 */
#include <stdint.h>

#include "jx_hip.h"
#include "jx_pad.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPadT = 256;              /* lanes per workgroup: one 16-byte chunk of a row pair each */
constexpr int kPadPairs = 4;            /* row pairs per lane: eight rows in flight */

struct PadArgs {
    const uint8_t *src;                 /* pixel (0, 0) of frame 0 */
    uint8_t *dst;                       /* the coded frames: rows of `pitch` bytes, frames npairs * 2 * pitch apart */
    size_t in_pitch, in_fstride;        /* bytes */
    uint32_t w3, h;                     /* 3 W; H */
    uint32_t pitch, npairs;             /* 3 cw; ch / 2 */
    uint32_t nframes;
};

/* the device's loads, as they are */
struct PadMem {
    __device__ __forceinline__ uint32_t u32(const uint8_t *p) const { return *(const uint32_t *)p; }
    __device__ __forceinline__ uint32_t u8(const uint8_t *p) const { return *p; }
};

__global__ __launch_bounds__(kPadT) void k_pad_edge(const PadArgs a)
{
    const uint32_t c = blockIdx.x * kPadT + threadIdx.x;        /* chunk of the row pair */
    if (c >= a.pitch / 8u) return;
    const JxPadChunk ck = jx_pad_chunk(c, a.pitch, a.w3);
    const PadMem mem;
    const uint32_t pair0 = blockIdx.y * kPadPairs;
    for (uint32_t f = blockIdx.z; f < a.nframes; f += gridDim.z) {
        const uint8_t *src = a.src + (size_t)f * a.in_fstride;
        uint8_t *dst = a.dst + (size_t)f * a.npairs * 2u * a.pitch;
        uint32_t d[kPadPairs][5], sh[kPadPairs];
        bool fast[kPadPairs];
#pragma unroll
        for (int j = 0; j < kPadPairs; j++) {
            const uint32_t pair = pair0 + j;
            fast[j] = false;
            if (pair >= a.npairs) continue;
            jx_pad_load(mem, src, a.in_pitch, a.w3, a.h, ck, pair, d[j], sh[j], fast[j]);
        }
        uint32_t slow = 0;                                      /* bit j: pair0 + j is left to the bytes */
#pragma unroll
        for (int j = 0; j < kPadPairs; j++) {
            const uint32_t pair = pair0 + j;
            if (pair >= a.npairs) continue;
            if (!fast[j]) {
                slow |= 1u << j;
                continue;
            }
            uint32_t w[4];
            JX_PAD_FUNNEL(w, d[j], sh[j]);
            *(u32x4 *)(dst + (size_t)pair * 2u * a.pitch + ck.o) = u32x4{w[0], w[1], w[2], w[3]};
        }
        /* the few chunks at a row's ends: rolled up, so that they cost the others no registers */
#pragma unroll 1
        for (; slow; slow &= slow - 1u) {
            const uint32_t pair = pair0 + (uint32_t)__builtin_ctz(slow);
            uint32_t w[4] = {0, 0, 0, 0};
            JX_PAD_BYTES(w, mem, src, a.in_pitch, a.w3, a.h, a.pitch, ck.o, pair);
            *(u32x4 *)(dst + (size_t)pair * 2u * a.pitch + ck.o) = u32x4{w[0], w[1], w[2], w[3]};
        }
    }
}

}  // namespace

extern "C" int jx_launch_pad(const uint8_t *d_rgb, uint8_t *d_coded, int width, int height, int coded_width,
                             int coded_height, int nframes, size_t in_pitch, size_t in_frame_stride, void *stream)
{
    PadArgs a;
    a.src = d_rgb;
    a.dst = d_coded;
    a.in_pitch = in_pitch;
    a.in_fstride = in_frame_stride;
    a.w3 = 3u * (uint32_t)width;
    a.h = (uint32_t)height;
    a.pitch = 3u * (uint32_t)coded_width;
    a.npairs = (uint32_t)coded_height / 2u;
    a.nframes = (uint32_t)nframes;
    /* a workgroup per 256 chunks of kPadPairs row pairs of a frame: about 4096 workgroups striding over
     * the groups instead measured 123 us where this takes 104 (8 x 3839 x 2159) */
    const uint32_t chunks = a.pitch / 8u;                       /* of a row pair */
    const dim3 grid((chunks + kPadT - 1) / kPadT, (a.npairs + kPadPairs - 1) / kPadPairs,
                    (unsigned)(nframes < 65535 ? nframes : 65535));
    hipLaunchKernelGGL(k_pad_edge, grid, dim3(kPadT), 0, (hipStream_t)stream, a);
    return jx_hip_rc(hipGetLastError());
}
