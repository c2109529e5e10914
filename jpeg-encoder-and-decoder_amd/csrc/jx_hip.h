/* jx_hip.h -- what only the HIP translation units share (jpgx_plan.cpp is built by plain g++
 * without the HIP headers and does not include this) */
#ifndef JX_HIP_H
#define JX_HIP_H
#include <hip/hip_runtime.h>

#include "../../include/jpgx.h"
#define JX_MAX_DEV 64       /* devices with state of their own (tables uploaded once per device) */
static inline int jx_hip_rc(hipError_t e) { return e == hipSuccess ? JPGX_OK : JPGX_EHIP; }

/* what the batch entry points (JFIF coder, decoder, pixels) check and carve alike */
static inline size_t jx_r16(size_t x) { return (x + 15) / 16 * 16; }

/* a workspace carved front to back: every part begins on a multiple of 16 bytes */
struct jx_carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t off = at;
        at += jx_r16(bytes);
        return off;
    }
};

/* a grid dimension holds the frame index */
static inline bool jx_frames_ok(size_t nframes) { return nframes != 0 && nframes <= 65535; }

/* frames of whole blocks, coef_frame_stride int16 elements apart, each with room for nblk blocks */
static inline bool jx_coef_batch_ok(size_t coef_frame_stride, uint32_t nblk)
{
    return coef_frame_stride % 64 == 0 && coef_frame_stride >= (size_t)nblk * 64;
}

/* k_pad_edge (jpgx_pad.hip, both libraries): the coded frames of nframes images of
 * width x height -- rows of 3 coded_width bytes, frames coded_height rows apart, from the 16-byte
 * aligned d_coded -- with the last column repeated to the right and the last row downwards.  d_rgb: any
 * alignment, in_pitch >= 3 width; nothing is read outside bytes [0, 3 width) of rows [0, height) of a
 * frame.  The caller (jpgx_blocks_gpu_any, jpgx_device.hip) has checked the geometry.  It stands here
 * and not in jpgx_internal.h, whose text is part of the transform kernels' source hash
 * (tools/pmc_summary.py). */
extern "C" int jx_launch_pad(const uint8_t *d_rgb, uint8_t *d_coded, int width, int height, int coded_width,
                             int coded_height, int nframes, size_t in_pitch, size_t in_frame_stride, void *stream);
#endif
