/*
 * jpgx_pad.c -- the edge rule of the encode side's _any entry points, stated on
 * the host in plain C99: the coded frame of an image is the image with its last column repeated to
 * the right and its last row repeated downwards, np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)),
 * mode="edge").  k_pad_edge (csrc/jpgx_pad.hip) computes the same bytes on the device;
 * jpgx_encode_rgb_to_jpeg_any (jpgx_jfif.c) pads with this routine.  No HIP, no allocation.
 */
#include <string.h>

#include "../../include/jpgx_compat.h"

int jpgx_pad_edge(const uint8_t *rgb, int width, int height, size_t pitch, int coded_width, int coded_height,
                  uint8_t *out)
{
    if (!rgb || !out) return JPGX_EARG;
    if (width <= 0 || height <= 0 || coded_width < width || coded_height < height) return JPGX_EGEOMETRY;
    if (pitch < (size_t)width * 3) return JPGX_EARG;
    const size_t w3 = (size_t)width * 3, cw3 = (size_t)coded_width * 3;
    for (int y = 0; y < coded_height; y++) {
        uint8_t *dst = out + (size_t)y * cw3;
        if (y >= height) {                                 /* the row above: the last row, padded */
            memcpy(dst, dst - cw3, cw3);
            continue;
        }
        const uint8_t *src = rgb + (size_t)y * pitch;
        memcpy(dst, src, w3);
        for (size_t x = w3; x < cw3; x++) dst[x] = src[w3 - 3 + x % 3];
    }
    return JPGX_OK;
}
