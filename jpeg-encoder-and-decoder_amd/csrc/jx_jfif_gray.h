/*
 * jx_jfif_gray.h -- the header bytes of a one-component (grayscale) baseline file, shared by the host
 * writer (csrc/jpgx_jfif_write.cpp: jpgx_write_jfif_gray) and the device coder (csrc/jpgx_jfif.hip:
 * jpgx_jfif_gpu_gray); the function is host/jpgx_jfif.c's.  Plain C99 that is also C++ and HIP.
 * Declared here and not in jpgx_internal.h, whose text is part of the transform kernels' source hash
 * (tools/pmc_summary.py).
 */
#ifndef JX_JFIF_GRAY_H
#define JX_JFIF_GRAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* SOI .. SOS of a width x height one-component file of `quality`: SOI, the colour writer's APP0, one DQT
 * (table 0, jpgx_jfif_qt(quality)[0]), SOF0 (SOF1 with a 16-bit table, q <= 23) with Nf = 1, component
 * id 1, sampling 0x11, Tq 0; two DHT segments, DC 0x00 and AC 0x10, holding bits[k] / vals[k] (bits
 * NULL: the Annex K.3 luminance tables, JX_JFIF_DHT_STD_GRAY bytes together; no table of
 * jx_jfif_optimal is longer); DRI of `ri` blocks when ri != 0; SOS with Ns = 1, Td / Ta 0 / 0, Ss 0,
 * Se 63.  *dht_at, when asked for, is where the first DHT segment begins: the bytes before it and the
 * bytes after the second segment do not depend on the tables.  Writes the first `cap` bytes into out
 * and returns their number (at most JX_JFIF_HDR_MAX; 0 when the quality is outside 1..97). */
#define JX_JFIF_DHT_STD_GRAY 216
size_t jx_jfif_header_gray(int width, int height, int quality, unsigned ri, const uint8_t bits[2][16],
                           const uint8_t vals[2][256], uint8_t *out, size_t cap, size_t *dht_at);
#ifdef __cplusplus
}
#endif

#endif
