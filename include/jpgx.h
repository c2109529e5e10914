/*
 * jpgx.h -- C ABI of the MI355X-native JPEG block-transform hot path (libjpgx.so).
 *
 * Replaces, for device-resident (or host) RGB frames, the per-8x8-block stage sequence of
 * matthewT53/JPEG-Encoder-and-Decoder that encode_bmp_to_jpeg() runs between loading the
 * bitmap and the entropy stage (reference src/jpg_encode.c:32-44):
 *
 *     preprocess_jpeg   src/preprocess.c:25-70   RGB -> YCbCr, level shift, 8x8 tiling
 *     chroma_subsample  src/downsample.c:9-32    (a print-only no-op in the reference)
 *     dct               src/dct.c:19-59          forward DCT-II per block
 *     quantise          src/quantise.c:30-86     quality-scaled tables, applied transposed
 *     zig_zag           src/zig_zag.c:17-58      scan order; result in JpgData.zig_zag_*
 *
 * Output contract (bit-exact to the reference on the same input, quirks included):
 *   int16 coefficients laid out [channel Y,Cb,Cr][block n, raster order][64 zig-zag], i.e. the
 *   reference's JpgData.zig_zag_Y[n][k], zig_zag_Cb[n][k], zig_zag_Cr[n][k]
 *   (src/headers/jpg_encode.h:60-62) narrowed to int16 (|coef| <= 2728 always fits).
 *
 * Input contract: interleaved, top-down pixels; byte k of each pixel is what the reference
 * loader calls plane k ("red", "green", "blue": src/bitmap.c:129-137).
 *
 * Conventions (unlike the reference, whose stages return void and mutate globals):
 *   - every entry point returns 0 or a negative JPGX_E* code;
 *   - callers own every buffer; the device path keeps no global mutable state (reentrant);
 *     the host-buffer path keeps its device buffers, streams and pinned staging in explicit
 *     contexts (jpgx_host_*), which jpgx_blocks / jpgx_blocks_multi take from a thread-safe
 *     process-wide pool (jpgx_host_release frees it).  One jpgx_host_ctx serves ONE caller at
 *     a time: its shards' buffers are reused call to call, so two threads must not call
 *     jpgx_host_blocks on the same context concurrently (use one context per thread, or the
 *     pooled jpgx_blocks, which hands each concurrent call its own context);
 *   - quantisation tables are rebuilt from the pristine base tables on every call
 *     (the reference rescales its globals in place, src/quantise.c:34-35).
 */
#ifndef JPGX_H
#define JPGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPGX_OK 0
#define JPGX_EGEOMETRY (-1)  /* width/height not a multiple of 8 (16 for 4:2:2 / 4:2:0)   */
#define JPGX_EQUALITY (-2)   /* quality outside [1, 97] (q >= 98 divides by zero, q <= 0
                                divides by zero: src/quantise.c:81-82)                     */
#define JPGX_ESAMPLE (-3)    /* sample_ratio not 0, 1 or 2                                 */
#define JPGX_EARG (-4)       /* null pointer, bad stripe, misaligned buffer or stride      */
#define JPGX_EHIP (-5)       /* HIP runtime error                                          */
#define JPGX_EWORKSPACE (-6) /* workspace smaller than jpgx_workspace_size()               */
#define JPGX_ENODEV (-7)     /* no usable GPU                                              */
#define JPGX_ENOMEM (-8)     /* host allocation failed                                     */
#define JPGX_EJFIF_HEADER (-9)  /* JFIF decoder: SOI .. SOS is not a file this decoder reads, or
                                   is not the geometry the caller stated                      */
#define JPGX_EJFIF_SCAN (-10)   /* JFIF decoder: the entropy-coded data, its restart markers or
                                   EOI are wrong                                              */

/* Chroma sampling constants, src/headers/jpg_encode.h:13-15.  The reference does not
 * actually subsample (src/downsample.c:24-32): 1 and 2 only tighten the geometry rule
 * (src/preprocess.c:87-95) and produce 4:4:4 output, which is what parity requires. */
#define JPGX_NO_CHROMA_SUBSAMPLING 0
#define JPGX_HORIZONTAL_SUBSAMPLING 1
#define JPGX_HORIZONTAL_VERTICAL_SUBSAMPLING 2

/* flags */
#define JPGX_FLAG_FORCE_EXACT 1u /* send every coefficient through the exact fp64 path     */
/* EXTENSION (no reference counterpart: src/downsample.c:24-32 only prints): with sample_ratio
 * 1 or 2, really subsample the chroma -- level-shifted Cb/Cr averaged over the horizontal pixel
 * pair (4:2:2) or the 2x2 quad (4:2:0), in that order; the (W/2) x H or (W/2) x (H/2) planes are
 * tiled in raster order (the x0 = -8 quirk stays a property of the 4:4:4 tiling only).  Y is
 * unchanged.  Frame output becomes Y [nb][64], Cb [nbc][64], Cr [nbc][64] contiguous, nbc =
 * jpgx_chroma_blocks(); for 4:2:0 stripes must start and end on even block rows. */
#define JPGX_FLAG_SUBSAMPLE 2u

typedef struct jpgx_params {
    int quality;              /* 1..97                                                    */
    int sample_ratio;         /* JPGX_*_SUBSAMPLING                                       */
    unsigned flags;           /* JPGX_FLAG_*                                              */
    uint8_t underflow[3][8];  /* [plane][x]: the 8 bytes the reference reads in front of
                                 each pixel plane r_new/g_new/b_new (src/preprocess.c:
                                 127-129) for the last block of block-row 0 (offset
                                 (y+y0)*W + x0 + x < 0 at :159, blockToCoords x0 = -8 at
                                 :199-211).  They are glibc's chunk-size words;
                                 jpgx_default_params fills the value a fresh
                                 encode_bmp_to_jpeg() process reads (all three equal). */
} jpgx_params;

/* A batch of frames, or one block-row stripe [row_begin, row_end) of each frame. */
typedef struct jpgx_frames {
    int width, height;        /* full-frame pixel geometry                                */
    int row_begin, row_end;   /* block rows processed; 0 and height/8 for whole frames    */
    int nframes;              /* frames in the batch (>= 1)                               */
    size_t in_pitch;          /* bytes between pixel rows (multiple of 8, at most 2^27)   */
    size_t in_frame_stride;   /* bytes between frames (multiple of 8)                     */
    size_t out_frame_stride;  /* int16 elements between frames' outputs                   */
} jpgx_frames;

/* Validation shared by every entry point. */
int jpgx_validate(int width, int height, const jpgx_params *p);

/* Defaults: the given quality/sample_ratio, no flags, glibc underflow bytes for a 24-bit
 * 54-byte-header BMP of this size (jpgx_glibc_underflow with file = 54 + 3*w*h). */
void jpgx_default_params(jpgx_params *p, int width, int height, int quality, int sample_ratio);

/* Chunk-size bytes glibc leaves in front of the reference's r_new/g_new/b_new planes
 * (src/preprocess.c:127-129) after its BMP loader freed a file-sized buffer
 * (src/bitmap.c:113,151), when the planes come from the top chunk or from mmap (every
 * image of 64x48 pixels or more in the fixtures; tiny images can reuse a freed chunk, then
 * pass the real bytes per plane).  n_pixels = w*h, bmp_file_size = size of the BMP file. */
void jpgx_glibc_underflow(long long n_pixels, long long bmp_file_size, uint8_t out[8]);

/* quantise.c:74-86 on a pristine base table: 0 = luminance, 1 = chrominance. */
int jpgx_scale_table(int which, int quality, int out[8][8]);

/* The guard band in use for `quality` (per channel, natural index v*8+u): a coefficient
 * whose fp32 quotient lies within lim of a rounding boundary is recomputed exactly.
 * Also returns the fp32 per-coefficient scale.  For tests and documentation. */
int jpgx_guard_band(int quality, float scale[3][64], float lim[3][64]);

/* Chroma blocks per channel of the stripe [row_begin, row_end) of a width-pixel frame: nb =
 * (row_end-row_begin)*width/8 without JPGX_FLAG_SUBSAMPLE (or sample_ratio 0), else
 * rows*width/16 (4:2:2) or rows/2*width/16 (4:2:0). */
size_t jpgx_chroma_blocks(int width, int row_begin, int row_end, int sample_ratio, unsigned flags);

/* ---- device path (pointers are device pointers; `stream` is a hipStream_t or NULL) ---- */

/* Bytes of device workspace one jpgx_blocks_gpu call on `fr` needs: 0 for every geometry
 * (both 4:4:4 kernels and k_chroma keep their exact-pass queues in LDS; d_workspace may then
 * be NULL).  Kept so callers stay source-compatible. */
size_t jpgx_workspace_size(const jpgx_frames *fr);

/* The fused hot path: RGB -> quantised zig-zag int16 for every block of fr's stripe of every
 * frame.  d_rgb points at pixel (0, 8*row_begin) of frame 0; when row_begin > 0 the pixel
 * row above it must be readable too (the x0 = -8 quirk reads the last 8 pixels of the
 * previous pixel row).  Frame f's output is [3][nb][64] at d_out + f*out_frame_stride,
 * nb = (row_end-row_begin)*width/8.  Asynchronous on `stream`. */
int jpgx_blocks_gpu(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                    int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* Same, and records hipEvent_t `event_between` (if non-NULL) on `stream` right after the
 * transform kernel (for timing the kernel alone against an event recorded before the call). */
int jpgx_blocks_gpu_ev(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                       int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream,
                       void *event_between);

/* Same as jpgx_blocks_gpu, and times the transform kernel itself: the 4:4:4 / true-4:2:x kernels
 * are launched through hipExtLaunchKernel with hipEvent_t ev_start / ev_stop (both required,
 * created by the caller), so hipEventElapsedTime(ev_start, ev_stop) is the kernel's execution
 * interval -- the one a rocprofv3 kernel trace reports, without the queue gap before the dispatch
 * that events recorded around the call include (bench.py's roofline).  The test-only library
 * records them around its kernels instead. */
int jpgx_blocks_gpu_timed(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                          int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream,
                          void *ev_start, void *ev_stop);

/* Entropy-stage statistics on the device: over one image's coefficients
 * d_coef = Y [nb_y][64] | Cb [nb_c][64] | Cr [nb_c][64] (what jpgx_blocks_gpu writes; nb_c =
 * nb_y unless JPGX_FLAG_SUBSAMPLE), the reference's in-place DC recurrence (src/dpcm.c:6-21)
 * into d_dc[nb_y + 2 nb_c] (int32), and huffman_encode's frequency pass (src/huffman.c:23-44,
 * 182-235; construct_huffman_table excluded) into d_hist[4][257] (uint32: lum_DC, lum_AC,
 * chrom_DC, chrom_AC; freq[256] = 1 as initialize_huffman reserves it; AC symbols keep the
 * reference's `run | size`).  carry (host, may be NULL = image start): per channel the last
 * dpcm'd DC of the blocks before these (jpgx_dpcm_dc semantics), for stripes.  Workspace:
 * jpgx_entropy_workspace_size() bytes, 8-byte aligned.  Asynchronous on `stream`. */
size_t jpgx_entropy_workspace_size(size_t nb_y, size_t nb_c);
int jpgx_entropy_stats_gpu(const int16_t *d_coef, size_t nb_y, size_t nb_c, const int32_t *carry,
                           int32_t *d_dc, uint32_t *d_hist, void *d_workspace,
                           size_t workspace_bytes, void *stream);
/* The same over a batch of nframes independent images of one size in one set of launches (what
 * jpgx_blocks_gpu writes for a frame batch: frame f's coefficients at d_coef + f *
 * coef_frame_stride int16 elements, a multiple of 64 and >= (nb_y + 2 nb_c) 64): d_dc
 * [nframes][nb_y + 2 nb_c], d_hist [nframes][4][257]; every frame starts its recurrence at the
 * image start (carry must be NULL unless nframes == 1).  Per-image launches leave the chip mostly
 * idle at 4K.  Workspace: jpgx_entropy_workspace_size_batch() bytes. */
size_t jpgx_entropy_workspace_size_batch(size_t nb_y, size_t nb_c, size_t nframes);
int jpgx_entropy_stats_gpu_batch(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, size_t nb_y,
                                 size_t nb_c, const int32_t *carry, int32_t *d_dc, uint32_t *d_hist,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

/* The JFIF files of a batch of frames, coded on the device from jpgx_blocks_gpu's output: frame
 * f's file (SOI .. EOI) at d_out + f * out_frame_stride, its length in d_len[f].  The bytes are
 * those of jpgx_write_jfif_ex (jpgx_compat.h) for the same coefficients, quality, sample_ratio and
 * restart interval: Annex K Huffman tables, one interleaved scan, d_coef frames laid out
 * [3][nb][64] (sample_ratio 0) or Y | Cb | Cr as JPGX_FLAG_SUBSAMPLE writes them (sample_ratio 1:
 * 4:2:2, 2: 4:2:0), frame f at d_coef + f * coef_frame_stride int16 elements (a multiple of 64,
 * at least one frame).
 * The device path NEEDS restart intervals -- they are what it codes in parallel: restart_rows >= 1
 * MCU rows per interval, or -1 for one MCU row per interval (NOT jpgx_write_jfif_ex's
 * thread-count-dependent -1: pass 1 there for the same bytes).  JPGX_EARG for restart_rows 0 or
 * below -1, for an interval above 65535 MCUs, nframes 0 or above 65535, out_frame_stride <
 * out_cap, null or misaligned pointers (d_coef, d_out, d_workspace: 16 bytes; d_len: 8);
 * JPGX_EWORKSPACE when workspace_bytes < jpgx_jfif_gpu_workspace_size() (0 for bad arguments).
 * Every argument check happens before the first device call.
 * Overflow: a frame that needs more than out_cap bytes writes nothing at or beyond out_cap in
 * its slot; d_len[f] then has bit 63 set and its low bits hold a capacity that suffices whatever
 * the byte stuffing (headers + 2 x unstuffed scan bytes + markers + EOI).  The other frames of
 * the batch are unaffected.  Asynchronous on `stream`, capturable, no global state; the library
 * initialises what it needs of the workspace itself. */
size_t jpgx_jfif_gpu_workspace_size(int width, int height, int sample_ratio, int restart_rows,
                                    size_t nframes, size_t out_cap);
int jpgx_jfif_gpu(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width,
                  int height, int quality, int sample_ratio, int restart_rows, uint8_t *d_out,
                  size_t out_frame_stride, size_t out_cap, uint64_t *d_len, void *d_workspace,
                  size_t workspace_bytes, void *stream);

/* A flag of the JFIF writers (jpgx_jfif_gpu_ex, jpgx_write_jfif_opt): per-image Huffman tables by
 * T.81 Annex K.2 from the image's own symbol counts instead of the Annex K.3 tables -- the same
 * file with other DHT contents and a shorter scan. */
#define JPGX_JFIF_OPTIMIZE 1u

/* jpgx_jfif_gpu with jfif_flags.  0: exactly jpgx_jfif_gpu_workspace_size / jpgx_jfif_gpu (the same
 * size, bytes and launches).  JPGX_JFIF_OPTIMIZE: frame f's file is, byte for byte, what
 * jpgx_write_jfif_opt writes for its coefficients with the same restart_rows and flags; every
 * frame of a batch gets its own tables.  The contract above holds as it stands (checks before any
 * device call, asynchronous, capturable, stateless, the workspace -- symbol counts included --
 * initialised by the call itself); in the overflow report "headers" is the frame's own header
 * length.  Unknown flag bits: JPGX_EARG (size 0 from the size query). */
size_t jpgx_jfif_gpu_workspace_size_ex(int width, int height, int sample_ratio, int restart_rows,
                                       size_t nframes, size_t out_cap, unsigned jfif_flags);
int jpgx_jfif_gpu_ex(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width,
                     int height, int quality, int sample_ratio, int restart_rows,
                     unsigned jfif_flags, uint8_t *d_out, size_t out_frame_stride, size_t out_cap,
                     uint64_t *d_len, void *d_workspace, size_t workspace_bytes, void *stream);

/* The way back: the coefficients of a batch of baseline JFIF files in device
 * memory -- entropy decoding only; dequantisation, IDCT and colour conversion are not part of it.
 * Frame f's file is the d_len[f] bytes at d_files + f * file_stride, exactly what jpgx_jfif_gpu
 * leaves (pass its d_out, out_frame_stride and d_len on); its coefficients go to d_coef + f *
 * coef_frame_stride int16 elements (a multiple of 64, at least one frame) in the layout of
 * jpgx_blocks_gpu: [3][nb][64] for sample_ratio 0, Y | Cb | Cr as JPGX_FLAG_SUBSAMPLE writes them
 * for 1 (4:2:2) and 2 (4:2:0); its two quantisation tables (Y's, then the one Cb and Cr share;
 * zig-zag order as in the file) to d_qt + f * 128 when d_qt is not NULL; its status to d_status[f].
 * What is read: jpgx_read_jfif's files (include/jpgx_compat.h) -- baseline SOF0, or SOF1 with 8-bit
 * samples; three components in one interleaved scan; DHT ids 0 and 1; any restart interval, none
 * included (the file is then decoded by a single lane).  The caller states width, height and
 * sample_ratio, so that every buffer can be sized without a look at the files.
 * d_status[f]: 0; JPGX_EJFIF_HEADER -- d_len[f] has bit 63 set (jpgx_jfif_gpu's overflow report) or
 * exceeds file_stride, the header is refused, or it states another geometry; JPGX_EJFIF_SCAN -- the
 * restart markers' count or numbers, a missing EOI, or an interval that does not decode to exactly
 * its MCUs.  The value equals jpgx_read_jfif's return for the same bytes.  A frame with status 0
 * has every coefficient written, equal to jpgx_read_jfif's; a failed frame's coefficients are
 * unspecified; nothing is written outside a frame's (nb + 2 nbc) * 64 elements, and a failed frame
 * does not touch the others.  The bytes are untrusted: no read leaves a file's d_len[f] bytes.
 * Returns JPGX_EARG for null or misaligned pointers (d_coef, d_workspace: 16 bytes; d_len: 8;
 * d_status: 4; d_qt: 2), nframes 0 or above 65535, file_stride 0 or within 4 KiB of 4 GiB and above, a
 * coef_frame_stride that is no multiple of 64 or below a frame; JPGX_EGEOMETRY for a width or height
 * that is no multiple of the MCU; JPGX_EWORKSPACE below jpgx_jfif_decode_gpu_workspace_size()
 * (file_cap = file_stride; 0 for bad arguments) -- all before the first device call.  Asynchronous
 * on `stream`, capturable, no global state; the call initialises what it reads of the workspace. */
size_t jpgx_jfif_decode_gpu_workspace_size(int width, int height, int sample_ratio, size_t nframes,
                                           size_t file_cap);
int jpgx_jfif_decode_gpu(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len,
                         size_t nframes, int width, int height, int sample_ratio, int16_t *d_coef,
                         size_t coef_frame_stride, uint16_t *d_qt, int32_t *d_status,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/* A flag of jpgx_jfif_decode_gpu_ex: decode inside the restart intervals.  A
 * workgroup of 256 lanes takes an interval; its lanes start at guessed places sub_bytes apart, hand
 * their exit states on until these are the sequential decoder's, and then write.  A file without
 * DRI is decoded by one workgroup instead of one lane. */
#define JPGX_JFIF_DECODE_SUBINTERVAL 1u

/* jpgx_jfif_decode_gpu with decode_flags.  0: exactly jpgx_jfif_decode_gpu_workspace_size /
 * jpgx_jfif_decode_gpu (the same size, outputs and launches).  JPGX_JFIF_DECODE_SUBINTERVAL: the
 * contract above holds as it stands -- the checks and their order, all before the first device
 * call; d_status[f] jpgx_read_jfif's return for the same bytes; a status-0 frame's coefficients
 * and tables the host's; no write outside a frame's elements, no read outside a file's bytes;
 * asynchronous, capturable, stateless, no memset -- with another kernel in the place of the scan.
 * Unknown flag bits: JPGX_EARG (size 0 from the size query).
 * jpgx_jfif_decode_sub_shape: the kernel's bytes per subsequence and subsequences per tile. */
size_t jpgx_jfif_decode_gpu_workspace_size_ex(int width, int height, int sample_ratio,
                                              size_t nframes, size_t file_cap, unsigned decode_flags);
int jpgx_jfif_decode_gpu_ex(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len,
                            size_t nframes, int width, int height, int sample_ratio,
                            unsigned decode_flags, int16_t *d_coef, size_t coef_frame_stride,
                            uint16_t *d_qt, int32_t *d_status, void *d_workspace,
                            size_t workspace_bytes, void *stream);
void jpgx_jfif_decode_sub_shape(uint32_t *sub_bytes, uint32_t *tile_subs);

/* The pixel half of the way back: coefficients to interleaved RGB, entirely on the
 * device.  The pixels are those of libjpeg's default decoder for the same coefficients and tables:
 * the 13-bit fixed-point ("islow") inverse DCT, the triangle-filter ("fancy") chroma upsampling for
 * 4:2:2 / 4:2:0 and the 16-bit fixed-point colour conversion -- pure int32 arithmetic that wraps,
 * stated in DESIGN.md 4.9 and equal, byte for byte, to jpgx_pixels_host (jpgx_compat.h).
 * d_coef, coef_frame_stride, width, height and sample_ratio mean what they mean for
 * jpgx_jfif_decode_gpu ([3][nb][64] for sample_ratio 0, Y | Cb | Cr as JPGX_FLAG_SUBSAMPLE writes
 * them for 1 and 2).  d_qt: [2][64] tables in zig-zag order (Y's, then the one Cb and Cr share),
 * frame f's pair at d_qt + f * qt_frame_stride: 128 is what jpgx_jfif_decode_gpu leaves, 0 means one
 * pair for the whole batch.  d_status may be NULL; otherwise a frame with d_status[f] != 0 is skipped
 * and none of its output bytes are written, so that jpgx_jfif_decode_gpu -> jpgx_pixels_gpu chains
 * on a stream with no host round trip.  Frame f's pixels: top-down rows out_pitch bytes apart at
 * d_rgb + f * out_frame_stride, byte 0 of a pixel = R = the byte the forward path reads as plane 0;
 * only bytes [0, 3 width) of a row are written.  Workspace: jpgx_pixels_gpu_workspace_size() bytes
 * (0 for sample_ratio 0, d_workspace may then be NULL; the chroma sample planes otherwise, 16-byte
 * aligned; 0 from the query for bad arguments).
 * JPGX_EARG: null d_coef, d_qt or d_rgb; d_coef not 16-byte, d_qt not 2-byte, d_status not 4-byte,
 * d_rgb not 8-byte aligned; nframes 0 or above 65535; a coef_frame_stride that is no multiple of 64
 * or below a frame; qt_frame_stride in [1, 127]; out_pitch below 3 width or no multiple of 8;
 * out_frame_stride below out_pitch * height or no multiple of 8; a needed workspace that is null or
 * misaligned.  JPGX_ESAMPLE: sample_ratio outside 0..2.  JPGX_EGEOMETRY: width or height no multiple
 * of the MCU.  JPGX_EWORKSPACE: workspace_bytes below the query's size.  All before the first device
 * call.  The coefficients and tables are untrusted: they only change values, never an address.
 * Asynchronous on `stream`, capturable, no global state, no memset; the call writes whatever it
 * reads of the workspace. */
size_t jpgx_pixels_gpu_workspace_size(int width, int height, int sample_ratio, size_t nframes);
int jpgx_pixels_gpu(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes,
                    int width, int height, int sample_ratio,
                    const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                    uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride,
                    void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- files of any width and height --------------------------------------
 * The entry points above take only sizes that are multiples of the MCU (8 x 8 for sample_ratio 0,
 * 16 x 8 for 1, 16 x 16 for 2).  The _any family takes any width and height in 1 .. 65535.  Such a
 * file codes every block of its coded frame: the size rounded up to the MCU (jpgx_coded_size).  The
 * coefficients are the coded frame's, in the layout above with nb and nbc counted over the coded
 * size; the pixels are the visible width x height.  For a size that is a multiple of the MCU every
 * output, return and workspace size of an _any call equals its sibling's.
 *
 * jpgx_coded_size: width and height rounded up to the MCU of sample_ratio, for sizing coefficient
 * buffers: nb = (coded_width / 8) * (coded_height / 8), nbc = nb / (1, 2, 4 for sample_ratio 0, 1,
 * 2).  JPGX_EARG for null pointers, a sample_ratio outside 0..2 or a side outside 1 .. 65535. */
int jpgx_coded_size(int width, int height, int sample_ratio, int *coded_width, int *coded_height);

/* jpgx_jfif_decode_gpu_workspace_size_ex / jpgx_jfif_decode_gpu_ex (decode_flags 0 or
 * JPGX_JFIF_DECODE_SUBINTERVAL) for files of any size.  width and height are the file's, as SOF
 * states them; a file that states others has status JPGX_EJFIF_HEADER.  coef_frame_stride is at least
 * the coded frame's (nb + 2 nbc) * 64; every block of the coded frame is decoded and written, the
 * blocks no pixel of which is visible included.  d_status[f], the coefficients and the tables equal
 * jpgx_read_jfif_any's for the same bytes.  The contract of jpgx_jfif_decode_gpu_ex holds otherwise,
 * word for word: the checks and their order, no read outside a file's d_len[f] bytes, no write
 * outside a frame's (nb + 2 nbc) * 64 elements.  A side outside 1 .. 65535 is JPGX_EARG;
 * JPGX_EGEOMETRY does not occur. */
size_t jpgx_jfif_decode_gpu_any_workspace_size(int width, int height, int sample_ratio,
                                               size_t nframes, size_t file_cap, unsigned decode_flags);
int jpgx_jfif_decode_gpu_any(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len,
                             size_t nframes, int width, int height, int sample_ratio,
                             unsigned decode_flags, int16_t *d_coef, size_t coef_frame_stride,
                             uint16_t *d_qt, int32_t *d_status, void *d_workspace,
                             size_t workspace_bytes, void *stream);

/* jpgx_pixels_gpu_workspace_size / jpgx_pixels_gpu for a frame of any size: d_coef holds the coded
 * frame's coefficients (jpgx_jfif_decode_gpu_any's output), width and height are the visible
 * frame's.  The pixels are libjpeg's default decoder's for a file of that size, equal byte for byte
 * to jpgx_pixels_host_any: whole blocks are transformed, and the chroma upsampling clamps at the
 * component's real extent, ceil(width / 2) samples per row and (4:2:0) ceil(height / 2) rows; with
 * two samples or fewer per row the chroma is replicated, not filtered.  This is not
 * a crop of the coded frame's pixels.  out_pitch is at least 3 width and a multiple of 8,
 * out_frame_stride at least out_pitch * height and a multiple of 8; only bytes [0, 3 width) of rows
 * [0, height) are written.  The workspace is the coded frame's chroma planes.  Everything else,
 * the checks, their order and their codes included, is jpgx_pixels_gpu's: a side outside
 * 1 .. 65535 is JPGX_EGEOMETRY, the only case of that code. */
size_t jpgx_pixels_gpu_any_workspace_size(int width, int height, int sample_ratio, size_t nframes);
int jpgx_pixels_gpu_any(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes,
                        int width, int height, int sample_ratio,
                        const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                        uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/* The encode side of the family.  The edge rule: the coded frame of a width x
 * height image is the image with its last column repeated to the right and its last row repeated
 * downwards, up to jpgx_coded_size's cw x ch -- numpy's np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)),
 * mode="edge").  It is this project's own rule, not libjpeg's (which fills the blocks beyond a
 * component's width with a DC-only copy of the block before); decoders crop to SOF's size, so the file
 * is valid either way.
 *
 * jpgx_workspace_size_any / jpgx_blocks_gpu_any: jpgx_blocks_gpu for a batch of images of any width
 * and height.  fr->width and fr->height are the visible size, 1 .. 65535 each; whole frames only:
 * fr->row_begin 0 and fr->row_end ch / 8.  d_rgb: any alignment, fr->in_pitch >= 3 width with no
 * multiple-of-8 rule, any fr->in_frame_stride that keeps the frames of a batch apart (at least
 * in_pitch (height - 1) + 3 width); nothing is read outside bytes [0, 3 width) of rows [0, height) of a
 * frame.  d_out and fr->out_frame_stride follow jpgx_blocks_gpu's rules for the coded frame.  The call
 * builds the coded frames in the workspace (k_pad_edge, csrc/jpgx_pad.hip) and runs jpgx_blocks_gpu's
 * launch over them: the output is exactly jpgx_blocks_gpu's for the padded images with the caller's
 * quality, sample_ratio and flags (parity mode, JPGX_FLAG_SUBSAMPLE, JPGX_FLAG_FORCE_EXACT), in the
 * coded frame's layout Y [nb][64] | Cb [nbc][64] | Cr [nbc][64] -- what jpgx_jfif_decode_gpu_any
 * returns.  cw x ch is the coded size of p->sample_ratio whatever the flags.  The underflow bytes
 * depend on the image size: where p->underflow equals jpgx_default_params' for width x height the
 * bytes of the coded size are used (jpgx_default_params(cw, ch)), other bytes are the caller's own and
 * stay.  Workspace: the padded batch, nframes * ch * 3 cw bytes, plus jpgx_workspace_size of the coded
 * frame, every part rounded up to 16 bytes; 16-byte aligned.  Asynchronous on `stream`, capturable, no
 * global state.  All checks happen before the first device call, the first that applies:
 * JPGX_EARG (null fr or p), JPGX_ESAMPLE, JPGX_EQUALITY, JPGX_EGEOMETRY (a side outside 1 .. 65535),
 * JPGX_EARG (nframes < 1, a stripe that is not the whole frame, in_pitch, in_frame_stride, null
 * d_rgb, d_out or d_workspace), JPGX_EWORKSPACE (too small or misaligned), then jpgx_blocks_gpu's own
 * for the coded frame.  The size query returns 0 where the call returns one of the first five. */
size_t jpgx_workspace_size_any(const jpgx_frames *fr, const jpgx_params *p);
int jpgx_blocks_gpu_any(const jpgx_frames *fr, const jpgx_params *p, const uint8_t *d_rgb,
                        int16_t *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* jpgx_jfif_gpu_workspace_size_ex / jpgx_jfif_gpu_ex (jfif_flags 0 or JPGX_JFIF_OPTIMIZE) for files of
 * any width and height, 1 .. 65535 each: d_coef holds the coded frames (jpgx_blocks_gpu_any's output,
 * coef_frame_stride at least the coded frame's (nb + 2 nbc) * 64), every block of which is coded by
 * the same kernels; SOF states width x height; the restart interval still counts MCUs of the coded
 * frame.  Frame f's file is jpgx_write_jfif_any's for the same arguments (restart_rows -1 there: 1),
 * which is jpgx_jfif_gpu_ex's file for the coded size with the four size bytes of SOF replaced.  A
 * sample_ratio outside 0 .. 2 or a side outside 1 .. 65535 is JPGX_EARG (0 from the size query);
 * JPGX_EGEOMETRY does not occur; the contract of jpgx_jfif_gpu_ex holds otherwise, word for word. */
size_t jpgx_jfif_gpu_any_workspace_size(int width, int height, int sample_ratio, int restart_rows,
                                        size_t nframes, size_t out_cap, unsigned jfif_flags);
int jpgx_jfif_gpu_any(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width,
                      int height, int quality, int sample_ratio, int restart_rows,
                      unsigned jfif_flags, uint8_t *d_out, size_t out_frame_stride, size_t out_cap,
                      uint64_t *d_len, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- one-component (grayscale) files -------------------------------------
 * The entry points above refuse a file with one component (JPGX_EJFIF_HEADER); the _gray family takes
 * such files and only such files, of any width and height in 1 .. 65535.  What is accepted is stated
 * at jpgx_read_jfif_gray (jpgx_compat.h): one component with any sampling factors 1 .. 4, which are
 * ignored, in one scan.  The file codes nb = ceil(width / 8) * ceil(height / 8) blocks in raster
 * order; DRI counts blocks.  Coefficients: Y [nb][64], zig-zag.  One table of [64] per frame.
 *
 * jpgx_jfif_decode_gpu_gray_workspace_size / jpgx_jfif_decode_gpu_gray: jpgx_jfif_decode_gpu_any's
 * contract without sample_ratio, word for word: decode_flags 0 or JPGX_JFIF_DECODE_SUBINTERVAL;
 * coef_frame_stride a multiple of 64 and at least nb * 64; frame f's table at d_qt + f * 64 (zeros
 * for a refused header; d_qt may be NULL); d_status[f], the coefficients and the table equal
 * jpgx_read_jfif_gray's for the same bytes; a file whose SOF states another size, or that has three
 * components, has status JPGX_EJFIF_HEADER.  The argument checks, their order and their codes are
 * the _any call's, all before the first device call; asynchronous, capturable, stateless, no memset;
 * the same five launches with the header and scan kernels in their one-component instantiations.
 * Workspace (0 from the query for bad arguments), every part rounded up to 16 bytes: per frame the
 * header walk's notes (sizeof(jxd_frame), csrc/jx_jfif_dec.h) and four decode tables
 * (4 * sizeof(jxd_tab)), 4 bytes of status, 4 bytes per 4 KiB chunk of file_cap, and 4 bytes per
 * block (nmcu = nb restart markers' places at most). */
size_t jpgx_jfif_decode_gpu_gray_workspace_size(int width, int height, size_t nframes, size_t file_cap,
                                                unsigned decode_flags);
int jpgx_jfif_decode_gpu_gray(const uint8_t *d_files, size_t file_stride, const uint64_t *d_len,
                              size_t nframes, int width, int height, unsigned decode_flags,
                              int16_t *d_coef, size_t coef_frame_stride, uint16_t *d_qt,
                              int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                              void *stream);

/* The pixels of one-component frames: libjpeg's default decoder's, equal byte for byte to
 * jpgx_pixels_host_gray.  channels 1: the range-limited inverse DCT's sample (JCS_GRAYSCALE);
 * channels 3: that sample as R = G = B (libjpeg's gray-to-RGB).  No workspace.  d_coef: Y [nb][64] per
 * frame, coef_frame_stride a multiple of 64 and at least nb * 64.  d_qt: frame f's table at
 * d_qt + f * qt_frame_stride; 64 is what jpgx_jfif_decode_gpu_gray leaves, 0 means one table for the
 * batch, [1, 63] is JPGX_EARG.  out_pitch is at least channels * width and a multiple of 8,
 * out_frame_stride at least out_pitch * height and a multiple of 8; only bytes
 * [0, channels * width) of rows [0, height) are written; a frame with d_status[f] != 0 is skipped and
 * untouched.  channels other than 1 and 3 is JPGX_EARG; a side outside 1 .. 65535 is JPGX_EGEOMETRY.
 * The alignments, the remaining checks, their order and everything else are jpgx_pixels_gpu_any's. */
int jpgx_pixels_gpu_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes,
                         int width, int height, const uint16_t *d_qt, size_t qt_frame_stride,
                         const int32_t *d_status, uint8_t *d_out, size_t out_pitch,
                         size_t out_frame_stride, int channels, void *stream);

/* ---- 1/2, 1/4 and 1/8 of the size ------------------------------------------------
 * libjpeg-turbo's default decoder with scale_num / scale_denom = 1 / scale_denom: reduced-size inverse
 * DCTs produce the small image from the coefficients directly.  The output is ow x oh =
 * ceil(width / scale_denom) x ceil(height / scale_denom) (jpgx_scaled_size; JPGX_EARG for null
 * pointers, a side outside 1 .. 65535 or a scale_denom other than 1, 2, 4, 8).  A luma block becomes
 * m x m = 8 / scale_denom samples; a chroma block m x m too, for 4:2:0 2m x 2m, which is the luma's
 * size; 4:2:2's chroma goes through the h2v1 triangle filter clamped at its real extent
 * ceil(width * m / 16), and is replicated where that is 2 or less and at 1/8.  Equal byte for byte to
 * jpgx_pixels_host_scaled / jpgx_pixels_host_gray_scaled (jpgx_compat.h).
 *
 * jpgx_pixels_gpu_scaled: jpgx_pixels_gpu_any's arguments with scale_denom after sample_ratio;
 * jpgx_pixels_gpu_gray_scaled: jpgx_pixels_gpu_gray's with scale_denom after height.  width and height
 * are the file's, the coefficients the coded frame's.  scale_denom 1 is the sibling's call, launch for
 * launch.  Otherwise the sibling's contract holds with ow x oh in the place of width x height:
 * out_pitch at least bytes per pixel * ow and a multiple of 8, out_frame_stride at least out_pitch * oh
 * and a multiple of 8; only bytes [0, bytes per pixel * ow) of rows [0, oh) are written; a frame with
 * d_status[f] != 0 is skipped and untouched.  The checks and their order are the sibling's, with
 * JPGX_EARG for a scale_denom other than 1, 2, 4, 8 among the first (the pointer and alignment checks).
 * Workspace (jpgx_pixels_gpu_scaled_workspace_size; 0 for bad arguments): the two chroma sample planes
 * at their reduced size for 4:2:2 at 1/2 and 1/4 and for 4:2:0, 16-byte aligned; none for 4:4:4, for
 * 4:2:2 at 1/8 and for one-component frames. */
int jpgx_scaled_size(int width, int height, int scale_denom, int *out_width, int *out_height);
size_t jpgx_pixels_gpu_scaled_workspace_size(int width, int height, int sample_ratio, int scale_denom,
                                             size_t nframes);
int jpgx_pixels_gpu_scaled(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes,
                           int width, int height, int sample_ratio, int scale_denom,
                           const uint16_t *d_qt, size_t qt_frame_stride, const int32_t *d_status,
                           uint8_t *d_rgb, size_t out_pitch, size_t out_frame_stride,
                           void *d_workspace, size_t workspace_bytes, void *stream);
int jpgx_pixels_gpu_gray_scaled(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes,
                                int width, int height, int scale_denom, const uint16_t *d_qt,
                                size_t qt_frame_stride, const int32_t *d_status, uint8_t *d_out,
                                size_t out_pitch, size_t out_frame_stride, int channels, void *stream);

/* ---- the encode side of the one-component family ---------------------------
 * The reference knows only RGB: this contract is the project's own (parity unpinned).  A one-channel
 * image of width x height, 1 .. 65535 each, is coded as jx_frame_make_gray's frame (csrc/jx_frame.h):
 * bw x bh = ceil(width / 8) x ceil(height / 8) blocks in raster order with standard tiling (no x0 = -8
 * quirk), no chroma, never rounded up to a larger MCU.  Pixels beyond the image follow the edge rule of
 * the any-size family: the last column repeated to the right, the last row downwards.  The sample is
 * (double)g - 128; a block's coefficients are the reference's dct_block in its exact operation order,
 * quantise_lum with the scaled luminance table applied transposed, C round() and zig-zag -- what
 * cpuref_dct_block, cpuref_quantise_block (with cpuref_scale_table(cpuref_q_lum, q)) and
 * cpuref_zigzag_block compute.  Output: int16 Y [nb][64] per frame, what jpgx_jfif_decode_gpu_gray
 * returns and jpgx_pixels_gpu_gray takes.
 *
 * jpgx_blocks_gpu_gray: one launch of k_gray (csrc/jpgx_gray.hip) over the batch.  d_gray: uint8
 * [height][width] top-down, rows in_pitch >= width bytes apart, frames in_frame_stride bytes apart (any
 * value: the input is only read, so frames may overlap or, with 0, be one frame);
 * any pitch and any alignment; nothing is read outside bytes [0, width) of rows [0, height) of a frame.
 * d_out: 16-byte aligned, frames out_frame_stride int16 elements apart, a multiple of 64 and at least
 * nb * 64; only a frame's nb * 64 elements are written.  flags: 0 or JPGX_FLAG_FORCE_EXACT (every
 * coefficient through the exact path; the same output).  No workspace; asynchronous on `stream`,
 * capturable, no state but the per-quality tables built once per device.  All checks happen before the
 * first device call, the first that applies: JPGX_EQUALITY (quality outside 1 .. 97), JPGX_EGEOMETRY (a
 * side outside 1 .. 65535), JPGX_EARG (null d_gray or d_out, unknown flags, in_pitch < width, nframes
 * outside 1 .. 65535, d_out not 16-byte aligned, an out_frame_stride that is not whole blocks or is too small, a batch of 2^32
 * blocks or more).
 *
 * jpgx_jfif_gpu_gray_workspace_size / jpgx_jfif_gpu_gray: jpgx_jfif_gpu_any's contract without
 * sample_ratio, for one-component files: d_coef holds Y [nb][64] per frame (coef_frame_stride a
 * multiple of 64 and at least nb * 64); frame f's file is jpgx_write_jfif_gray's (jpgx_compat.h) for
 * the same arguments byte for byte, restart_rows -1 meaning one block row here.  restart_rows counts
 * block rows, DRI counts blocks: rows x bw must fit 16 bits, 0 is refused.  jfif_flags 0 or
 * JPGX_JFIF_OPTIMIZE (the frame's own two luminance tables).  The same kernels as the colour coder walk
 * the one-component frame (hs = vs = lum = bpm = 1, cbw = bw, cbh = bh, nbc = 0).  JPGX_EARG for a side
 * outside 1 .. 65535, the interval, the flags, the pointers and the strides; JPGX_EQUALITY;
 * JPGX_EWORKSPACE; the capacity report in d_len[f] (bit 63 and a capacity that suffices) and everything
 * else are jpgx_jfif_gpu_ex's.  jpgx_jfif_bound(8 bw, 8 bh) bounds a frame's file. */
int jpgx_blocks_gpu_gray(const uint8_t *d_gray, size_t in_pitch, size_t in_frame_stride, size_t nframes,
                         int width, int height, int quality, unsigned flags, int16_t *d_out,
                         size_t out_frame_stride, void *stream);
size_t jpgx_jfif_gpu_gray_workspace_size(int width, int height, int restart_rows, size_t nframes,
                                         size_t out_cap, unsigned jfif_flags);
int jpgx_jfif_gpu_gray(const int16_t *d_coef, size_t coef_frame_stride, size_t nframes, int width, int height,
                       int quality, int restart_rows, unsigned jfif_flags, uint8_t *d_out,
                       size_t out_frame_stride, size_t out_cap, uint64_t *d_len,
                       void *d_workspace, size_t workspace_bytes, void *stream);
/* k_gray's fp32 scales and guard band limits of `quality`, [v * 8 + u] for coefficient (row v, column
 * u): as jpgx_guard_band, from the sample bound [-128, 127].  JPGX_EQUALITY, JPGX_EARG (null). */
int jpgx_guard_band_gray(int quality, float scale[64], float lim[64]);

/* The two tables exactly as the JFIF writers put them into DQT for `quality` (the divisors the
 * forward path applied, zig-zag order): jpgx_blocks_gpu's output can be turned into pixels without
 * writing a file.  JPGX_EQUALITY outside 1..97, JPGX_EARG for a null qt. */
int jpgx_jfif_qt(int quality, uint16_t qt[2][64]);

/* Synthetic frames, generated directly in device memory (SURVEY.md 8c generator G: byte k
 * of the buffer = splitmix64(seed + (k+1)*0x9E3779B97F4A7C15) >> 56). */
int jpgx_gen_splitmix_gpu(uint8_t *d_dst, size_t nbytes, uint64_t seed, void *stream);
/* Tie frame T: flat gray 8x8 blocks, v = 97 + 2*(block_index % 40), R=G=B. */
int jpgx_gen_tie_gpu(uint8_t *d_dst, int width, int height, void *stream);

/* ---- host-buffer path (synchronous; csrc/jpgx_host.cpp) ------------------------------ */

/* A host-buffer context: the image is cut into `nshards` balanced block-row shards
 * (jpgx_stripe; MCU-row pairs for true 4:2:0), shard k runs on GPU devices[k] (NULL: k modulo
 * the device count; several shards may name the same GPU), one host thread per shard, no
 * communication between shards (each reads the pixel row above its first block row as halo and
 * writes a disjoint range of the output).  A shard streams its rows through the device in
 * chunks of `chunk_rows` block rows (0: about 4 MB of RGB per chunk), two chunks in flight on
 * two streams, so one chunk's H2D overlaps the previous chunk's D2H.  Device chunk buffers,
 * streams, events and pinned staging buffers are allocated on first use, grown when an image
 * needs more, and kept until jpgx_host_destroy.  Pageable caller buffers are staged through
 * the pinned buffers (host copies overlapped with the DMA); page-locked ones (hipHostMalloc,
 * jpgx_host_register) are copied directly.  A context is used by one call at a time. */
typedef struct jpgx_host_ctx jpgx_host_ctx;
int jpgx_host_create(jpgx_host_ctx **ctx, int nshards, const int *devices, int chunk_rows);
void jpgx_host_destroy(jpgx_host_ctx *ctx);

/* Whole image in host memory (pixel rows `pitch` bytes apart) -> host int16 output laid out as
 * jpgx_blocks_gpu's frame output ([3][nb][64], or Y | Cb | Cr with JPGX_FLAG_SUBSAMPLE). */
int jpgx_host_blocks(jpgx_host_ctx *ctx, const uint8_t *rgb, int width, int height, size_t pitch,
                     const jpgx_params *p, int16_t *out);

/* Page-lock (hipHostRegister, portable) / release a caller buffer so that jpgx_host_blocks
 * DMAs it directly. */
int jpgx_host_register(void *ptr, size_t bytes);
int jpgx_host_unregister(void *ptr);

/* Frees the pooled contexts behind jpgx_blocks / jpgx_blocks_multi. */
void jpgx_host_release(void);

/* Whole image on GPU `device` (a pooled one-shard context). */
int jpgx_blocks(const uint8_t *rgb, int width, int height, size_t pitch, const jpgx_params *p,
                int16_t *out, int device);

/* Same, sharded into ngpus block-row stripes on GPUs 0..ngpus-1 (a pooled context). */
int jpgx_blocks_multi(const uint8_t *rgb, int width, int height, size_t pitch,
                      const jpgx_params *p, int16_t *out, int ngpus);

/* Block-row stripe bounds of shard k of n (balanced, contiguous). */
void jpgx_stripe(int block_rows, int nshards, int k, int *row_begin, int *row_end);

/* Number of visible GPUs (0 if none). */
int jpgx_device_count(void);

/* Library version string. */
const char *jpgx_version(void);

#ifdef __cplusplus
}
#endif
#endif
