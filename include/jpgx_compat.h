/*
 * jpgx_compat.h -- the reference-compatible host API of libjpgx.so (C99, host code).
 *
 * The drop-in surface a user of matthewT53/JPEG-Encoder-and-Decoder keeps while the batched
 * hot path runs on the GPU (jpgx.h):
 *
 *   1. Block API with the reference's semantics, one 8x8 block of doubles at a time
 *      (src/headers/block.h:10-40, src/block.c:15-67; src/dct.c:36-59; src/quantise.c:52-86;
 *      src/zig_zag.c:48-58).  jpgx_block has the reference's struct _block layout, so the
 *      pointers are interchangeable.  These are per-block CPU calls for API compatibility and
 *      small jobs -- the throughput path is jpgx_blocks_gpu().
 *   2. A JpgData adapter: struct jpgx_jpeg_data has the field order and types of the
 *      reference's JpegData (src/headers/jpg_encode.h:21-70), and jpgx_fill_jpgdata() widens
 *      the GPU's int16 [3][nb][64] output into its zig_zag_Y/Cb/Cr int** arrays exactly as
 *      zig_zag() allocates them (src/zig_zag.c:24-32), so an unmodified dpcm()-style consumer
 *      (src/dpcm.c:6-21) works on it.
 *   3. Host stitch of the DC recurrence (src/dpcm.c:6-21) over the int16 layout, with a
 *      carry so that block-row stripes computed on different GPUs stitch exactly.
 *   4. The BMP reader (src/bitmap.c:41-152 semantics) and the stage sequence of
 *      encode_bmp_to_jpeg() up to the entropy stage (src/jpg_encode.c:19-47).
 *
 * Differences from the reference, all deliberate: functions report errors through return
 * codes (the reference returns void); zig-zag does not print one line per block
 * (src/zig_zag.c:21,50); nothing leaks (the reference never frees JpgData).
 */
#ifndef JPGX_COMPAT_H
#define JPGX_COMPAT_H

#include <stddef.h>
#include <stdint.h>

#include "jpgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. Block API ------------------------------------------------------------------------ */

/* src/block.c:15-17: 64 doubles, index y*8+x */
typedef struct jpgx_block {
    double values[64];
} jpgx_block;
typedef jpgx_block *jpgx_Block;

jpgx_Block jpgx_new_block(void);                                /* block.c:20-23   */
double jpgx_get_value_block(jpgx_Block b, int x, int y);       /* block.c:25-28   */
void jpgx_set_value_block(jpgx_Block b, int x, int y, double v); /* block.c:30-33 */
jpgx_Block jpgx_copy_block(jpgx_Block b);                       /* block.c:35-48   */
void jpgx_show_block(jpgx_Block b);                             /* block.c:50-62   */
void jpgx_destroy_block(jpgx_Block b);                          /* block.c:64-67   */

/* In-place forward DCT-II, the reference's exact operation order and double arithmetic
 * (dct.c:36-59): F(u,v) stored at get(b,u,v) = values[v*8+u]. */
void jpgx_dct_block(jpgx_Block b);

/* values[j*8+i] = round(values[j*8+i] / table[i][j]) -- the reference's transposed use of the
 * table (quantise.c:52-72), with an explicit table (reentrant). */
void jpgx_quantise_block(jpgx_Block b, const int table[8][8]);

/* Legacy global-table variants (quantise.c:8-26,52-72): they read jpgx_q_table_lum/chr, which
 * start as the base tables and are rescaled in place by jpgx_scale_table_inplace(), as the
 * reference's quantise() does (quantise.c:34-35; a second call rescales again).  Not
 * reentrant, by the reference's design; prefer jpgx_quantise_block(). */
extern int jpgx_q_table_lum[8][8];
extern int jpgx_q_table_chr[8][8];
void jpgx_quantise_lum(jpgx_Block b);
void jpgx_quantise_chr(jpgx_Block b);
/* quantise.c:74-86, in place, no validation (q outside [1,97] gives the reference's zeros) */
void jpgx_scale_table_inplace(int table[8][8], int quality);

/* zz[scan_order[i][j]] = (int) get(b, j, i)  (zig_zag.c:48-58) */
void jpgx_zig_zag_block(jpgx_Block b, int *zz);

/* ---- 2. JpgData adapter ------------------------------------------------------------------ */

/* src/headers/jpg_encode.h:21-34 */
typedef struct jpgx_huffman_data {
    int freq[257];
    int code_len[257];
    int others[257];
    int bits[32];
    int huffval[256];
} jpgx_huffman_data;

/* src/headers/jpg_encode.h:36-70, field for field */
typedef struct jpgx_jpeg_data {
    char *output_filename;
    char *input_filename;
    int width;
    int height;
    int sample_ratio;
    int quality;
    int num_blocks_Y;
    int num_blocks_Cb;
    int num_blocks_Cr;
    jpgx_Block *Y;
    jpgx_Block *Cb;
    jpgx_Block *Cr;
    int **zig_zag_Y;
    int **zig_zag_Cb;
    int **zig_zag_Cr;
    jpgx_huffman_data lum_DC;
    jpgx_huffman_data lum_AC;
    jpgx_huffman_data chrom_DC;
    jpgx_huffman_data chrom_AC;
} jpgx_jpeg_data;
typedef jpgx_jpeg_data *jpgx_JpgData;

/* j->width, j->height must be set (multiples of 8) and zig_zag_Y/Cb/Cr must be NULL (a filled
 * JpgData is released with jpgx_free_jpgdata first).  Allocates zig_zag_* as zig_zag() does
 * (an int* array of int[64], zig_zag.c:24-32), widens coef [3][nb][64] into it and then sets
 * num_blocks_* = (W/8)(H/8) (preprocess.c:45-47).  Returns 0, JPGX_EARG, or JPGX_ENOMEM
 * (then j is unchanged). */
int jpgx_fill_jpgdata(jpgx_JpgData j, const int16_t *coef);
/* frees what jpgx_fill_jpgdata allocated (zig_zag_*), leaves the rest */
void jpgx_free_jpgdata(jpgx_JpgData j);
/* dpcm.c:6-21 on j->zig_zag_*, in place */
void jpgx_dpcm(jpgx_JpgData j);

/* ---- 3. DC recurrence over the int16 layout ---------------------------------------------- */

/* dc[c][i] for channel c, block i of a run of nb blocks of coef [3][nb][64]:
 *   dc[c][0] = coef[c][0][0] - carry[c],  dc[c][i] = coef[c][i][0] - dc[c][i-1]
 * i.e. dpcm.c:10-20 (which reads the already-updated previous entry).  For a whole frame
 * carry = 0 and dc[c][0] = coef[c][0][0] (the reference leaves block 0 as is); for the
 * stripe starting at block s, carry = the previous stripe's last dc.  int32 output: the
 * recurrence is an alternating sum and can leave the int16 range.  Returns 0 / JPGX_EARG. */
int jpgx_dpcm_dc(const int16_t *coef, size_t nb, const int32_t carry[3], int32_t *dc);

/* ---- 4. BMP input and the encode stage sequence ------------------------------------------ */

/* Reads a BMP with the reference loader's semantics (bitmap.c:41-152): width/height/bit depth
 * from header offsets 18/22/28; pixel row i (top-down) taken from file offset
 * fs - (i+1)*W*(bpp/8) (the file is read backwards from its end, offsetRGB and row padding
 * ignored); stored byte order kept (byte 0 of a triple is the reference's "red").
 * Output: *rgb = malloc'd interleaved top-down W*H*3 bytes (free with jpgx_free), *file_size
 * = the file size (it sets the underflow bytes, jpgx_glibc_underflow).
 * Returns 0, JPGX_EARG (unreadable / not 24-bit / too short). */
int jpgx_bmp_read(const char *path, uint8_t **rgb, int *width, int *height, size_t *file_size);
void jpgx_free(void *p);

/* encode_bmp_to_jpeg() up to the entropy stage (jpg_encode.c:19-47): read the BMP, run the
 * block transform on GPU `device`, widen into *j (jpgx_fill_jpgdata) and, if do_dpcm, apply
 * dpcm.  Fills width/height/sample_ratio/quality.  Geometry rules as jpgx_validate(); the
 * underflow bytes follow the glibc model for this file (jpgx_glibc_underflow). */
int jpgx_encode_bmp(const char *path, int quality, int sample_ratio, int device, int do_dpcm,
                    jpgx_JpgData j);

/* ---- 5. Entropy stage: a baseline JFIF writer (the build's own; the reference's Huffman stage
 *         never terminates, src/huffman.c:23-235, so this has no reference to match) --------- */

/* Upper bound of the file size jpgx_write_jfif can produce for a width x height image. */
size_t jpgx_jfif_bound(int width, int height);

/* Baseline sequential JFIF (8-bit, one interleaved scan, 4:4:4, ITU-T T.81 Annex K.3 Huffman
 * tables, true DC prediction) of coef [3][nb][64] (zig-zag, raster blocks).  The DQT holds the
 * divisors the reference applied (its scaled tables, transposed: src/quantise.c:58), so a
 * standard decoder reproduces the reference's coefficients' image.  Returns 0, JPGX_EARG
 * (geometry, or cap too small: *len is then the size needed), JPGX_EQUALITY. */
int jpgx_write_jfif(const int16_t *coef, int width, int height, int quality, uint8_t *out,
                    size_t cap, size_t *len);

/* The same for coef = Y [nb][64] | Cb [nbc][64] | Cr [nbc][64] with sample_ratio 1 (true 4:2:2,
 * Y sampled 2x1, MCU = 2 Y + Cb + Cr) or 2 (true 4:2:0, 2x2, MCU = 4 Y + Cb + Cr), the layout
 * JPGX_FLAG_SUBSAMPLE produces; sample_ratio 0 is jpgx_write_jfif. */
int jpgx_write_jfif_sub(const int16_t *coef, int width, int height, int quality,
                        int sample_ratio, uint8_t *out, size_t cap, size_t *len);

/* The same with restart intervals, coded on host threads: `restart_rows` MCU rows per interval
 * (0: none, the single-interval stream of jpgx_write_jfif_sub; -1: about four intervals per
 * thread; the interval, rows x MCUs per row, must fit DRI's 16 bits), a DRI segment, DC
 * predictors reset and an RSTm marker at every interval boundary (T.81 F.1.2.1.3, B.2.4.4);
 * `nthreads` threads (0: one per online CPU, at most 64) code contiguous runs of intervals
 * into their own buffers, concatenated in order -- e.g. the 8 GPU stripes of a 16384^2 frame.
 * Returns as jpgx_write_jfif_sub, or JPGX_ENOMEM. */
int jpgx_write_jfif_ex(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                       int restart_rows, int nthreads, uint8_t *out, size_t cap, size_t *len);

/* The same with jfif_flags (include/jpgx.h).  0: jpgx_write_jfif_ex.  JPGX_JFIF_OPTIMIZE: the four
 * DHT segments hold tables built by T.81 Annex K.2 from the image's own symbol counts (one
 * counting pass over the coefficients on the same threads) and the scan is coded with them; the
 * rest of the file is unchanged and it is never longer than the K.3 header allows for.  The bytes
 * do not depend on `nthreads` for a fixed restart_rows >= 0 (-1, auto, chooses the interval from
 * the thread count, as in jpgx_write_jfif_ex).  Unknown flag bits: JPGX_EARG. */
int jpgx_write_jfif_opt(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                        int restart_rows, int nthreads, unsigned jfif_flags, uint8_t *out,
                        size_t cap, size_t *len);

/* jpgx_write_jfif_opt for a file of any width and height, 1 .. 65535 each: coef holds
 * the coded frame's blocks -- the size rounded up to the MCU of sample_ratio (jpgx_coded_size), what
 * jpgx_blocks_gpu_any writes and jpgx_read_jfif_any returns -- all of which are coded; SOF states
 * width x height; the restart interval counts MCUs of the coded frame.  Byte for byte the file is
 * jpgx_write_jfif_opt's for the coded size with the four size bytes of SOF replaced, and for a size
 * that is a multiple of the MCU it is that file.  jpgx_jfif_bound(coded width, coded height) bounds
 * its size.  JPGX_EARG for a sample_ratio outside 0 .. 2 or a side outside 1 .. 65535;
 * JPGX_EGEOMETRY does not occur; everything else as jpgx_write_jfif_opt. */
int jpgx_write_jfif_any(const int16_t *coef, int width, int height, int quality, int sample_ratio,
                        int restart_rows, int nthreads, unsigned jfif_flags, uint8_t *out,
                        size_t cap, size_t *len);

/* jpgx_write_jfif_opt for a one-component (grayscale) file of any width and height, 1 .. 65535 each
 * (include/jpgx.h: the encode side of the one-component family): coef holds Y [nb][64],
 * nb = ceil(width / 8) * ceil(height / 8) blocks in raster order -- what jpgx_blocks_gpu_gray writes
 * and jpgx_read_jfif_gray returns.  The file: SOI, jpgx_write_jfif's APP0, one DQT (table 0,
 * jpgx_jfif_qt(quality)[0]), SOF0 with Nf = 1 (component 1, sampling 0x11, Tq 0; SOF1 and a 16-bit table
 * for q <= 23), DHT DC 0x00 and AC 0x10 only -- the K.3 luminance tables or, with JPGX_JFIF_OPTIMIZE,
 * the image's own by Annex K.2, counted over these two tables alone -- DRI when there are intervals,
 * SOS with Ns = 1, the scan, EOI.  restart_rows counts block rows (0 none, -1 auto as in
 * jpgx_write_jfif_ex) and DRI counts blocks: rows x ceil(width / 8) must fit 16 bits.  Luminance never
 * reaches the coder's clamps (|AC| <= 1020, |DC difference| <= 2040 at q 97), so reading the file back
 * returns coef for every input.  The threading contract is jpgx_write_jfif_opt's: the bytes do not
 * depend on nthreads for restart_rows >= 0.  jpgx_jfif_bound(8 bw, 8 bh) bounds the file.  JPGX_EARG for
 * a side outside 1 .. 65535, the interval, unknown flags and null pointers, JPGX_EQUALITY, JPGX_ENOMEM,
 * and JPGX_EARG with *len = the size needed when cap is too small, as jpgx_write_jfif_opt. */
int jpgx_write_jfif_gray(const int16_t *coef, int width, int height, int quality, int restart_rows,
                         int nthreads, unsigned jfif_flags, uint8_t *out, size_t cap, size_t *len);

/* The edge rule of the encode side's _any entry points, on the host: out, coded_height rows of
 * 3 coded_width bytes, is the width x height image rgb (rows `pitch` >= 3 width bytes apart) with its
 * last column repeated to the right and its last row repeated downwards -- numpy's
 * np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)), mode="edge").  This is the project's own rule, not
 * libjpeg's (which fills the blocks beyond a component's width with a DC-only copy of the block
 * before); decoders crop to SOF's size, so the file is valid either way.  JPGX_EARG: null pointers,
 * pitch below 3 width; JPGX_EGEOMETRY: a side <= 0 or a coded side below the image's. */
int jpgx_pad_edge(const uint8_t *rgb, int width, int height, size_t pitch, int coded_width,
                  int coded_height, uint8_t *out);

/* ---- 6. The way back: a baseline JFIF file's coefficients (entropy decoding only) ------------- */

typedef struct jpgx_jfif_info {
    int width, height, sample_ratio;    /* 0: 4:4:4, 1: 4:2:2, 2: 4:2:0                        */
    unsigned restart_interval;          /* DRI's MCUs per interval, 0: none                    */
    size_t scan_offset, nb_y, nb_c;     /* the first entropy-coded byte; blocks of Y, of Cb    */
} jpgx_jfif_info;

/* The header walk alone (SOI .. SOS).  Returns 0, JPGX_EARG (null pointers), JPGX_EJFIF_HEADER. */
int jpgx_jfif_info_of(const uint8_t *file, size_t len, jpgx_jfif_info *info);

/* The quantised coefficients of a baseline JFIF file, in the layout the writers above take:
 * [3][nb][64] for 4:4:4, Y [nb][64] | Cb [nbc][64] | Cr [nbc][64] for 4:2:2 / 4:2:0 (zig-zag,
 * raster blocks) -- what jpgx_write_jfif* were given wherever that was inside their clamps.
 * Reads baseline SOF0 (SOF1 with 8-bit samples), three components in one interleaved scan, luma
 * sampled 1x1, 2x1 or 2x2 and chroma 1x1 (Cb and Cr sharing a quantisation table), width and
 * height multiples of the MCU, DQT with 8- or 16-bit entries, DHT ids 0 and 1, DRI; skips APPn and
 * COM; everything else, a file shorter than its header included: JPGX_EJFIF_HEADER.
 * The restart intervals are found by their markers (FF D0 .. D7 cannot occur inside entropy-coded
 * data) and decoded on `nthreads` threads (0: one per online CPU, at most 64); the result does
 * not depend on the thread count.  A file without DRI is one interval.  JPGX_EJFIF_SCAN: the
 * markers are not (intervals - 1) in number or not numbered k mod 8, EOI does not end the file, or
 * an interval does not decode to exactly its MCUs (a code that is in no table, a coefficient past
 * index 63, a DC size above 11 or an AC size above 10, a DC outside int16, bytes that run out or
 * are left over).  The bytes are untrusted: no read leaves [file, file + len), no write leaves the
 * frame's coefficients.  coef_cap: int16 elements at coef, at least (nb + 2 nbc) * 64, else
 * JPGX_EARG (*info is then filled, so the size can be asked for with coef_cap 0 and a non-null
 * coef).  qt (may be NULL): Y's table, then the chroma table, zig-zag order as in the file.  info
 * (may be NULL): filled whenever the header was accepted. */
int jpgx_read_jfif(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap,
                   uint16_t qt[2][64], jpgx_jfif_info *info);

/* The host twin of the device decoder that works inside a restart interval (include/jpgx.h:
 * JPGX_JFIF_DECODE_SUBINTERVAL).  It runs the routines the kernel runs
 * (csrc/jx_jfif_sub.h), lane after lane, round after round and tile after tile, on one thread: an
 * interval's bytes cut into subsequences of sub_bytes bytes and tiles of tile_subs subsequences
 * (sub_bytes >= 16, tile_subs >= 2, their product at most 2^24, else JPGX_EARG; 0, 0: the kernel's
 * shape, jpgx_jfif_decode_sub_shape).  Arguments, outputs and returns are jpgx_read_jfif's, for
 * every input and every shape.  stats (may be NULL) counts what the mechanism did. */
typedef struct jpgx_jfif_sub_stats {
    uint64_t subsequences, tiles, /* decoded; loaded                                              */
        rounds_max,               /* the most rounds a tile took before no lane changed its entry */
        redecodes,                /* subsequences decoded again in a round                        */
        wrong_first_guesses,      /* lanes whose guess did not lead to the exit state they ended with */
        starts_on_stuffing,       /* guesses moved off a stuffed 00                               */
        units_across_sub,         /* units whose last bit lies past their subsequence ...         */
        units_across_tile;        /* ... and past their tile                                      */
} jpgx_jfif_sub_stats;
int jpgx_read_jfif_sub(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs,
                       int16_t *coef, size_t coef_cap, uint16_t qt[2][64], jpgx_jfif_info *info,
                       jpgx_jfif_sub_stats *stats);

/* The host twin of jpgx_pixels_gpu (include/jpgx.h): one frame's coefficients, in
 * the layout jpgx_read_jfif returns, and its two zig-zag tables -> interleaved top-down RGB rows
 * `pitch` bytes apart (only bytes [0, 3 width) of a row are written).  The same arithmetic from the
 * same source (csrc/jx_idct.h): libjpeg's default decoder's pixels.  Runs over MCU rows on
 * `nthreads` threads (0: one per online CPU, at most 64); the result does not depend on the thread
 * count.  Returns 0, JPGX_EARG (null pointers, pitch < 3 width, nthreads < 0), JPGX_ESAMPLE,
 * JPGX_EGEOMETRY, JPGX_ENOMEM. */
int jpgx_pixels_host(const int16_t *coef, int width, int height, int sample_ratio,
                     const uint16_t qt[2][64], uint8_t *rgb, size_t pitch, int nthreads);

/* Files of any width and height (include/jpgx.h: the _any family): each of the four
 * takes its sibling's arguments and keeps its sibling's contract without "width and height multiples
 * of the MCU" -- any width and height in 1 .. 65535.  info.width / height are the SOF's; nb_y / nb_c
 * and the coefficients are the coded frame's, the size rounded up to the MCU (jpgx_coded_size),
 * every block of which the file codes.  jpgx_read_jfif_sub_any is the host twin of the device
 * decoder's kernel as jpgx_read_jfif_sub is.  jpgx_pixels_host_any takes the coded frame's
 * coefficients and the visible width and height and writes bytes [0, 3 width) of rows [0, height):
 * libjpeg's default decoder's pixels for a file of that size -- the chroma upsampling clamps at the
 * component's real extent and replicates a row of two samples or fewer, so they are
 * not a crop of the coded frame's pixels; a side outside 1 .. 65535 is JPGX_EGEOMETRY.  For a size
 * that is a multiple of the MCU every output and return equals the sibling's. */
int jpgx_jfif_info_of_any(const uint8_t *file, size_t len, jpgx_jfif_info *info);
int jpgx_read_jfif_any(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap,
                       uint16_t qt[2][64], jpgx_jfif_info *info);
int jpgx_read_jfif_sub_any(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs,
                           int16_t *coef, size_t coef_cap, uint16_t qt[2][64], jpgx_jfif_info *info,
                           jpgx_jfif_sub_stats *stats);
int jpgx_pixels_host_any(const int16_t *coef, int width, int height, int sample_ratio,
                         const uint16_t qt[2][64], uint8_t *rgb, size_t pitch, int nthreads);

/* One-component (grayscale) baseline files (include/jpgx.h: the _gray family).  Accepted:
 * SOF0, or SOF1 with 8-bit samples, with ONE component (any id, Tq <= 3, sampling factors 1 .. 4
 * each, which are ignored: the scan is not interleaved, so its MCU is one block whatever SOF says,
 * T.81 A.2.2) and one scan of that component (Td, Ta <= 1, Ss 0, Se 63, Ah / Al 0); DQT, DHT, DRI,
 * APPn and COM as for jpgx_read_jfif, only the tables the component selects need to be there; any
 * width and height in 1 .. 65535.  Everything else, a three-component file included, is
 * JPGX_EJFIF_HEADER.  The file codes nb = ceil(width / 8) * ceil(height / 8) blocks in raster order;
 * DRI counts blocks, and an interval may begin and end inside a block row.
 * info: the SOF's width and height, sample_ratio 0, nb_y = nb, nb_c = 0, restart_interval in blocks.
 * coef: Y [nb][64], zig-zag; coef_cap at least nb * 64.  qt: the component's table, zig-zag order.
 * jpgx_read_jfif_gray keeps jpgx_read_jfif_any's contract and return codes otherwise, and
 * jpgx_read_jfif_sub_gray, the host twin of the device decoder's one-component kernel, returns what
 * jpgx_read_jfif_gray returns for every input and every shape.
 * jpgx_pixels_host_gray: libjpeg's default decoder's pixels of such a frame, `channels` bytes per
 * pixel: 1 is the range-limited inverse DCT's sample (JCS_GRAYSCALE), 3 is that sample as R = G = B
 * (libjpeg's gray-to-RGB).  Writes bytes [0, channels * width) of rows [0, height), `pitch` bytes
 * apart.  JPGX_EARG: null pointers, channels other than 1 and 3, pitch < channels * width,
 * nthreads < 0; JPGX_EGEOMETRY: a side outside 1 .. 65535. */
int jpgx_jfif_info_of_gray(const uint8_t *file, size_t len, jpgx_jfif_info *info);
int jpgx_read_jfif_gray(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap,
                        uint16_t qt[64], jpgx_jfif_info *info);
int jpgx_read_jfif_sub_gray(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs,
                            int16_t *coef, size_t coef_cap, uint16_t qt[64], jpgx_jfif_info *info,
                            jpgx_jfif_sub_stats *stats);
int jpgx_pixels_host_gray(const int16_t *coef, int width, int height, const uint16_t qt[64],
                          uint8_t *out, size_t pitch, int channels, int nthreads);

/* The host twins of jpgx_pixels_gpu_scaled and jpgx_pixels_gpu_gray_scaled (include/jpgx.h; DESIGN.md
 * 4.9b): libjpeg-turbo's default decoder's pixels with scale_num / scale_denom = 1 / scale_denom, from
 * the same source (csrc/jx_idct.h).  jpgx_pixels_host_any's and jpgx_pixels_host_gray's arguments and
 * contracts with scale_denom, 1, 2, 4 or 8, after sample_ratio (after height for the one-component
 * frame): the coefficients are the coded frame's, width and height the file's, and bytes
 * [0, bytes per pixel * ow) of rows [0, oh) are written, ow x oh = ceil(width / scale_denom) x
 * ceil(height / scale_denom).  scale_denom 1 is the sibling's call.  JPGX_EARG: the sibling's cases with
 * the pitch measured against ow, and any other scale_denom. */
int jpgx_pixels_host_scaled(const int16_t *coef, int width, int height, int sample_ratio, int scale_denom,
                            const uint16_t qt[2][64], uint8_t *rgb, size_t pitch, int nthreads);
int jpgx_pixels_host_gray_scaled(const int16_t *coef, int width, int height, int scale_denom,
                                 const uint16_t qt[64], uint8_t *out, size_t pitch, int channels,
                                 int nthreads);

/* encode_bmp_to_jpeg with flags: JPGX_FLAG_SUBSAMPLE and sample_ratio 1/2 write a truly
 * subsampled JFIF (extension); otherwise exactly jpgx_encode_bmp_to_jpeg.  GPU `device`. */
int jpgx_encode_bmp_to_jpeg_ex(const char *input, const char *output, int quality,
                               int sample_ratio, unsigned flags, int device);

/* The reference's declared in-memory entry point (src/headers/jpg_encode.h:99,
 * encode_rgb_to_jpeg(Byte *colours, output, quality, sample_ratio); declared, never defined
 * there, and without the image size, which this one takes): interleaved top-down RGB rows
 * `pitch` bytes apart -> the block transform on GPU `device` -> a JFIF file at `output`
 * (truly subsampled with JPGX_FLAG_SUBSAMPLE and sample_ratio 1/2).  The x0 = -8 underflow
 * bytes are jpgx_default_params's (those of a 54-byte-header BMP of this size).  Returns 0 or a
 * JPGX_E* code. */
int jpgx_encode_rgb_to_jpeg(const uint8_t *rgb, int width, int height, size_t pitch,
                            const char *output, int quality, int sample_ratio, unsigned flags,
                            int device);

/* The same for an image of any width and height, 1 .. 65535 each: the coded frame by the edge rule
 * (jpgx_pad_edge, into a staging buffer), jpgx_blocks over it with the coded size's default
 * parameters, jpgx_write_jfif_any.  The coded frame is that of the file's sampling: sample_ratio with
 * JPGX_FLAG_SUBSAMPLE, 0 (4:4:4, MCU 8 x 8) without.  JPGX_ESAMPLE, JPGX_EQUALITY, JPGX_EGEOMETRY (a
 * side outside 1 .. 65535), JPGX_EARG (null pointers, pitch below 3 width) before any work. */
int jpgx_encode_rgb_to_jpeg_any(const uint8_t *rgb, int width, int height, size_t pitch,
                                const char *output, int quality, int sample_ratio, unsigned flags,
                                int device);

/* The reference's public entry point (src/headers/jpg_encode.h:85): BMP in, JPEG file out --
 * the block transform on GPU 0, then jpgx_write_jfif.  Returns 0 or a JPGX_E* code. */
int jpgx_encode_bmp_to_jpeg(const char *input, const char *output, int quality,
                            int sample_ratio);

#ifdef __cplusplus
}
#endif

#endif
