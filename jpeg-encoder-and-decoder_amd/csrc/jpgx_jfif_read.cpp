/*
 * jpgx_jfif_read.cpp -- the host decoder of baseline JFIF files back to the coefficient layout
 * (DESIGN.md 4.8): jpgx_jfif_info_of, jpgx_read_jfif, their _any siblings for files of any width and
 * height and their _gray siblings for one-component files, and jpgx_coded_size (include/jpgx_compat.h, include/jpgx.h).  The routines are
 * those of jx_jfif_dec.h, the ones the device decoder (jpgx_jfif_dec.hip) runs; this file adds the
 * search for the restart markers and the threads.  No HIP: built with g++, as jpgx_plan.cpp.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/jpgx_compat.h"
#include "jx_jfif_dec.h"
#include "jx_jfif_sub.h"
#include "jx_par.h"

namespace {

struct Job {
    const uint8_t *file;
    size_t len;
    const jxd_frame *fr;
    const jxd_tab *tabs;
    const size_t *marks;                /* [ni - 1] the restart markers' places */
    int16_t *coef;
    int gray;                           /* the one-component frame */
    int rc[JX_PAR_MAX];                 /* per thread */
};

/* the header walk's modes (jx_jfif_dec.h) */
enum { kPlain, kAny, kGray };

/* thread t's intervals (jx_par.h) */
void run(void *ctx, uint32_t t, uint64_t iv0, uint64_t iv1)
{
    Job *j = (Job *)ctx;
    const jxd_frame *fr = j->fr;
    for (uint32_t iv = (uint32_t)iv0; iv < (uint32_t)iv1; iv++) {
        const size_t begin = iv ? j->marks[iv - 1] + 2 : (size_t)fr->scan_off;
        const size_t end = iv + 1 < fr->ni ? j->marks[iv] : j->len - 2;
        const uint32_t mcu0 = iv * fr->mpi;
        const uint32_t count = fr->nmcu - mcu0 < fr->mpi ? fr->nmcu - mcu0 : fr->mpi;
        const int rc = j->gray ? jxd_decode_interval_gray(j->file, j->len, begin, end, fr, j->tabs, mcu0, count, j->coef)
                               : jxd_decode_interval(j->file, j->len, begin, end, fr, j->tabs, mcu0, count, j->coef);
        if (rc) j->rc[t] = JPGX_EJFIF_SCAN;
    }
}

void fill_info(const jxd_frame &fr, jpgx_jfif_info *info)
{
    info->width = (int)fr.width;
    info->height = (int)fr.height;
    info->sample_ratio = jxd_sample_ratio(&fr);
    info->restart_interval = fr.ri;
    info->scan_offset = (size_t)fr.scan_off;
    info->nb_y = fr.nb;
    info->nb_c = fr.nbc;
}

/* the header walk in one of its modes */
int parse(int mode, const uint8_t *file, size_t len, jxd_frame *fr, jxd_tab *tabs)
{
    return mode == kGray ? jxd_parse_header<1, 1>(file, len, fr, tabs)
           : mode == kAny ? jxd_parse_header<1>(file, len, fr, tabs) : jxd_parse_header<0>(file, len, fr, tabs);
}

/* the tables the caller gets: Y's and the chroma's, or the one-component frame's one */
void copy_qt(int mode, const jxd_frame &fr, uint16_t *qt)
{
    if (qt) memcpy(qt, fr.qt, mode == kGray ? sizeof fr.qt[0] : sizeof fr.qt);
}

/* the restart markers: FF D0 .. D7 cannot occur inside entropy-coded data.  Their count must be the
 * intervals' less one, their numbers run k mod 8, and EOI ends the file.  marks: [ni - 1] */
int find_marks(const uint8_t *file, size_t len, const jxd_frame *fr, size_t *marks)
{
    const size_t scan = (size_t)fr->scan_off;
    size_t found = 0;
    if (!jxd_has_eoi(file, len, scan)) return JPGX_EJFIF_SCAN;
    for (size_t p = scan; p + 1 < len; p++) {
        if (!jxd_is_rst(file, len, scan, p)) continue;
        if (found >= fr->ni - 1 || (file[p + 1] & 7u) != (found & 7u)) return JPGX_EJFIF_SCAN;
        marks[found++] = p;
    }
    return found != fr->ni - 1 ? JPGX_EJFIF_SCAN : 0;
}

int info_of(int mode, const uint8_t *file, size_t len, jpgx_jfif_info *info)
{
    if (!file || !info) return JPGX_EARG;
    jxd_frame fr;
    jxd_tab *tabs = (jxd_tab *)malloc(4 * sizeof(jxd_tab));
    if (!tabs) return JPGX_ENOMEM;
    memset(&fr, 0, sizeof fr);
    const int rc = parse(mode, file, len, &fr, tabs);
    free(tabs);
    if (rc) return rc;
    fill_info(fr, info);
    return JPGX_OK;
}

int read_jfif(int mode, const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap, uint16_t *qt,
              jpgx_jfif_info *info)
{
    if (!file || !coef || nthreads < 0) return JPGX_EARG;
    jxd_frame fr;
    memset(&fr, 0, sizeof fr);
    jxd_tab *tabs = (jxd_tab *)malloc(4 * sizeof(jxd_tab));
    if (!tabs) return JPGX_ENOMEM;
    int rc = parse(mode, file, len, &fr, tabs);
    if (rc) {
        free(tabs);
        return rc;
    }
    if (info) fill_info(fr, info);
    copy_qt(mode, fr, qt);
    if (coef_cap < (size_t)fr.nblk * 64) {
        free(tabs);
        return JPGX_EARG;
    }
    size_t *marks = (size_t *)malloc((fr.ni > 1 ? fr.ni - 1 : 1) * sizeof(size_t));
    if (!marks) {
        free(tabs);
        return JPGX_ENOMEM;
    }
    rc = find_marks(file, len, &fr, marks);
    if (!rc) {
        Job j = {file, len, &fr, tabs, marks, coef, mode == kGray, {0}};
        jx_par_run(fr.ni, jx_thread_count(nthreads), run, &j);
        for (uint32_t t = 0; t < JX_PAR_MAX; t++)
            if (j.rc[t]) rc = j.rc[t];
    }
    free(marks);
    free(tabs);
    return rc;
}

}  // namespace

extern "C" {

int jpgx_jfif_info_of(const uint8_t *file, size_t len, jpgx_jfif_info *info) { return info_of(kPlain, file, len, info); }

int jpgx_jfif_info_of_any(const uint8_t *file, size_t len, jpgx_jfif_info *info) { return info_of(kAny, file, len, info); }

int jpgx_jfif_info_of_gray(const uint8_t *file, size_t len, jpgx_jfif_info *info) { return info_of(kGray, file, len, info); }

int jpgx_read_jfif(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap, uint16_t qt[2][64],
                   jpgx_jfif_info *info)
{
    return read_jfif(kPlain, file, len, nthreads, coef, coef_cap, (uint16_t *)qt, info);
}

int jpgx_read_jfif_any(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap, uint16_t qt[2][64],
                       jpgx_jfif_info *info)
{
    return read_jfif(kAny, file, len, nthreads, coef, coef_cap, (uint16_t *)qt, info);
}

int jpgx_read_jfif_gray(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap, uint16_t qt[64],
                        jpgx_jfif_info *info)
{
    return read_jfif(kGray, file, len, nthreads, coef, coef_cap, qt, info);
}

int jpgx_coded_size(int width, int height, int sample_ratio, int *coded_width, int *coded_height)
{
    if (!coded_width || !coded_height || sample_ratio < 0 || sample_ratio > 2) return JPGX_EARG;
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return JPGX_EARG;
    const int mw = sample_ratio ? 16 : 8, mh = sample_ratio == 2 ? 16 : 8;
    *coded_width = (width + mw - 1) / mw * mw;
    *coded_height = (height + mh - 1) / mh * mh;
    return JPGX_OK;
}

}  /* extern "C" */

/* ---- the host twin of k_jd_sub: jx_jfif_sub.h's routines, lane after lane ------- */
namespace {

/* the last pass's writer with the twin's counters */
template <int GRAY>
struct StatStore : jxs_store_t<GRAY> {
    jpgx_jfif_sub_stats *stats;
    uint32_t sub_end, tile_bytes;
    void unit(uint32_t, uint32_t last)
    {
        if (!stats || last < sub_end) return;
        stats->units_across_sub++;
        if (sub_end == tile_bytes) stats->units_across_tile++;
    }
};

struct Lane {
    jxs_state first, entry, exit;       /* first: the exit of the lane's first decode */
    uint32_t nblk;
};

/* one restart interval, as k_jd_sub's workgroup decodes it; lanes: [T].  GRAY: the one-component frame */
template <int GRAY>
int sub_interval(const uint8_t *file, size_t len, size_t begin, size_t end, const jxd_frame *fr, const jxd_tab *tabs,
                 uint32_t mcu0, uint32_t count, int16_t *coef, uint32_t S, uint32_t T, Lane *lanes,
                 jpgx_jfif_sub_stats *stats)
{
    const int bad = JPGX_EJFIF_SCAN;
    if (begin > end || end > len || mcu0 > fr->nmcu || count > fr->nmcu - mcu0) return bad;
    jxs_tabs t;
    if (GRAY) jxs_tabs_of_gray(fr, tabs, &t);
    else jxs_tabs_of(fr, tabs, &t);
    const uint32_t nblocks = count * t.bpm;
    for (uint32_t o = 0; o < nblocks; o++) {
        const uint32_t blk = jxs_block_of_t<GRAY>(fr, mcu0, nblocks, o);
        if (blk == JXS_INVALID) return bad;
        memset(coef + (size_t)blk * 64, 0, 64 * sizeof(int16_t));
    }
    jxs_state carry = {0u, 0u};
    uint32_t carry_blocks = 0, err = 0, done = 0;
    for (size_t tb = begin; tb < end && !done; tb += (size_t)S * T) {
        const jxs_tile tile = jxs_tile_of(end - tb, S, T);
        const jxs_flat rd = {file + tb};
        const uint32_t nl = (tile.n + S - 1) / S;           /* the lanes that have bytes */
        if (stats) stats->tiles++, stats->subsequences += nl;
        /* bare FFs, guesses and the first decode */
        for (uint32_t i = 0; i < nl; i++) {
            Lane &l = lanes[i];
            const uint32_t sub_end = (i + 1) * S < tile.n ? (i + 1) * S : tile.n;
            err |= jxs_bare_ff(rd, i * S, sub_end, tile.end_rel);
            uint32_t on_stuffing = 0;
            l.entry = i ? jxs_guess(rd, i, S, &on_stuffing) : carry;
            if (stats) stats->starts_on_stuffing += on_stuffing;
            jxs_nowrite nw;
            jxs_decode_sub(rd, tile.lim, sub_end, l.entry, &t, nw, &l.exit, &l.nblk);
            l.first = l.exit;
        }
        /* rounds: a lane takes its neighbour's exit where that is valid and not what it decoded from */
        uint32_t rounds = 0;
        for (; rounds < T; rounds++) {
            uint32_t changed = 0;
            jxs_state prev = lanes[0].exit;                 /* the exits as they were before the round */
            for (uint32_t i = 1; i < nl; i++) {
                Lane &l = lanes[i];
                const jxs_state mine = l.exit;
                if (prev.p != JXS_INVALID && !jxs_same(prev, l.entry)) {
                    const uint32_t sub_end = (i + 1) * S < tile.n ? (i + 1) * S : tile.n;
                    l.entry = prev;
                    jxs_nowrite nw;
                    jxs_decode_sub(rd, tile.lim, sub_end, l.entry, &t, nw, &l.exit, &l.nblk);
                    changed = 1;
                    if (stats) stats->redecodes++;
                }
                prev = mine;
            }
            if (!changed) break;
        }
        if (stats && rounds > stats->rounds_max) stats->rounds_max = rounds;
        /* the first lane whose exit is invalid: it and the lanes before it decoded from true states */
        uint32_t first_bad = T;
        for (uint32_t i = nl; i-- > 0;)
            if (lanes[i].exit.p == JXS_INVALID) first_bad = i;
        /* place and write */
        uint32_t ord = carry_blocks;
        for (uint32_t i = 0; i < nl; i++) {
            Lane &l = lanes[i];
            if (i <= first_bad && l.entry.p != JXS_INVALID && ord < nblocks) {
                if (stats && i && !jxs_same(l.first, l.exit)) stats->wrong_first_guesses++;
                StatStore<GRAY> wr;
                wr.open(fr, coef, mcu0, nblocks, ord);
                wr.stats = stats;
                wr.sub_end = (i + 1) * S < tile.n ? (i + 1) * S : tile.n;
                wr.tile_bytes = S * T;
                jxs_state out;
                uint32_t nb;
                jxs_decode_sub(rd, tile.lim, wr.sub_end, l.entry, &t, wr, &out, &nb);
                if (out.p == JXS_INVALID) err = 1;
                else if (wr.ord == nblocks) {
                    done = 1;
                    if (!jxs_tail_ok(rd, tile.lim, tile.end_rel, out.p)) err = 1;
                }
            }
            ord += l.nblk;
        }
        if (first_bad < T) break;                           /* nothing behind an invalid state is true */
        carry = lanes[nl - 1].exit;
        carry.p -= S * T * 8u;                              /* seen from the next tile (if there is one) */
        carry_blocks = ord;
    }
    if (err || !done) return bad;
    /* the DC predictors: per component a running sum over the interval's blocks in decode order,
     * 256 at a time, each chunk's sums checked against int16 before the carry moves on */
    for (uint32_t comp = 0; comp < (GRAY ? 1u : 3u); comp++) {
        const uint32_t per = comp ? 1u : t.lum, nbk = count * per;
        int32_t pred = 0;
        for (uint32_t i0 = 0; i0 < nbk; i0 += 256) {
            for (uint32_t i = i0; i < nbk && i < i0 + 256; i++) {
                const uint32_t m = i / per, j = comp ? t.lum + comp - 1u : i - m * per;
                const uint32_t blk = jxs_block_of_t<GRAY>(fr, mcu0, nblocks, m * t.bpm + j);
                if (blk == JXS_INVALID) return bad;
                pred += coef[(size_t)blk * 64];
                if (pred < -32768 || pred > 32767) err = 1;
                coef[(size_t)blk * 64] = (int16_t)pred;
            }
            if (err) return bad;
        }
    }
    return 0;
}

int read_sub(int mode, const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs, int16_t *coef,
             size_t coef_cap, uint16_t *qt, jpgx_jfif_info *info, jpgx_jfif_sub_stats *stats)
{
    if (!file || !coef) return JPGX_EARG;
    if (!sub_bytes && !tile_subs) sub_bytes = JXS_SUB, tile_subs = JXS_TILE;
    if (sub_bytes < 16 || tile_subs < 2 || (uint64_t)sub_bytes * tile_subs > (1u << 24)) return JPGX_EARG;
    if (stats) memset(stats, 0, sizeof *stats);
    jxd_frame fr;
    memset(&fr, 0, sizeof fr);
    jxd_tab *tabs = (jxd_tab *)malloc(4 * sizeof(jxd_tab));
    if (!tabs) return JPGX_ENOMEM;
    int rc = parse(mode, file, len, &fr, tabs);
    if (rc) {
        free(tabs);
        return rc;
    }
    if (info) fill_info(fr, info);
    copy_qt(mode, fr, qt);
    if (coef_cap < (size_t)fr.nblk * 64) {
        free(tabs);
        return JPGX_EARG;
    }
    size_t *marks = (size_t *)malloc((fr.ni > 1 ? fr.ni - 1 : 1) * sizeof(size_t));
    Lane *lanes = (Lane *)malloc(tile_subs * sizeof(Lane));
    if (!marks || !lanes) {
        free(lanes);
        free(marks);
        free(tabs);
        return JPGX_ENOMEM;
    }
    rc = find_marks(file, len, &fr, marks);
    for (uint32_t iv = 0; !rc && iv < fr.ni; iv++) {
        const size_t begin = iv ? marks[iv - 1] + 2 : (size_t)fr.scan_off;
        const size_t end = iv + 1 < fr.ni ? marks[iv] : len - 2;
        const uint32_t mcu0 = iv * fr.mpi;
        const uint32_t count = fr.nmcu - mcu0 < fr.mpi ? fr.nmcu - mcu0 : fr.mpi;
        rc = mode == kGray
                 ? sub_interval<1>(file, len, begin, end, &fr, tabs, mcu0, count, coef, sub_bytes, tile_subs, lanes, stats)
                 : sub_interval<0>(file, len, begin, end, &fr, tabs, mcu0, count, coef, sub_bytes, tile_subs, lanes, stats);
    }
    free(lanes);
    free(marks);
    free(tabs);
    return rc;
}

}  // namespace

extern "C" {

void jpgx_jfif_decode_sub_shape(uint32_t *sub_bytes, uint32_t *tile_subs)
{
    if (sub_bytes) *sub_bytes = JXS_SUB;
    if (tile_subs) *tile_subs = JXS_TILE;
}

int jpgx_read_jfif_sub(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs, int16_t *coef,
                       size_t coef_cap, uint16_t qt[2][64], jpgx_jfif_info *info, jpgx_jfif_sub_stats *stats)
{
    return read_sub(kPlain, file, len, sub_bytes, tile_subs, coef, coef_cap, (uint16_t *)qt, info, stats);
}

int jpgx_read_jfif_sub_any(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs, int16_t *coef,
                           size_t coef_cap, uint16_t qt[2][64], jpgx_jfif_info *info, jpgx_jfif_sub_stats *stats)
{
    return read_sub(kAny, file, len, sub_bytes, tile_subs, coef, coef_cap, (uint16_t *)qt, info, stats);
}

int jpgx_read_jfif_sub_gray(const uint8_t *file, size_t len, uint32_t sub_bytes, uint32_t tile_subs, int16_t *coef,
                            size_t coef_cap, uint16_t qt[64], jpgx_jfif_info *info, jpgx_jfif_sub_stats *stats)
{
    return read_sub(kGray, file, len, sub_bytes, tile_subs, coef, coef_cap, qt, info, stats);
}

}  /* extern "C" */
