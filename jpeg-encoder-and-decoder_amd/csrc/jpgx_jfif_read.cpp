/*
 * jpgx_jfif_read.cpp -- the host decoder of baseline JFIF files back to the coefficient layout
 * (DESIGN.md 4.8): jpgx_jfif_info_of, jpgx_read_jfif (include/jpgx_compat.h).  The routines are
 * those of jx_jfif_dec.h, the ones the device decoder (jpgx_jfif_dec.hip) runs; this file adds the
 * search for the restart markers and the threads.  No HIP: built with g++, as jpgx_plan.cpp.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/jpgx_compat.h"
#include "jx_jfif_dec.h"

namespace {

struct Job {
    const uint8_t *file;
    size_t len;
    const jxd_frame *fr;
    const jxd_tab *tabs;
    const size_t *marks;                /* [ni - 1] the restart markers' places */
    int16_t *coef;
    uint32_t iv0, iv1;                  /* this thread's intervals */
    int rc;
};

void *run(void *arg)
{
    Job *j = (Job *)arg;
    const jxd_frame *fr = j->fr;
    j->rc = 0;
    for (uint32_t iv = j->iv0; iv < j->iv1; iv++) {
        const size_t begin = iv ? j->marks[iv - 1] + 2 : (size_t)fr->scan_off;
        const size_t end = iv + 1 < fr->ni ? j->marks[iv] : j->len - 2;
        const uint32_t mcu0 = iv * fr->mpi;
        const uint32_t count = fr->nmcu - mcu0 < fr->mpi ? fr->nmcu - mcu0 : fr->mpi;
        if (jxd_decode_interval(j->file, j->len, begin, end, fr, j->tabs, mcu0, count, j->coef)) j->rc = JPGX_EJFIF_SCAN;
    }
    return NULL;
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

}  // namespace

extern "C" {

int jpgx_jfif_info_of(const uint8_t *file, size_t len, jpgx_jfif_info *info)
{
    if (!file || !info) return JPGX_EARG;
    jxd_frame fr;
    jxd_tab *tabs = (jxd_tab *)malloc(4 * sizeof(jxd_tab));
    if (!tabs) return JPGX_ENOMEM;
    memset(&fr, 0, sizeof fr);
    const int rc = jxd_parse_header(file, len, &fr, tabs);
    free(tabs);
    if (rc) return rc;
    fill_info(fr, info);
    return JPGX_OK;
}

int jpgx_read_jfif(const uint8_t *file, size_t len, int nthreads, int16_t *coef, size_t coef_cap, uint16_t qt[2][64],
                   jpgx_jfif_info *info)
{
    if (!file || !coef || nthreads < 0) return JPGX_EARG;
    jxd_frame fr;
    memset(&fr, 0, sizeof fr);
    jxd_tab *tabs = (jxd_tab *)malloc(4 * sizeof(jxd_tab));
    if (!tabs) return JPGX_ENOMEM;
    int rc = jxd_parse_header(file, len, &fr, tabs);
    if (rc) {
        free(tabs);
        return rc;
    }
    if (info) fill_info(fr, info);
    if (qt) memcpy(qt, fr.qt, sizeof fr.qt);
    if (coef_cap < (size_t)fr.nblk * 64) {
        free(tabs);
        return JPGX_EARG;
    }
    /* the restart markers: FF D0 .. D7 cannot occur inside entropy-coded data.  Their count must be
     * the intervals' less one, their numbers run k mod 8, and EOI ends the file */
    const size_t scan = (size_t)fr.scan_off;
    size_t *marks = (size_t *)malloc((fr.ni > 1 ? fr.ni - 1 : 1) * sizeof(size_t));
    if (!marks) {
        free(tabs);
        return JPGX_ENOMEM;
    }
    size_t found = 0;
    rc = jxd_has_eoi(file, len, scan) ? 0 : JPGX_EJFIF_SCAN;
    for (size_t p = scan; !rc && p + 1 < len; p++) {
        if (!jxd_is_rst(file, len, scan, p)) continue;
        if (found >= fr.ni - 1 || (file[p + 1] & 7u) != (found & 7u)) rc = JPGX_EJFIF_SCAN;
        else marks[found++] = p;
    }
    if (!rc && found != fr.ni - 1) rc = JPGX_EJFIF_SCAN;
    if (!rc) {
        long ncpu = nthreads ? nthreads : sysconf(_SC_NPROCESSORS_ONLN);
        if (ncpu < 1) ncpu = 1;
        if (ncpu > 64) ncpu = 64;
        uint32_t nt = (uint32_t)ncpu < fr.ni ? (uint32_t)ncpu : fr.ni;
        Job jobs[64];
        pthread_t th[64];
        bool started[64];
        for (uint32_t t = 0; t < nt; t++) {
            Job &j = jobs[t];
            j.file = file;
            j.len = len;
            j.fr = &fr;
            j.tabs = tabs;
            j.marks = marks;
            j.coef = coef;
            j.iv0 = (uint32_t)((uint64_t)fr.ni * t / nt);
            j.iv1 = (uint32_t)((uint64_t)fr.ni * (t + 1) / nt);
            j.rc = 0;
            /* the last run on this thread; a thread that does not start is run here as well */
            started[t] = t + 1 < nt && pthread_create(&th[t], NULL, run, &j) == 0;
            if (!started[t]) run(&j);
        }
        for (uint32_t t = 0; t < nt; t++) {
            if (started[t]) pthread_join(th[t], NULL);
            if (jobs[t].rc) rc = jobs[t].rc;
        }
    }
    free(marks);
    free(tabs);
    return rc;
}

}  /* extern "C" */
