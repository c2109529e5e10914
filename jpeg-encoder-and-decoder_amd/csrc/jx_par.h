/*
 * jx_par.h -- the host twins' thread fan-out: how many threads a call takes and a runner that splits
 * n items among them.  Header-only and host-only: jpgx_jfif_read.cpp, jpgx_jfif_write.cpp and
 * jpgx_pixels_host.cpp include it, no kernel source does.
 */
#ifndef JX_PAR_H
#define JX_PAR_H

#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <unistd.h>

#define JX_PAR_MAX 64

/* the threads of a call that asks for `nthreads`: 0 is one per online CPU; 1 .. JX_PAR_MAX */
static inline uint32_t jx_thread_count(int nthreads)
{
    long n = nthreads ? nthreads : sysconf(_SC_NPROCESSORS_ONLN);
    if (n < 1) n = 1;
    if (n > JX_PAR_MAX) n = JX_PAR_MAX;
    return (uint32_t)n;
}

/* range t of the nt that n items are split into is [i0, i1) */
typedef void (*jx_par_fn)(void *ctx, uint32_t t, uint64_t i0, uint64_t i1);

struct jx_par_task {
    jx_par_fn fn;
    void *ctx;
    uint32_t t;
    uint64_t i0, i1;
    pthread_t th;
    int started;
};

static inline void *jx_par_main(void *arg)
{
    const jx_par_task *k = (const jx_par_task *)arg;
    k->fn(k->ctx, k->t, k->i0, k->i1);
    return NULL;
}

/* fn(ctx, t, n t / nt, n (t + 1) / nt) for t = 0 .. nt - 1, with nt no more than n and any count
 * otherwise; every range on a thread of its own except the last, which runs on the caller's, as does
 * a range whose thread does not start.  All of them have returned when this returns. */
static inline void jx_par_run(uint64_t n, uint64_t nt, jx_par_fn fn, void *ctx)
{
    jx_par_task few[JX_PAR_MAX], *tasks = few;
    if (nt > n) nt = n;
    if (nt > JX_PAR_MAX) tasks = (jx_par_task *)malloc((size_t)nt * sizeof *tasks);
    for (uint64_t t = 0; t < nt; t++) {
        jx_par_task one = {fn, ctx, (uint32_t)t, n * t / nt, n * (t + 1) / nt, pthread_t(), 0};
        jx_par_task *k = tasks ? &tasks[t] : &one;          /* no memory for the tasks: one by one, here */
        *k = one;
        k->started = tasks && t + 1 < nt && pthread_create(&k->th, NULL, jx_par_main, k) == 0;
        if (!k->started) jx_par_main(k);
    }
    for (uint64_t t = 0; tasks && t < nt; t++)
        if (tasks[t].started) pthread_join(tasks[t].th, NULL);
    if (tasks != few) free(tasks);
}

#endif
