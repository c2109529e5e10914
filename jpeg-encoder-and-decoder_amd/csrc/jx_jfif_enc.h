/*
 * jx_jfif_enc.h -- the baseline JFIF entropy coder's routines, one source for the
 * host writer (csrc/jpgx_jfif_write.cpp, g++) and the device coder (csrc/jpgx_jfif.hip): the
 * magnitude categories of T.81 F.1.2.1, the clamps, one block's walk (DC symbol, run/size symbols,
 * ZRL, EOB).  The scan's geometry and the place of an MCU's blocks in the coefficient array are
 * jx_frame.h's.  Plain functions and templates, no allocation, no I/O, no global state.
 *
 * Not here, because the two sides differ by nature: the bit writers (a growable buffer with
 * stuffing on the host; bit offsets, LDS slots and a later stuffing pass on the device), the table
 * builder of Annex K.2 (jx_jfif_optimal, restated in parallel by k_jf_tables) and what
 * restart_rows 0 and -1 mean.
 */
#ifndef JX_JFIF_ENC_H
#define JX_JFIF_ENC_H

#include <stddef.h>
#include <stdint.h>

#include "jx_frame.h"

#if defined(__HIPCC__)
#define JXE_FN __host__ __device__ static inline
#else
#define JXE_FN static inline
#endif

/* the largest DC difference and AC magnitude baseline Huffman coding has a category for; the
 * reference's coefficients pass them only for chroma at q >= 93 (its Cb sign error) */
#define JXE_DC_MAX 2047
#define JXE_AC_MAX 1023

/* magnitude category and the value's additional bits (T.81 F.1.2.1) */
JXE_FN uint32_t jxe_category(int v, uint32_t *extra)
{
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    const uint32_t s = a ? 32u - (uint32_t)__builtin_clz(a) : 0u;
    *extra = (uint32_t)(v < 0 ? v + (1 << s) - 1 : v) & ((1u << s) - 1u);
    return s;
}

/* the DC difference against the component's previous block (true DC prediction), clamped */
JXE_FN int jxe_dc_diff(int dc, int pred)
{
    int d = dc - pred;
    d = d > JXE_DC_MAX ? JXE_DC_MAX : d;
    d = d < -JXE_DC_MAX ? -JXE_DC_MAX : d;
    return d;
}

/* One block's symbols (T.81 F.1.2) into a sink: the DC symbol of `diff` (jxe_dc_diff), then one
 * symbol per turn over nz, the mask of the nonzero AC coefficients (bit k: coefficient k; bit 0
 * clear) -- a ZRL while the run of zeros exceeds 15, else run << 4 | category of the clamped
 * coefficient -- then EOB unless coefficient 63 is nonzero.
 *   coef.fetch(k)         reads coefficient k (zig-zag order) in whatever form memory holds it;
 *                         asked only for set bits of nz (and for k = 0 when there is none left)
 *   coef.value(raw, k)    what fetch(k) returned, as an int
 *   sink.dc(s, extra)     the DC symbol: category s and its s additional bits
 *   sink.ac(sym, s, extra)   an AC symbol (ZRL 0xf0 and EOB 0x00 with s = 0)
 * The sink looks the symbol's code up, if it needs one.  The next turn's coefficient is fetched
 * before this turn's symbol goes to the sink and unpacked only in its own turn, so that on the
 * device the read is in flight under the sink's table lookup and nothing waits for it before that
 * (the time of k_jf_len and k_jf_pack depends on it: the device's fetch is an LDS read of a packed
 * pair, its value() the shift; on the host both are z[k]). */
template <class Sink, class Coef>
JXE_FN void jxe_walk(Sink &sink, Coef coef, uint64_t nz, int diff)
{
    uint32_t extra;
    uint32_t s = jxe_category(diff, &extra);
    sink.dc(s, extra);
    uint32_t prev = 0;
    uint32_t k = nz ? (uint32_t)__builtin_ctzll(nz) : 0u;
    auto raw = coef.fetch(k);
    while (nz) {
        const uint32_t run = k - prev - 1u;
        const bool zrl = run > 15u;
        const uint64_t nzn = zrl ? nz : nz & (nz - 1);
        const uint32_t kn = nzn ? (uint32_t)__builtin_ctzll(nzn) : 0u;
        const auto rawn = coef.fetch(kn);
        int v = coef.value(raw, k);
        v = v > JXE_AC_MAX ? JXE_AC_MAX : v;
        v = v < -JXE_AC_MAX ? -JXE_AC_MAX : v;
        s = jxe_category(v, &extra);
        const uint32_t sym = zrl ? 0xf0u : (run << 4 | s);
        s = zrl ? 0u : s;
        extra = zrl ? 0u : extra;
        prev = zrl ? prev + 16u : k;
        nz = nzn;
        k = kn;
        raw = rawn;
        sink.ac(sym, s, extra);
    }
    if (prev < 63u) sink.ac(0x00u, 0u, 0u);
}

#endif
