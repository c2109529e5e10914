/*
 * jpgx_gray_host.cpp -- TEST-ONLY: k_gray (csrc/jpgx_gray.hip) restated on the host from the text it shares
 * with the kernel, csrc/jx_gray.h: the load rule with every load checked against a buffer
 * (jx_gray_load_trace), the fp32 sequence and band against the exact coefficient (jx_selftest_gray,
 * jx_selftest_gray_blocks; the bench tool reads the flagged share from the latter) and the whole transform
 * of an image (jx_gray_host_blocks).  The tables are the host plan's (jx_plan_tables_gray,
 * csrc/jpgx_plan.cpp).  No HIP: built with g++, as jpgx_plan.cpp.
 */
#include <math.h>
#include <string.h>

#include "jpgx_internal.h"
#include "jx_consts.h"
#include "jx_gray.h"

namespace {

inline uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

uint64_t sm64(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

const double kGrayCos[8][8] = JX_COS_INIT;
const int kGrayScan[8][8] = JX_SCAN_ORDER_INIT;

/* the host's loads, as they are */
struct GrayHostMem {
    uint64_t u64(const uint8_t *p) const
    {
        uint64_t v;
        memcpy(&v, p, 8);
        return v;
    }
    uint32_t u32(const uint8_t *p) const
    {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    uint8_t u8(const uint8_t *p) const { return *p; }
};

/* loads that are checked against a buffer and recorded instead of trusted: touched[i] |= 1 (byte load),
 * 2 (4-byte), 4 (8-byte) for every byte read; a load outside the buffer, or an aligned load that is not
 * aligned, is counted in bad and returns zeros */
struct GrayTraceMem {
    const uint8_t *buf;
    size_t len;
    uint8_t *touched;
    long long *bad;
    uint64_t get(const uint8_t *p, size_t n, uint8_t mark) const
    {
        const size_t off = (size_t)(p - buf);
        if (p < buf || off > len || n > len - off || ((uintptr_t)p & (n - 1))) {
            ++*bad;
            return 0;
        }
        uint64_t v = 0;
        memcpy(&v, p, n);
        for (size_t i = 0; i < n; i++) touched[off + i] |= mark;
        return v;
    }
    uint64_t u64(const uint8_t *p) const { return get(p, 8, 4); }
    uint32_t u32(const uint8_t *p) const { return (uint32_t)get(p, 4, 2); }
    uint8_t u8(const uint8_t *p) const { return (uint8_t)get(p, 1, 1); }
};

struct GrayTabs {
    float w[64], lim[64];          /* [v * 8 + u] */
    int16_t q[64];                 /* [u * 8 + v] */
};

/* one block as k_gray computes it: the fp32 path, the band test, the exact value for flagged
 * coefficients.  out (may be NULL): zig-zag int16.  Returns the mask of flagged coefficients, bit
 * v * 8 + u; *bad += unflagged coefficients whose fp32 result is not the exact value. */
uint64_t gray_block(const uint32_t (&raw)[8][2], const GrayTabs &t, bool force, int16_t *out, long long *bad)
{
    float T[8][8];
    jx_gray_rows(raw, T);
    const auto px = [&](int x, int y) { return jx_gray_byte(raw, x, y); };
    uint64_t flags = 0;
    for (int u = 0; u < 8; u++) {
        float wu[8], tm[8], d[8];
        for (int v = 0; v < 8; v++) wu[v] = t.w[v * 8 + u];
        jx_gray_col(T, u, wu, tm, d);
        for (int v = 0; v < 8; v++) {
            const bool flag = fabsf(d[v]) >= (force ? -1.0f : t.lim[v * 8 + u]);
            const int16_t fast = (int16_t)(uint16_t)bits(tm[v]);
            const int16_t exact = jx_gray_exact(px, u, v, t.q[u * 8 + v], kGrayCos);
            if (flag) flags |= 1ull << (v * 8 + u);
            else if (fast != exact && bad) ++*bad;
            if (out) out[kGrayScan[v][u]] = flag ? exact : fast;
        }
    }
    return flags;
}

}  // namespace

/* k_gray's arithmetic on the host over given blocks px [nblocks][64] (row-major samples): returns the
 * number of unflagged coefficients whose fp32 result differs from the exact value (must be 0), -1 for a
 * bad quality; *flagged: the flagged coefficients; flagmask (may be NULL) [nblocks]: bit v * 8 + u */
extern "C" long long jx_selftest_gray_blocks(const uint8_t *px, long long nblocks, int quality, long long *flagged,
                                             uint64_t *flagmask)
{
    GrayTabs t;
    if (!px || jx_plan_tables_gray(quality, t.w, t.lim, t.q)) return -1;
    long long bad = 0, nfl = 0;
    for (long long n = 0; n < nblocks; n++) {
        uint32_t raw[8][2];
        jx_gray_load_block(GrayHostMem{}, px + 64 * n, 8, 8, 8, 0, 0, raw);
        const uint64_t m = gray_block(raw, t, false, NULL, &bad);
        nfl += __builtin_popcountll(m);
        if (flagmask) flagmask[n] = m;
    }
    if (flagged) *flagged = nfl;
    return bad;
}

/* the same over generated blocks: noise, flat, two-level and ramp blocks in turn (jx_selftest_pk's) */
extern "C" long long jx_selftest_gray(long long nblocks, unsigned long long seed, int quality, long long *flagged)
{
    uint64_t s = seed;
    long long bad = 0, nfl = 0;
    for (long long n = 0; n < nblocks; n++) {
        uint8_t px[64];
        const int kind = (int)(n % 4);
        const uint64_t r0 = sm64(s);
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) {
                uint8_t v;
                if (kind == 0) v = (uint8_t)(sm64(s) >> 56);
                else if (kind == 1) v = (uint8_t)r0;
                else if (kind == 2) v = ((r0 >> (x + 8 * y)) & 1) ? 255 : (uint8_t)(r0 >> 40);
                else v = (uint8_t)((x * (int)(r0 & 31) + y * (int)((r0 >> 5) & 31)) & 255);
                px[y * 8 + x] = v;
            }
        long long f = 0;
        const long long b = jx_selftest_gray_blocks(px, 1, quality, &f, NULL);
        if (b < 0) return -1;
        bad += b;
        nfl += f;
    }
    if (flagged) *flagged = nfl;
    return bad;
}

/* k_gray on the host, lane by lane: the coefficients of a width x height image (rows pitch bytes apart)
 * into out [nb][64].  For the tests: the kernel's load rule, arithmetic and exact pass without a device. */
extern "C" int jx_gray_host_blocks(const uint8_t *img, int width, int height, size_t pitch, int quality, int force,
                                   int16_t *out)
{
    GrayTabs t;
    if (!img || !out || width < 1 || height < 1 || width > 65535 || height > 65535 || pitch < (size_t)width)
        return JPGX_EARG;
    if (jx_plan_tables_gray(quality, t.w, t.lim, t.q)) return JPGX_EQUALITY;
    const uint32_t bw = ((uint32_t)width + 7u) / 8u, bh = ((uint32_t)height + 7u) / 8u;
    for (uint32_t by = 0; by < bh; by++)
        for (uint32_t bx = 0; bx < bw; bx++) {
            uint32_t raw[8][2];
            jx_gray_load_block(GrayHostMem{}, img, (long long)pitch, (uint32_t)width, (uint32_t)height, bx, by, raw);
            gray_block(raw, t, force != 0, out + ((size_t)by * bw + bx) * 64, NULL);
        }
    return JPGX_OK;
}

/* jx_gray_load_block for every block of a width x height frame that begins at buf + base_off, with every
 * load checked against [buf, buf + buflen) and recorded in touched [buflen] (GrayTraceMem); blocks
 * [nb][64]: the samples it assembled.  Returns the number of refused loads (must be 0). */
extern "C" long long jx_gray_load_trace(const uint8_t *buf, size_t buflen, size_t base_off, int width, int height,
                                        size_t pitch, uint8_t *touched, uint8_t *blocks)
{
    long long bad = 0;
    const GrayTraceMem mem{buf, buflen, touched, &bad};
    const uint32_t bw = ((uint32_t)width + 7u) / 8u, bh = ((uint32_t)height + 7u) / 8u;
    for (uint32_t by = 0; by < bh; by++)
        for (uint32_t bx = 0; bx < bw; bx++) {
            uint32_t raw[8][2];
            jx_gray_load_block(mem, buf + base_off, (long long)pitch, (uint32_t)width, (uint32_t)height, bx, by, raw);
            uint8_t *b = blocks + ((size_t)by * bw + bx) * 64;
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) b[y * 8 + x] = (uint8_t)jx_gray_byte(raw, x, y);
        }
    return bad;
}
