/*
 * jpgx_plan.cpp -- host side of the C-ABI shim: argument validation, quantisation tables,
 * the underflow bytes, and the rigorous fp32 guard band.  No device code here.
 *
 * Guard band.  The kernel computes each quotient t = F(u,v)/Q[u][v] in fp32 (xform_math.h,
 * FOps).  BoundOps below pushes an interval [lo,hi] of the exact value and a bound E on the
 * fp32 error through the very same template code, starting from pixel bytes in [0,255]:
 *     add/sub:  E = Ea + Eb + 2^-24 (|c| + Ea + Eb)
 *     a*k:      E = Ea|k_f| + |a| |k_f - k| + 2^-24 (...)
 *     fma:      E = Ea|k_f| + |a| |k_f - k| + Eb + 2^-24 (...)
 * and adds the error of the fp32 scale.  If the fp32 quotient sits farther than E_t from a
 * half-integer, the reference's double quotient rounds (src/quantise.c:58, C round()) to the
 * same integer; otherwise the kernel flags the coefficient for the exact-order fp64 path.
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "jpgx_internal.h"
#include "jx_consts.h"
#include "jx_gray.h"
#include "xform_math.h"

/* pristine base tables, src/quantise.c:8-25 (row index = first subscript) */
static const int kLum[8][8] = JX_Q_LUM_INIT;
static const int kChr[8][8] = JX_Q_CHR_INIT;

namespace {

struct Bnd {
    double lo, hi, E;
};

struct BoundOps {
    typedef Bnd T;
    static double mag(const Bnd &a) { return std::max(fabs(a.lo), fabs(a.hi)); }
    static Bnd round_(double lo, double hi, double err)
    {
        const double u = 0x1p-24;
        Bnd c{lo, hi, 0};
        c.E = err + u * (mag(c) + err);
        return c;
    }
    static void span(double a, double b, double &lo, double &hi)
    {
        lo = std::min(a, b);
        hi = std::max(a, b);
    }
    static Bnd add(Bnd a, Bnd b) { return round_(a.lo + b.lo, a.hi + b.hi, a.E + b.E); }
    static Bnd sub(Bnd a, Bnd b) { return round_(a.lo - b.hi, a.hi - b.lo, a.E + b.E); }
    static Bnd mulc(Bnd a, jx_const k)
    {
        double lo, hi;
        span(a.lo * k.x, a.hi * k.x, lo, hi);
        return round_(lo, hi, a.E * fabs((double)k.f) + mag(a) * fabs((double)k.f - k.x));
    }
    static Bnd fmac(Bnd a, jx_const k, Bnd b)
    {
        double lo, hi;
        span(a.lo * k.x, a.hi * k.x, lo, hi);
        return round_(lo + b.lo, hi + b.hi,
                      a.E * fabs((double)k.f) + mag(a) * fabs((double)k.f - k.x) + b.E);
    }
    static Bnd lit(jx_const k) { return Bnd{k.x, k.x, fabs((double)k.f - k.x)}; }
};

/* sub: 0 = one pixel per sample (4:4:4 and the reference's parity modes); 1 = true 4:2:2,
 * 2 = true 4:2:0, in the kernels' (k_chroma, k_sub422) operation order: the colour transform
 * of the pair's / quad's byte sums (exact integers <= 510 / 1020 in fp32), times 0.5 / 0.25.
 * The exact value is the average of the pixels' samples (the oracle's definition); the colour
 * transform being linear, it equals the transform of the sums scaled, in real arithmetic. */
template <int CH>
void coef_bounds(Bnd F[8][8], int sub = 0)
{
    const Bnd byte{0.0, sub == 1 ? 510.0 : (sub == 2 ? 1020.0 : 255.0), 0.0};
    Bnd px[8], row[8];
    Bnd p = jx_pixel<BoundOps, CH>(byte, byte, byte);
    if (sub == 1) p = BoundOps::mulc(p, JX_K(0.5));
    if (sub == 2) p = BoundOps::mulc(p, JX_K(0.25));
    for (int x = 0; x < 8; x++) px[x] = p;
    jx_fdct8<BoundOps>(px, row);   /* every pixel row has the same bound */
    for (int u = 0; u < 8; u++) {
        Bnd col[8], out[8];
        for (int y = 0; y < 8; y++) col[y] = row[u];
        jx_fdct8<BoundOps>(col, out);
        for (int v = 0; v < 8; v++) F[v][u] = out[v];
    }
}

}  // namespace

extern "C" {

int jpgx_validate(int width, int height, const jpgx_params *p)
{
    if (!p) return JPGX_EARG;
    if (p->sample_ratio < 0 || p->sample_ratio > 2) return JPGX_ESAMPLE;
    if (p->quality < 1 || p->quality > 97) return JPGX_EQUALITY;
    /* src/preprocess.c:82-98 pads by w%8 / w%16 / h%16 (not up to a multiple), after which
     * its copy loop is wrong: only exact multiples have defined reference behaviour. */
    const int wm = p->sample_ratio == 0 ? 8 : 16, hm = p->sample_ratio == 2 ? 16 : 8;
    if (width <= 0 || height <= 0 || width % wm || height % hm) return JPGX_EGEOMETRY;
    return JPGX_OK;
}

static unsigned long long req2size(unsigned long long n)
{
    unsigned long long s = (n + 8 + 15) & ~15ULL;
    return s < 32 ? 32 : s;
}

void jpgx_glibc_underflow(long long n_pixels, long long bmp_file_size, uint8_t out[8])
{
    /* glibc malloc (64-bit): the chunk-size word sits 8 bytes before the user pointer.
     * r_new is an sbrk chunk (size | PREV_INUSE) unless it is at or above the mmap
     * threshold (size rounded to pages | IS_MMAPPED).  The threshold starts at 128 KiB and
     * rises to the size of the mmapped file buffer freed at src/bitmap.c:151 when that
     * chunk is at most 32 MiB (DEFAULT_MMAP_THRESHOLD_MAX). */
    const unsigned long long page = 4096, thr0 = 128 * 1024, thr_max = 32ULL << 20;
    unsigned long long thr = thr0;
    const unsigned long long fchunk = req2size((unsigned long long)bmp_file_size);
    if (fchunk >= thr0) {
        const unsigned long long mm = (fchunk + 8 + page - 1) & ~(page - 1);
        if (mm > thr && mm <= thr_max) thr = mm;
    }
    const unsigned long long nb = req2size((unsigned long long)n_pixels);
    const unsigned long long size =
        nb >= thr ? (((nb + 8 + page - 1) & ~(page - 1)) | 2ULL) : (nb | 1ULL);
    for (int k = 0; k < 8; k++) out[k] = (uint8_t)(size >> (8 * k));
}

void jpgx_default_params(jpgx_params *p, int width, int height, int quality, int sample_ratio)
{
    memset(p, 0, sizeof *p);
    p->quality = quality;
    p->sample_ratio = sample_ratio;
    const long long n = (long long)width * height;
    jpgx_glibc_underflow(n, 54 + 3 * n, p->underflow[0]);
    memcpy(p->underflow[1], p->underflow[0], 8);
    memcpy(p->underflow[2], p->underflow[0], 8);
}

int jpgx_scale_table(int which, int quality, int out[8][8])
{
    if (quality < 1 || quality > 97) return JPGX_EQUALITY;
    const int(*base)[8] = which == 0 ? kLum : kChr;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;  /* quantise.c:81 */
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) out[i][j] = (s * base[i][j] + 50) / 100;  /* :82 */
    return JPGX_OK;
}

void jx_under_dwords(const uint8_t under[3][8], uint32_t out[6])
{
    /* the missing pixel row, interleaved like the input: pixel x = (r_x, g_x, b_x) */
    uint8_t row[24];
    for (int x = 0; x < 8; x++)
        for (int k = 0; k < 3; k++) row[3 * x + k] = under[k][x];
    memcpy(out, row, sizeof row);
}

/* long-double evaluation of the same 1-D transform code (near-exact constants) */
struct LDOps {
    typedef long double T;
    static T add(T a, T b) { return a + b; }
    static T sub(T a, T b) { return a - b; }
    static T mulc(T a, jx_const k) { return a * (long double)k.x; }
    static T fmac(T a, jx_const k, T b) { return a * (long double)k.x + b; }
    static T lit(jx_const k) { return (long double)k.x; }
};

/* Factor that turns output k of jx_fdct8 into sum_x in[x] cos((2x+1)k pi/16): evaluated on
 * in[x] = cos((2x+1)k pi/16) (where that sum is 8 for k = 0, else 4). */
static long double dct_kfactor(int k)
{
    const long double pi = 3.141592653589793238462643383279502884L;
    long double in[8], out[8];
    for (int x = 0; x < 8; x++) in[x] = cosl((2 * x + 1) * k * pi / 16);
    jx_fdct8<LDOps>(in, out);
    return (k == 0 ? 8.0L : 4.0L) / out[k];
}

/* this quality's scaled divisors: qs[t][u][v], and q[t][u * 8 + v] as the kernels take them */
static int plan_divisors(int quality, int qs[2][8][8], int16_t q[2][64])
{
    const int rc = jpgx_scale_table(0, quality, qs[0]);
    if (rc) return rc;
    jpgx_scale_table(1, quality, qs[1]);
    for (int t = 0; t < 2; t++)
        for (int u = 0; u < 8; u++)
            for (int v = 0; v < 8; v++) q[t][u * 8 + v] = (int16_t)qs[t][u][v];
    return JPGX_OK;
}

/* a coefficient's fp32 scale and band limit from its exact scale ws and the bound b of its fp32
 * value: the error of t_fp vs the reference's real-arithmetic quotient, plus the final fma
 * rounding of d (< 2^-25), plus slack for the reference's own double rounding (< 1e-10) and for
 * this bound's own double arithmetic */
static void plan_band(long double ws, const Bnd &b, float *w, float *lim)
{
    const float wf = (float)ws;
    const double mF = BoundOps::mag(b) + b.E;
    double et = b.E * fabs((double)wf) + mF * (double)fabsl((long double)wf - ws) + 0x1p-25;
    et = et * 1.01 + 1e-7;
    *w = wf;
    *lim = (float)(0.5 - et);
}

int jx_plan_tables_mode(int quality, int sub, float w[3][64], float lim[3][64], int16_t q[2][64])
{
    int qs[2][8][8];
    const int rc = plan_divisors(quality, qs, q);
    if (rc) return rc;

    Bnd F[3][8][8];
    coef_bounds<0>(F[0]);                  /* luma is never averaged */
    coef_bounds<1>(F[1], sub);
    coef_bounds<2>(F[2], sub);
    const long double a0 = 1.0L / sqrtl(2.0L);
    for (int ch = 0; ch < 3; ch++) {
        const int t = ch == 0 ? 0 : 1;
        for (int v = 0; v < 8; v++)
            for (int u = 0; u < 8; u++) {
                /* exact scale: 1/4 a(u) a(v) k(u) k(v) / Q[u][v] (dct.c:54, quantise.c:58) */
                const long double au = u == 0 ? a0 : 1.0L, av = v == 0 ? a0 : 1.0L;
                const long double ku = dct_kfactor(u), kv = dct_kfactor(v);
                const long double ws = 0.25L * au * av * ku * kv / (long double)qs[t][u][v];
                plan_band(ws, F[ch][v][u], &w[ch][v * 8 + u], &lim[ch][v * 8 + u]);
            }
    }
    return JPGX_OK;
}

int jx_plan_tables(int quality, float w[3][64], float lim[3][64], int16_t q[2][64])
{
    return jx_plan_tables_mode(quality, 0, w, lim, q);
}

int jpgx_guard_band(int quality, float scale[3][64], float lim[3][64])
{
    int16_t q[2][64];
    return jx_plan_tables(quality, scale, lim, q);
}

void jpgx_stripe(int block_rows, int nshards, int k, int *row_begin, int *row_end)
{
    /* contiguous, sizes differ by at most one block row: the first block_rows % n get +1 */
    const int base = block_rows / nshards, extra = block_rows % nshards;
    *row_begin = k * base + std::min(k, extra);
    *row_end = *row_begin + base + (k < extra ? 1 : 0);
}

const char *jpgx_version(void) { return "jpgx 0.1 (gfx950)"; }

size_t jpgx_chroma_blocks(int width, int row_begin, int row_end, int sample_ratio, unsigned flags)
{
    if (width <= 0 || row_end < row_begin) return 0;
    const size_t rows = (size_t)(row_end - row_begin);
    if (!(flags & JPGX_FLAG_SUBSAMPLE) || sample_ratio == 0) return rows * (size_t)(width / 8);
    return (sample_ratio == 2 ? rows / 2 : rows) * (size_t)(width / 16);
}

size_t jpgx_workspace_size(const jpgx_frames *fr)
{
    /* every kernel keeps its exact-pass queues in LDS */
    (void)fr;
    return 0;
}

}  /* extern "C" */

/* ---- packed-pair equivalence (host) --------------------------------------------------------
 * The kernel's packed path (xform_math.h: PairOps, jx_fdct8_pk) must produce, lane by lane, the
 * very fp32 values of the scalar FOps code the guard band was derived for.  HostPair evaluates
 * the packed code with one correctly rounded scalar operation per lane, as v_pk_* does. */
namespace {
struct HF2 {
    float x, y;
};
struct HostPair {
    typedef HF2 V;
    static V mk(float a, float b) { return V{a, b}; }
    static float lo(V a) { return a.x; }
    static float hi(V a) { return a.y; }
    static V add(V a, V b) { return V{a.x + b.x, a.y + b.y}; }
    static V sub(V a, V b) { return V{a.x - b.x, a.y - b.y}; }
    static V mul(V a, V b) { return V{a.x * b.x, a.y * b.y}; }
    static V fma(V a, V b, V c) { return V{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y)}; }
};

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

/* one block-channel both ways: scalar rows/cols (the bound's code) vs the kernel's packed
 * order (rows: jx_fdct8_pk on pixel pairs; columns: jx_fdct8 over PairOps on column pairs) */
template <int CH>
long long block_mismatch(const uint8_t px[8][8][3], const float w[64])
{
    typedef PairOps<HostPair> PO;
    float T[8][8], Fs[8][8];
    for (int y = 0; y < 8; y++) {
        float in[8];
        for (int x = 0; x < 8; x++)
            in[x] = jx_pixel<FOps, CH>((float)px[y][x][0], (float)px[y][x][1], (float)px[y][x][2]);
        jx_fdct8<FOps>(in, T[y]);
    }
    for (int u = 0; u < 8; u++) {
        float col[8], out[8];
        for (int y = 0; y < 8; y++) col[y] = T[y][u];
        jx_fdct8<FOps>(col, out);
        for (int v = 0; v < 8; v++) Fs[v][u] = out[v];
    }
    HF2 Tp[8][4];
    for (int y = 0; y < 8; y++) {
        HF2 in[4];
        for (int k = 0; k < 4; k++) {
            const HF2 r{(float)px[y][2 * k][0], (float)px[y][2 * k + 1][0]};
            const HF2 g{(float)px[y][2 * k][1], (float)px[y][2 * k + 1][1]};
            const HF2 b{(float)px[y][2 * k][2], (float)px[y][2 * k + 1][2]};
            in[k] = jx_pixel<PO, CH>(r, g, b);
        }
        jx_fdct8_pk<HostPair>(in, Tp[y]);
    }
    long long bad = 0;
    const float magic = 12582912.0f;
    for (int j = 0; j < 4; j++) {
        HF2 col[8], out[8];
        for (int y = 0; y < 8; y++) col[y] = Tp[y][j];
        jx_fdct8<PO>(col, out);
        for (int v = 0; v < 8; v++)
            for (int l = 0; l < 2; l++) {
                const int u = jx_pk_k(j, l);
                const float Fp = l ? out[v].y : out[v].x;
                if (bits(Fp) != bits(Fs[v][u])) bad++;
                /* quantiser: tm = fma(F,w,M), d = fma(F,w,-(tm-M)) in both forms */
                const float ww = w[v * 8 + u];
                const HF2 Fw = HostPair::mk(Fp, Fp), W = HostPair::mk(ww, ww);
                const HF2 tm = HostPair::fma(Fw, W, HostPair::mk(magic, magic));
                const HF2 rr = HostPair::sub(tm, HostPair::mk(magic, magic));
                const HF2 d = HostPair::fma(Fw, W, HostPair::mk(-rr.x, -rr.y));
                const float tms = fmaf(Fs[v][u], ww, magic), ds = fmaf(Fs[v][u], ww, -(tms - magic));
                if (bits(tm.x) != bits(tms) || bits(d.x) != bits(ds)) bad++;
            }
    }
    return bad;
}
}  // namespace

extern "C" long long jx_selftest_pk(long long nblocks, unsigned long long seed)
{
    float w[3][64], lim[3][64];
    int16_t q[2][64];
    jx_plan_tables(90, w, lim, q);
    uint64_t s = seed;
    long long bad = 0;
    uint8_t px[8][8][3];
    for (long long n = 0; n < nblocks; n++) {
        const int kind = (int)(n % 4);  /* random, flat, two-level, ramps */
        const uint64_t r0 = sm64(s);
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++)
                for (int c = 0; c < 3; c++) {
                    uint8_t v;
                    if (kind == 0) v = (uint8_t)(sm64(s) >> 56);
                    else if (kind == 1) v = (uint8_t)(r0 >> (8 * c));
                    else if (kind == 2) v = ((r0 >> (x + 8 * y)) & 1) ? 255 : (uint8_t)(r0 >> 40);
                    else v = (uint8_t)((x * (int)(r0 & 31) + y * (int)((r0 >> 5) & 31) + c * 7) & 255);
                    px[y][x][c] = v;
                }
        bad += block_mismatch<0>(px, w[0]) + block_mismatch<1>(px, w[1]) + block_mismatch<2>(px, w[2]);
    }
    return bad;
}

/* ---- k_mxs / k_mxs422 / k_mxs420: colour conversion + row DCT as f16 MFMA products --------
 *
 * The kernels multiply a row of pixel bytes b_k by a matrix B[k][n], split into two f16 parts
 * (JX_MX_PARTS: hi and lo).  Three matrices ("mode"), one code path below:
 *   mode 0 (k_mxs, and the Y of every kernel): a pixel row of a block, 24 bytes (k = 3x + p, plane
 *     p of pixel x), B[k][n] = a[c][p] cos((2x+1)u pi/16), n = 8c + u, c = Y, Cb, Cr, with a bias
 *     row (input 1.0) carrying the level shift, -8 * 128 for Y at u = 0 (preprocess.c:160-162,
 *     186-188: Y - 128; the level-shifted chroma has no constant; the true cosines of u > 0 sum
 *     to 0).  One K = 32 product per part.
 *   mode 1 / 2 (the chroma of k_mxs422 / k_mxs420; the EXTENSION's definition, oracle/cpu_ref.c
 *     cpuref_chroma_sample): a chroma row of a chroma block is, for 4:2:2, the 16 pixels (48 bytes)
 *     of one pixel row of its MCU, the sample X the average of pixels 2X, 2X+1 of the level-shifted
 *     chroma; for 4:2:0 the 16 pixels of two pixel rows (96 bytes, k = 48 r + 3x + p), the sample
 *     the average of the 2 x 2 quad.  The row transform is linear in the bytes:
 *       R(u) = sum_{r, x < 16, p} b_{48r+3x+p} w a[c][p] cos((2 floor(x/2) + 1) u pi/16),
 *     w = 1/2 or 1/4, c = Cb, Cr, n = 8 c' + u (c' = 0 Cb, 1 Cr); its bias row is all zero.  Two /
 *     three K = 32 products per part (k = 0..31, 32..63 [, 64..95]).
 * The split: Bh = B rounded to a multiple of 2^-11 (|B| < 1: 11 bits; bias: its f16), Bl = the f16
 * of B - Bh, stored at the hi part's scale: R = acc_h + acc_l is one add.
 * Encoding (the kernel's A is one v_perm per two bytes): A holds the byte zero-extended to 16
 * bits, i.e. the f16 subnormal b 2^-24 (exact), the bias lanes 1.0; B's byte rows are stored
 * x 2^15 and the bias row x 2^-9, so every product is b B 2^-9 (exact in fp32) and the MFMA's
 * results are R 2^-9.  Scaling by a power of two changes no rounding, so the kernel's fp32
 * values are those of the true-scale arithmetic below times 2^-9 bit for bit; the column pass
 * scales with them, and the quantiser's w x 2^9 (jpgx_mx.hip kRScale) gives the very fp32 F w.
 * acc_h = sum_k b_k Bh_k is EXACT whatever the order of the MFMA's additions: every product
 * and every partial sum is a multiple of 2^-11 below 2^13 in magnitude (24 bits).  acc_l =
 * sum_k b_k Bl_k is below 1 in magnitude; each of its additions is charged one ulp
 * (32 products per MFMA plus the accumulator: 33, 65 or 97 by mode).  R = fl(acc_h + acc_l)
 * then enters the column pass (jx_fdct8, FOps, two blocks per v_pk_* pair) as usual.
 *
 * Operand layout (v_mfma_f32_16x16x32_f16: lane l holds A[row l & 15][k = 8 (l >> 4) + e] and
 * B[k = 8 (l >> 4) + e][column l & 15], e = 0..7); mode 0: k < 24 is byte k of the pixel row,
 * k = 24 the bias (A = 1.0), k > 24 weight 0.
 */
static const double kMxA[3][3] = {{0.299, 0.587, 0.114},
                                  {-0.168736, 0.331264, -0.5},
                                  {0.5, -0.418688, -0.081312}};

/* round to the nearest f16 (ties to even); bit pattern in *bits */
static long double f16_round(long double x, uint16_t *bits)
{
    if (x == 0) {
        *bits = 0;
        return 0;
    }
    const int e = ilogbl(x);
    const int qe = std::max(e - 10, -24);
    const long double v = rintl(ldexpl(x, -qe)) * ldexpl(1.0L, qe);
    const long double av = fabsl(v);
    uint16_t s = v < 0 ? 0x8000 : 0;
    const int ev = ilogbl(av);
    if (ev < -14) {
        s |= (uint16_t)llrintl(ldexpl(av, 24));
    } else {
        const long long mant = llrintl(ldexpl(av, 10 - ev)) - 1024;
        s |= (uint16_t)(((ev + 15) << 10) | mant);
    }
    *bits = s;
    return v;
}

/* a mode's byte rows (the bias row is row mx_nk), columns, and K = 32 products per part */
static int mx_nk(int mode) { return mode ? 48 * mode : 24; }
static int mx_ncol(int mode) { return mode ? 16 : 24; }
static int mx_products(int mode) { return mode + 1; }

/* exact B[k][n] of a mode (k < mx_nk: matrix, k = mx_nk: bias row) */
static long double mx_exact(int mode, int k, int n)
{
    if (n >= mx_ncol(mode) || k > mx_nk(mode)) return 0;
    const long double pi = 3.141592653589793238462643383279502884L;
    const int u = n % 8;
    if (mode == 0) {
        const int c = n / 8;
        if (k < 24) {
            const int x = k / 3, p = k % 3;
            return (long double)kMxA[c][p] * cosl((2 * x + 1) * u * pi / 16);
        }
        return u == 0 && c == 0 ? -1024.0L : 0;
    }
    if (k == mx_nk(mode)) return 0;
    const int c = 1 + n / 8, kk = k % 48, x = kk / 3, p = kk % 3;
    return (mode == 1 ? 0.5L : 0.25L) * (long double)kMxA[c][p] * cosl((2 * (x / 2) + 1) * u * pi / 16);
}

/* f16 encodings of the split parts (see above): a byte row's value x 2^15, the bias row's
 * x 2^-9; returns the true-scale value the encoding represents */
constexpr int kMxBExp = 15, kMxBiasExp = -9;
static long double mx_enc(long double v, bool bias, uint16_t *bits)
{
    const int e = bias ? kMxBiasExp : kMxBExp;
    return ldexpl(f16_round(ldexpl(v, e), bits), -e);
}

/* one mode's split matrix: true-scale values and f16 bit patterns, rows 0..nk (nk = the bias row) */
struct MxSplit {
    int mode, nk, ncol;
    long double h[97][24], l[97][24];
    uint16_t bh[97][24], bl[97][24];
    uint16_t bits(int part, int k, int n) const { return k > nk ? 0 : (part == 0 ? bh[k][n] : bl[k][n]); }
};
typedef std::unique_ptr<MxSplit> MxSplitPtr;        /* heap, per call: reentrant across threads */

static int mx_split(int mode, MxSplit &S)
{
    memset(&S, 0, sizeof S);
    S.mode = mode;
    S.nk = mx_nk(mode);
    S.ncol = mx_ncol(mode);
    for (int k = 0; k <= S.nk; k++)
        for (int n = 0; n < S.ncol; n++) {
            const long double B = mx_exact(mode, k, n);
            const bool bias = k == S.nk;
            const long double hv = mx_enc(bias ? B : rintl(ldexpl(B, 11)) / 2048.0L, bias, &S.bh[k][n]);
            if (ldexpl(hv, 11) != rintl(ldexpl(hv, 11))) return JPGX_EARG;
            S.h[k][n] = hv;
            S.l[k][n] = mx_enc(B - hv, bias, &S.bl[k][n]);
        }
    for (int n = 0; n < S.ncol; n++) {          /* acc_h exactness: partial sums < 2^13 */
        long double sh = fabsl(S.h[S.nk][n]);
        for (int k = 0; k < S.nk; k++) sh += 255.0L * fabsl(S.h[k][n]);
        if (sh >= 8192.0L) return JPGX_EARG;
    }
    return JPGX_OK;
}

/* the split as the tests and pins read it: two parts, the lo part at the hi part's scale (2^0) */
extern "C" int jx_mx_parts(void) { return JX_MX_PARTS; }
extern "C" int jx_mx_loexp(void) { return 0; }

/* k_mxs's operands, 3 * part + which; lane l holds B[k = 8 (l >> 4) + e][plan column of l & 15].
 * which 0 = columns j = 8c + u for c = Y, Cb; 1 = Cr at u = j for j < 8, zero columns j >= 8;
 * 2 = zero columns j < 8, Cr at u = j - 8 for j >= 8 (the six-tile form sums A_set0 B1 + A_set1 B2:
 * the two sets concatenated along K; tests/test_mx_pins.py pins it, k_mxs itself runs the three
 * tiles jx_mxs_device_operands derives from it) */
extern "C" int jx_mx_operands(uint16_t ops[3 * JX_MX_PARTS][64][8])
{
    MxSplitPtr S(new MxSplit);
    const int rc = mx_split(0, *S);
    if (rc) return rc;
    for (int part = 0; part < JX_MX_PARTS; part++)
        for (int which = 0; which < 3; which++)
            for (int l = 0; l < 64; l++)
                for (int e = 0; e < 8; e++) {
                    const int k = 8 * (l >> 4) + e, j = l & 15;
                    int n = -1;
                    if (which == 0) n = j;
                    else if (which == 1 && j < 8) n = 16 + j;
                    else if (which == 2 && j >= 8) n = 16 + j - 8;
                    ops[3 * part + which][l][e] = n >= 0 ? S->bits(part, k, n) : 0;
                }
    return JPGX_OK;
}

/* What k_mxs keeps on the device (g_mxs_B), derived from the six tiles above: 0 = Y|Cb hi
 * (ops[0]), 1 = Y|Cb lo (ops[3]), 2 = Bc = [Bh_cr | Bl_cr], the Cr matrix's hi part in C columns
 * 0..7 and its lo part in columns 8..15 -- lane for lane ops[3 * 0 + 1] where l % 16 < 8 and
 * ops[3 * 1 + 2] elsewhere (the set-1 tile is the same matrix shifted by eight columns).  One
 * product A Bc gives acc_h in columns 0..7 and acc_l in columns 8..15 of the same set's Cr. */
static_assert(JX_MX_PARTS == 2, "the Cr tile's halves are the split's two parts");
extern "C" int jx_mxs_device_operands(uint16_t out[3][64][8])
{
    std::unique_ptr<uint16_t[][64][8]> ops(new uint16_t[3 * JX_MX_PARTS][64][8]);
    const int rc = jx_mx_operands(ops.get());
    if (rc) return rc;
    for (int l = 0; l < 64; l++)
        for (int e = 0; e < 8; e++) {
            out[0][l][e] = ops[0][l][e];
            out[1][l][e] = ops[3][l][e];
            out[2][l][e] = (l & 15) < 8 ? ops[3 * 0 + 1][l][e] : ops[3 * 1 + 2][l][e];
        }
    return JPGX_OK;
}

/* k_mxs422's / k_mxs420's operands [part][which][lane][e], which < 2 + mx_products(mode): 0 / 1 = Y
 * of set 0 / set 1 (mode 0's Y columns in C columns 0..7 / 8..15, the other half zero: the product
 * A_set0 B_Y0 + A_set1 B_Y1 is K-concatenated as k_mxs's Cr), 2.. = the chroma K steps
 * (k = 32 (which - 2) + 8 (l >> 4) + e); lane l holds B[k][column l & 15] */
static int mxc_operands(int mode, uint16_t *ops)
{
    MxSplitPtr Y(new MxSplit), C(new MxSplit);
    int rc = mx_split(0, *Y);
    if (!rc) rc = mx_split(mode, *C);
    if (rc) return rc;
    const int nwhich = 2 + mx_products(mode);
    for (int part = 0; part < JX_MX_PARTS; part++)
        for (int which = 0; which < nwhich; which++)
            for (int l = 0; l < 64; l++)
                for (int e = 0; e < 8; e++) {
                    const int j = l & 15, k = 8 * (l >> 4) + e;
                    uint16_t v = 0;
                    if (which >= 2) v = C->bits(part, 32 * (which - 2) + k, j);
                    else if (which == 0 ? j < 8 : j >= 8) v = Y->bits(part, k, j & 7);
                    ops[((part * nwhich + which) * 64 + l) * 8 + e] = v;
                }
    return JPGX_OK;
}

extern "C" int jx_mx422_operands(uint16_t ops[JX_MX_PARTS][4][64][8]) { return mxc_operands(1, &ops[0][0][0][0]); }
extern "C" int jx_mx420_operands(uint16_t ops[JX_MX_PARTS][5][64][8]) { return mxc_operands(2, &ops[0][0][0][0]); }

/* Interval + error bound of R (the column pass input) for column n of the split's matrix. */
static Bnd mx_row_bound(const MxSplit &S, int n)
{
    const int nk = S.nk;
    long double loh = S.h[nk][n], hih = S.h[nk][n];
    long double lol = S.l[nk][n], hil = lol;
    long double sl = fabsl(S.l[nk][n]);
    long double rep = fabsl(mx_exact(S.mode, nk, n) - S.h[nk][n] - S.l[nk][n]);
    for (int k = 0; k < nk; k++) {             /* bytes 0..255 */
        const long double bh = S.h[k][n], bo = S.l[k][n];
        loh += std::min(0.0L, 255.0L * bh);
        hih += std::max(0.0L, 255.0L * bh);
        lol += std::min(0.0L, 255.0L * bo);
        hil += std::max(0.0L, 255.0L * bo);
        sl += 255.0L * fabsl(S.l[k][n]);
        rep += 255.0L * fabsl(mx_exact(S.mode, k, n) - S.h[k][n] - S.l[k][n]);
    }
    /* acc_l: mx_products MFMAs of 32 products (mode 0: 25 weights, 7 zeros; k_mxs's Cr
     * tile's second, K-concatenated MFMA adds exact zeros in every column) plus the accumulator
     * input; every addition charged one ulp of the magnitude bound, twice over for an unknown
     * summation tree and rounding mode */
    const double nadd = 2.0 * (32.0 * mx_products(S.mode) + 1.0);
    const double el = (double)(nadd * sl * 0x1p-23L + rep);
    return BoundOps::add(Bnd{(double)loh, (double)hih, 0.0},
                         Bnd{(double)lol - el, (double)hil + el, el});
}

/* The tables of the kernel of `mode`, plan columns n = 8 c + u as jx_mxtab: mode 0 all three
 * channels from mode 0's matrix; mode 1 / 2: c = 0 Y (mode 0's bound), 1 Cb, 2 Cr (the subsampled
 * rows' matrix, columns n - 8) */
static int mx_plan_tables(int mode, int quality, float w[24][8], float lim[24][8], int16_t q[2][64])
{
    int qs[2][8][8];
    int rc = plan_divisors(quality, qs, q);
    if (rc) return rc;
    MxSplitPtr Y(new MxSplit), C;
    rc = mx_split(0, *Y);
    if (!rc && mode) {
        C.reset(new MxSplit);
        rc = mx_split(mode, *C);
    }
    if (rc) return rc;
    const long double a0 = 1.0L / sqrtl(2.0L);
    for (int n = 0; n < 24; n++) {
        const int c = n / 8, u = n % 8, t = c == 0 ? 0 : 1;
        const Bnd R = mode == 0 || c == 0 ? mx_row_bound(*Y, n) : mx_row_bound(*C, n - 8);
        Bnd col[8], out[8];
        for (int y = 0; y < 8; y++) col[y] = R;
        jx_fdct8<BoundOps>(col, out);
        for (int v = 0; v < 8; v++) {
            /* the row transform uses exact cosines: only the column pass's k(v) */
            const long double au = u == 0 ? a0 : 1.0L, av = v == 0 ? a0 : 1.0L;
            const long double ws = 0.25L * au * av * dct_kfactor(v) / (long double)qs[t][u][v];
            plan_band(ws, out[v], &w[n][v], &lim[n][v]);
        }
    }
    return JPGX_OK;
}

extern "C" int jx_plan_tables_mx(int quality, float w[24][8], float lim[24][8], int16_t q[2][64])
{
    return mx_plan_tables(0, quality, w, lim, q);
}

extern "C" int jx_plan_tables_mx422(int quality, float w[24][8], float lim[24][8], int16_t q[2][64])
{
    return mx_plan_tables(1, quality, w, lim, q);
}

extern "C" int jx_plan_tables_mx420(int quality, float w[24][8], float lim[24][8], int16_t q[2][64])
{
    return mx_plan_tables(2, quality, w, lim, q);
}

/* the emulation's test rows: random bytes, every fourth block flat, and for the chroma modes every
 * fourth saturated red */
static void mx_selftest_rows(int mode, long long bk, int nk, uint64_t &s, int px[8][96])
{
    for (int y = 0; y < 8; y++)
        for (int k = 0; k < nk; k++) {
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            px[y][k] = (int)(s >> 56);
            if ((bk & 3) == 1) px[y][k] = px[0][k % 3];      /* flat blocks too */
            if (mode && (bk & 3) == 2) px[y][k] = (k % 3 == 0) ? 255 : 0;
        }
}

/* the exact sample X of a row of channel c (the definition): mode 0 the level-shifted colour of
 * pixel X from double coefficients, mode 1 / 2 the average of the pair's / quad's chroma */
static long double mx_selftest_sample(int mode, int c, const int *row, int X)
{
    if (mode == 0) {
        long double s = (long double)kMxA[c][0] * row[3 * X] + (long double)kMxA[c][1] * row[3 * X + 1] +
                        (long double)kMxA[c][2] * row[3 * X + 2];
        s += c == 0 ? -128.0L : 0.0L;
        return s;
    }
    long double cs = 0;
    for (int r = 0; r < mode; r++)
        for (int h = 0; h < 2; h++) {
            const int x = 2 * X + h, o = 48 * r + 3 * x;
            cs += (long double)kMxA[c][0] * row[o] + (long double)kMxA[c][1] * row[o + 1] +
                  (long double)kMxA[c][2] * row[o + 2];
        }
    return (mode == 1 ? 0.5L : 0.25L) * cs;
}

/* Host emulation of a kernel's fast path on random rows (acc_h exact, acc_l summed in fp32,
 * R = fl(acc_h + acc_l), then the kernel's FOps column pass and quantiser) against the exact
 * quotient 1/4 a(u) a(v) sum_x sum_y X c_u(x) c_v(y) / Q: counts the coefficients whose unflagged
 * fp32 result differs from round(exact quotient) (must be 0) and the flagged ones.  ratio[0] = max
 * |fp32 quotient - exact| / (0.5 - lim).  Mode 0 covers k_mxs's 24 plan columns, mode 1 / 2 the 16
 * chroma columns of k_mxs422 / k_mxs420 (their Y is mode 0's). */
static long long mx_selftest(int mode, long long nblocks, unsigned long long seed, int quality,
                             long long *flagged, double *ratio)
{
    MxSplitPtr S_(new MxSplit);
    const MxSplit &S = *S_;
    if (mx_split(mode, *S_)) return -1;
    float w[24][8], lim[24][8];
    int16_t q[2][64];
    if (mx_plan_tables(mode, quality, w, lim, q)) return -1;
    const long double pi = 3.141592653589793238462643383279502884L;
    const long double a0 = 1.0L / sqrtl(2.0L);
    long double cs[8][8];                       /* cos((2x+1) u pi/16) at [x][u] */
    for (int x = 0; x < 8; x++)
        for (int u = 0; u < 8; u++) cs[x][u] = cosl((2 * x + 1) * u * pi / 16);
    uint64_t s = seed;
    long long bad = 0, nfl = 0;
    double worst = 0;
    for (long long bk = 0; bk < nblocks; bk++) {
        int px[8][96];                          /* row y: mode 0 [8 pixels][3], else [r][16 pixels][3] */
        mx_selftest_rows(mode, bk, S.nk, s, px);
        for (int n = 0; n < S.ncol; n++) {
            const int pn = 24 - S.ncol + n, c = pn / 8, u = pn % 8;      /* plan column */
            float R[8];
            for (int y = 0; y < 8; y++) {
                long double ah = S.h[S.nk][n];
                float al = (float)S.l[S.nk][n];
                for (int k = 0; k < S.nk; k++) {
                    const int sv = px[y][k];
                    ah += sv * S.h[k][n];
                    al = al + (float)(sv * S.l[k][n]);
                }
                R[y] = (float)ah + al;
            }
            float F[8];
            jx_fdct8<FOps>(R, F);
            for (int v = 0; v < 8; v++) {
                long double sum = 0;
                for (int y = 0; y < 8; y++)
                    for (int X = 0; X < 8; X++)
                        sum += mx_selftest_sample(mode, c, px[y], X) * cs[X][u] * cs[y][v];
                const long double au = u == 0 ? a0 : 1.0L, av = v == 0 ? a0 : 1.0L;
                const long double qx = 0.25L * au * av * sum / q[c == 0 ? 0 : 1][u * 8 + v];
                const float tm = fmaf(F[v], w[pn][v], 12582912.0f);
                const float rr = tm - 12582912.0f;
                const float d = fmaf(F[v], w[pn][v], -rr);
                const double qf = (double)F[v] * (double)w[pn][v];
                const double band = 0.5 - (double)lim[pn][v];
                worst = std::max(worst, (double)fabsl((long double)qf - qx) / band);
                if (fabsf(d) >= lim[pn][v]) {
                    nfl++;
                    continue;
                }
                if ((long double)rr != roundl(qx)) bad++;
            }
        }
    }
    if (flagged) *flagged = nfl;
    if (ratio) *ratio = worst;
    return bad;
}

extern "C" long long jx_selftest_mx(long long nblocks, unsigned long long seed, int quality,
                                    long long *flagged, double *ratio)
{
    return mx_selftest(0, nblocks, seed, quality, flagged, ratio);
}

extern "C" long long jx_selftest_mx422(long long nblocks, unsigned long long seed, int quality,
                                       long long *flagged, double *ratio)
{
    return mx_selftest(1, nblocks, seed, quality, flagged, ratio);
}

extern "C" long long jx_selftest_mx420(long long nblocks, unsigned long long seed, int quality,
                                       long long *flagged, double *ratio)
{
    return mx_selftest(2, nblocks, seed, quality, flagged, ratio);
}

/* ---- the one-channel forward path: k_gray (csrc/jpgx_gray.hip, csrc/jx_gray.h) ----
 * The sample is byte - 128, an exact integer in [-128, 127]: the bound starts there with no error and
 * runs through the kernel's own sequence, jx_fdct8 on rows and on columns.  Scales and divisors are the
 * luminance ones of the colour path (same indexing: [v * 8 + u], divisor Qs[u][v]).  The kernel's
 * restatement on the host, for the tests, is csrc/jpgx_gray_host.cpp. */

namespace {

void coef_bounds_gray(Bnd F[8][8])
{
    const Bnd p{-128.0, 127.0, 0.0};
    Bnd px[8], row[8];
    for (int x = 0; x < 8; x++) px[x] = p;
    jx_fdct8<BoundOps>(px, row);   /* every pixel row has the same bound */
    for (int u = 0; u < 8; u++) {
        Bnd col[8], out[8];
        for (int y = 0; y < 8; y++) col[y] = row[u];
        jx_fdct8<BoundOps>(col, out);
        for (int v = 0; v < 8; v++) F[v][u] = out[v];
    }
}

}  // namespace

extern "C" int jx_plan_tables_gray(int quality, float w[64], float lim[64], int16_t q[64])
{
    int qs[2][8][8];
    int16_t qq[2][64];
    const int rc = plan_divisors(quality, qs, qq);
    if (rc) return rc;
    memcpy(q, qq[0], sizeof qq[0]);
    Bnd F[8][8];
    coef_bounds_gray(F);
    const long double a0 = 1.0L / sqrtl(2.0L);
    for (int v = 0; v < 8; v++)
        for (int u = 0; u < 8; u++) {
            const long double au = u == 0 ? a0 : 1.0L, av = v == 0 ? a0 : 1.0L;
            const long double ws = 0.25L * au * av * dct_kfactor(u) * dct_kfactor(v) / (long double)qs[0][u][v];
            plan_band(ws, F[v][u], &w[v * 8 + u], &lim[v * 8 + u]);
        }
    return JPGX_OK;
}

extern "C" int jpgx_guard_band_gray(int quality, float scale[64], float lim[64])
{
    int16_t q[64];
    if (!scale || !lim) return JPGX_EARG;
    return jx_plan_tables_gray(quality, scale, lim, q);
}
