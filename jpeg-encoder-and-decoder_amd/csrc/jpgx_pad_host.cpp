/*
 * jpgx_pad_host.cpp -- TEST-ONLY: k_pad_edge (csrc/jpgx_pad.hip) restated on the host from the text it
 * shares with the kernel, csrc/jx_pad.h: the chunk rule run chunk by chunk over a batch, with plain loads
 * or with every load checked against a buffer and recorded (jx_pad_host).  What the device cannot show --
 * a fifth dword that supplies no byte, read past a row's end -- is a refused load here.  The counters say
 * which paths a set of inputs reached.  No HIP: built with g++, as jpgx_plan.cpp.
 */
#include <string.h>

#include "jx_pad.h"

namespace {

/* the host's loads, as they are */
struct PadHostMem {
    uint32_t u32(const uint8_t *p) const
    {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    uint32_t u8(const uint8_t *p) const { return *p; }
};

/* loads that are checked against a buffer and recorded instead of trusted: touched[i] |= 1 (byte load),
 * 2 (4-byte) for every byte read; a load that is not wholly inside the buffer, or a dword load that is not
 * aligned, is counted in bad: it returns the bytes it may have, zeros for the others, so that a rule
 * which reads too far and uses none of it still builds the right frame, as it would on the device */
struct PadTraceMem {
    const uint8_t *buf;
    size_t len;
    uint8_t *touched;
    long long *bad;
    uint32_t get(const uint8_t *p, size_t n, uint8_t mark) const
    {
        const ptrdiff_t off = p - buf;
        if (off < 0 || (size_t)off > len || n > len - (size_t)off || ((uintptr_t)p & (n - 1))) ++*bad;
        uint32_t v = 0;
        for (size_t i = 0; i < n; i++) {
            const ptrdiff_t at = off + (ptrdiff_t)i;
            if (at < 0 || (size_t)at >= len) continue;
            v |= (uint32_t)buf[at] << (8 * i);
            touched[at] |= mark;
        }
        return v;
    }
    uint32_t u32(const uint8_t *p) const { return get(p, 4, 2); }
    uint32_t u8(const uint8_t *p) const { return get(p, 1, 1); }
};

struct PadGeom {
    size_t in_pitch, in_fstride;
    uint32_t w3, h, pitch, npairs, nframes;
};

/* the kernel's grid, lane by lane: frames x row pairs x chunks */
template <class Mem>
long long pad_run(const Mem &mem, const uint8_t *src0, const PadGeom &g, uint8_t *out, uint64_t *stats)
{
    long long unexplained = 0;
    for (uint32_t f = 0; f < g.nframes; f++) {
        const uint8_t *src = src0 + (size_t)f * g.in_fstride;
        uint8_t *dst = out + (size_t)f * g.npairs * 2u * g.pitch;
        for (uint32_t pair = 0; pair < g.npairs; pair++)
            for (uint32_t c = 0; c < g.pitch / 8u; c++) {
                const JxPadChunk ck = jx_pad_chunk(c, g.pitch, g.w3);
                uint32_t d[5], sh, w[4] = {0, 0, 0, 0};
                bool fast;
                jx_pad_load(mem, src, g.in_pitch, g.w3, g.h, ck, pair, d, sh, fast);
                if (fast) JX_PAD_FUNNEL(w, d, sh);
                else JX_PAD_BYTES(w, mem, src, g.in_pitch, g.w3, g.h, g.pitch, ck.o, pair);
                memcpy(dst + (size_t)pair * 2u * g.pitch + ck.o, w, 16);
                if (!stats) continue;
                stats[8] += c >= 256u;
                if (fast) {
                    stats[sh]++;
                    stats[9 + sh] += ck.xb - sh + 20u == g.w3;
                    continue;
                }
                /* why a chunk is slow, by what the counters are for and not by the rule's own words */
                if (ck.o < g.pitch && ck.o + 16u > g.pitch) stats[7]++;
                else if (ck.xb + 16u > g.w3) stats[5]++;
                else if (ck.xb < sh) stats[4]++;
                else if (sh != 0u && ck.xb - sh + 20u > g.w3) {
                    stats[6]++;
                    stats[13 + sh] += ck.xb - sh + 20u == g.w3 + 1u;
                } else unexplained++;
            }
    }
    return unexplained;
}

}  // namespace

extern "C" long long jx_pad_host(const uint8_t *buf, size_t len, size_t base_off, int width, int height,
                                 size_t in_pitch, size_t in_frame_stride, int nframes, int coded_width,
                                 int coded_height, uint8_t *out, uint8_t *touched, uint64_t *stats)
{
    if (!buf || !out || width < 1 || height < 1 || width > 65535 || height > 65535 || nframes < 1 ||
        coded_width < width || coded_height < height || coded_width % 8 || coded_height % 8 || coded_width > 65536 ||
        coded_height > 65536 || in_pitch < 3u * (size_t)width)
        return -1;
    PadGeom g;
    g.in_pitch = in_pitch;
    g.in_fstride = in_frame_stride;
    g.w3 = 3u * (uint32_t)width;
    g.h = (uint32_t)height;
    g.pitch = 3u * (uint32_t)coded_width;
    g.npairs = (uint32_t)coded_height / 2u;
    g.nframes = (uint32_t)nframes;
    if (!touched) return pad_run(PadHostMem{}, buf + base_off, g, out, stats);
    long long bad = 0;
    const PadTraceMem mem{buf, len, touched, &bad};
    const long long unexplained = pad_run(mem, buf + base_off, g, out, stats);
    return bad + unexplained;
}
