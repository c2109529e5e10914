/*
 * jx_jd_sub_body.h -- the body of the kernel that decodes inside a restart interval,
 * included by csrc/jpgx_jfif_dec.hip once per frame family, inside its namespace, with
 *   JD_SUB_KERNEL      the kernel's name: k_jd_sub (three components), k_jd_sub_gray (one)
 *   JD_SUB_TABS_OF     jxs_tabs_of / jxs_tabs_of_gray
 *   JD_SUB_BLOCK_OF    jxs_block_of / jxs_block_of_gray
 *   JD_SUB_STORE       jxs_store / jxs_store_t<1>
 *   JD_SUB_COMPONENTS  3u / 1u: the DC predictors
 * A text inclusion and no template: k_jd_sub has to stay the instructions it was measured as, and a
 * body shared through an inlined function template was compiled to others.
 * No include guard: it is meant to be included more than once.
 */
__global__ __launch_bounds__(kT) void JD_SUB_KERNEL(const JdArgs a)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    __shared__ jxd_tab tabs[4];
    __shared__ uint32_t tile_s[(kTile + 2) * kRow];
    __shared__ uint32_t ex_p[kT], ex_cz[kT];
    __shared__ uint32_t wtot[kT / 64];
    __shared__ uint32_t first_bad_s;
    const uint32_t f = blockIdx.y, t = threadIdx.x;
    if (a.st[f]) return;                /* the same for the whole workgroup */
    const jxd_frame *fr = a.frames + f;
    const uint32_t ni = fr->ni;
    if (blockIdx.x >= ni || fr->nblk != a.nblk) return;     /* as k_jd_scan: the stated geometry's blocks fit the slot */
    const uint32_t *src = (const uint32_t *)(a.tabs + 4 * (size_t)f);
    for (uint32_t i = t; i < 4u * sizeof(jxd_tab) / 4u; i += kT) ((uint32_t *)tabs)[i] = src[i];
    jxs_tabs tb;
    JD_SUB_TABS_OF(fr, tabs, &tb);
    const size_t len = (size_t)a.len[f];
    const uint8_t *file = a.files + (size_t)f * a.fstride;
    int16_t *coef = a.coef + (size_t)f * a.cstride;
    const uint32_t *mpos = a.mpos + (size_t)f * a.nmcu;
    uint32_t err = 0;
    for (uint32_t iv = blockIdx.x; iv < ni; iv += gridDim.x) {
        const size_t begin = iv ? (size_t)mpos[iv - 1] + 2 : (size_t)fr->scan_off;
        const size_t end = iv + 1 < ni ? (size_t)mpos[iv] : len - 2;
        const uint32_t mcu0 = iv * fr->mpi;
        const uint32_t count = min(fr->mpi, fr->nmcu - mcu0);
        const uint32_t nblocks = count * tb.bpm;
        if (begin > end || end > len) {  /* the same for the whole workgroup */
            err = 1;
            continue;
        }
        /* the interval's blocks zeroed, 16 bytes a lane; the stores are complete before a coefficient's */
        for (uint32_t o = t; o < nblocks * 8u; o += kT) {
            const uint32_t blk = JD_SUB_BLOCK_OF(fr, mcu0, nblocks, o >> 3);
            const u4 zero = {0u, 0u, 0u, 0u};
            if (blk != JXS_INVALID) ((u4 *)(coef + (size_t)blk * 64))[o & 7u] = zero;
            else err = 1;
        }
        __threadfence();
        __syncthreads();                /* also: the tables are in LDS, the last interval's LDS is free */
        jxs_state carry = {0u, 0u};
        uint32_t carry_blocks = 0, done = 0;
        for (size_t tbeg = begin; tbeg < end; tbeg += (size_t)kS * kTile) {
            const jxs_tile tile = jxs_tile_of(end - tbeg, kS, kTile);
            /* load: 16-byte pieces from the boundary before the tile, whole ones by one load */
            const uint8_t *g0 = file + tbeg;
            const uint32_t shift = (uint32_t)((uintptr_t)g0 & 15u);
            const uint32_t npiece = (shift + tile.lim + 15u) / 16u;
            for (uint32_t k = t; k < npiece; k += kT) {
                const uint32_t q = 16u * k;         /* the piece's place in LDS, before the padding */
                u4 v = {0u, 0u, 0u, 0u};
                if (q >= shift && q + 16u - shift <= tile.lim) {
                    v = *(const u4 *)(g0 + (q - shift));
                } else {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (uint32_t j = 0; j < 16u; j++)
                        if (q + j >= shift && q + j - shift < tile.lim) w[j >> 2] |= (uint32_t)g0[q + j - shift] << (8u * (j & 3u));
                    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
                }
                uint32_t *dst = tile_s + (q / kS) * kRow + (q % kS) / 4u;
                dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
            }
            if (t == 0) first_bad_s = kT;
            __syncthreads();
            const JdTile rd = {(const uint8_t *)tile_s, shift};
            const bool active = t * kS < tile.n;
            const uint32_t sub_end = min((t + 1u) * kS, tile.n);
            jxs_state entry = carry, exit = {JXS_INVALID, 0u};
            uint32_t nblk = 0;
            jxs_nowrite nw;
            if (active) {
                err |= jxs_bare_ff(rd, t * kS, sub_end, tile.end_rel);
                if (t) entry = jxs_guess(rd, t, kS, (uint32_t *)nullptr);
                jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, nw, &exit, &nblk);
            }
            /* rounds: at most kT, and after r of them the first r + 1 exits are the sequential decoder's */
            for (uint32_t round = 0; round < kT; round++) {
                ex_p[t] = exit.p;
                ex_cz[t] = exit.cz;
                __syncthreads();
                int changed = 0;
                if (active && t) {
                    const jxs_state prev = {ex_p[t - 1], ex_cz[t - 1]};
                    if (prev.p != JXS_INVALID && !jxs_same(prev, entry)) {
                        entry = prev;
                        jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, nw, &exit, &nblk);
                        changed = 1;
                    }
                }
                if (!__syncthreads_or(changed)) break;
            }
            /* the first lane whose exit is invalid decoded from a true state, as all before it did */
            if (active && exit.p == JXS_INVALID) atomicMin(&first_bad_s, t);
            uint32_t total;
            const uint32_t ord = carry_blocks + jd_scan(active ? nblk : 0u, wtot, total);
            const uint32_t first_bad = first_bad_s;
            int mine = 0;
            if (active && t <= first_bad && entry.p != JXS_INVALID && ord < nblocks) {
                JD_SUB_STORE wr;
                wr.open(fr, coef, mcu0, nblocks, ord);
                jxs_state out;
                uint32_t nb;
                jxs_decode_sub(rd, tile.lim, sub_end, entry, &tb, wr, &out, &nb);
                if (out.p == JXS_INVALID) {
                    err = 1;
                } else if (wr.ord == nblocks) {             /* this lane completed the interval's last block */
                    mine = 1;
                    if (!jxs_tail_ok(rd, tile.lim, tile.end_rel, out.p)) err = 1;
                }
            }
            const uint32_t last_p = ex_p[kT - 1], last_cz = ex_cz[kT - 1];
            done = (uint32_t)__syncthreads_or(mine);        /* and: the tile's LDS is free */
            if (done || first_bad < kT) break;              /* nothing behind an invalid state is true */
            carry.p = last_p - kS * kTile * 8u;             /* seen from the next tile (if there is one) */
            carry.cz = last_cz;
            carry_blocks += total;
        }
        if (!done) err = 1;
        /* the DC predictors: per component a running sum over the interval's blocks in decode order,
         * 256 at a time, each chunk's sums checked against int16 before the carry moves on */
        __threadfence();
        if (__syncthreads_or((int)err)) {
            err = 1;
            continue;
        }
        for (uint32_t comp = 0; comp < JD_SUB_COMPONENTS; comp++) {
            const uint32_t per = comp ? 1u : tb.lum, nbk = count * per;
            uint32_t pred = 0;
            for (uint32_t i0 = 0; i0 < nbk; i0 += kT) {
                const uint32_t i = i0 + t;
                uint32_t blk = JXS_INVALID;
                if (i < nbk) {
                    const uint32_t m = i / per, j = comp ? tb.lum + comp - 1u : i - m * per;
                    blk = JD_SUB_BLOCK_OF(fr, mcu0, nblocks, m * tb.bpm + j);
                }
                const uint32_t d = blk != JXS_INVALID ? (uint32_t)(int32_t)coef[(size_t)blk * 64] : 0u;
                uint32_t sum;
                const int32_t dc = (int32_t)(pred + jd_scan(d, wtot, sum) + d);
                const int out_of_range = dc < -32768 || dc > 32767;
                if (blk != JXS_INVALID && !out_of_range) coef[(size_t)blk * 64] = (int16_t)dc;
                if (__syncthreads_or(out_of_range)) {
                    err = 1;
                    break;
                }
                pred += sum;
            }
            if (err) break;
        }
    }
    if (err) a.status[f] = JPGX_EJFIF_SCAN;
}
