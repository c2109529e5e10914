"""An independent decoder of one-component (grayscale) baseline JPEG files (test helper), written from
ITU-T T.81 on the bit reader and the canonical tables of tests/jfif_decode.py.  A scan of one
component is not interleaved (T.81 A.2.2): whatever sampling factors SOF states, the MCU is one block,
the frame has ceil(W / 8) x ceil(H / 8) of them in raster order, and DRI counts blocks."""
import numpy as np

from jfif_decode import _Bits, _decode_sym, _extend, _table, _u16


def decode(data: bytes):
    """{width, height, coef int32 [nb][64] (zig-zag), qt [64] (zig-zag), sampling, restart_interval, restarts}"""
    b = bytes(data)
    assert b[:2] == b"\xff\xd8", "no SOI"
    i = 2
    dqt, dht, comp, W, H, ri, sel = {}, {}, None, 0, 0, 0, None
    while True:
        assert b[i] == 0xFF
        m, ln = b[i + 1], _u16(b, i + 2)
        seg = b[i + 4:i + 2 + ln]
        if m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                dqt[tq] = [_u16(seg, j + 1 + 2 * k) for k in range(64)] if pq else list(seg[j + 1:j + 65])
                j += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                bits = list(seg[j + 1:j + 17])
                dht[seg[j]] = _table(bits, list(seg[j + 17:j + 17 + sum(bits)]))
                j += 17 + sum(bits)
        elif m in (0xC0, 0xC1):
            assert seg[0] == 8 and seg[5] == 1, "one 8-bit component"
            H, W = _u16(seg, 1), _u16(seg, 3)
            comp = (seg[6], seg[7], seg[8])
        elif m == 0xDD:
            ri = _u16(seg, 0)
        elif m == 0xDA:
            assert seg[0] == 1 and seg[1] == comp[0]
            sel = seg[2]
            assert (seg[3], seg[4], seg[5]) == (0, 63, 0)
            i += 2 + ln
            break
        i += 2 + ln
    bw, bh = -(-W // 8), -(-H // 8)
    out = np.zeros((bw * bh, 64), np.int32)
    dc_t, ac_t = dht[sel >> 4], dht[0x10 | (sel & 15)]
    br = _Bits(b[i:])
    pred, nrst = 0, 0
    for blk in range(bw * bh):
        if ri and blk and blk % ri == 0:
            br.restart(nrst)
            nrst += 1
            pred = 0
        s = _decode_sym(br, dc_t)
        pred += _extend(br.bits(s), s)
        out[blk, 0] = pred
        k = 1
        while k < 64:
            rs = _decode_sym(br, ac_t)
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r == 15:
                    k += 16
                    continue
                break
            k += r
            out[blk, k] = _extend(br.bits(s), s)
            k += 1
    assert br.d[br.i:][-2:] == b"\xff\xd9", "no EOI after the scan"
    return {"width": W, "height": H, "coef": out, "qt": dqt[comp[2]], "sampling": (comp[1] >> 4, comp[1] & 15),
            "restart_interval": ri, "restarts": nrst}
