"""Test helper: the contract of the decode at 1 / d of the size, d = 2, 4, 8, restated
in numpy on wrapping int32 -- libjpeg-turbo's default decoder with scale_num / scale_denom = 1 / d.
Written from the contract's text, not from csrc/jx_idct.h: the tests compare the host twins with it.

A luma block becomes m x m = 8 / d samples, a chroma block n x n (chroma_n); the 4-point transform
never reads input 4, the 2-point one never inputs 2, 4 and 6; the 1-point sample is the range-limited
DESCALE(dequantised DC, 3).  4:2:2's chroma goes through the h2v1 triangle filter, clamped at the
component's real extent wc = ceil(W n / 16), and is replicated where wc <= 2 and at d = 8.
"""
import numpy as np

import idct_ref as R8
from idct_ref import I32, ZZ, mul24

SCALES = (2, 4, 8)


def _mul32(a, c):
    return a * I32(c)


def _m24(a, c):
    return mul24(a, np.full_like(a, c))


def _descale(x, s):
    return (x + (I32(1) << I32(s - 1))) >> I32(s)


def T4(i, s, mul=_mul32):
    """eight int32 arrays (i[4] is not read) -> four"""
    tmp0 = i[0] << I32(14)
    tmp2 = mul(i[2], 15137) - mul(i[6], 6270)
    t10, t12 = tmp0 + tmp2, tmp0 - tmp2
    o0 = -mul(i[7], 1730) + mul(i[5], 11893) - mul(i[3], 17799) + mul(i[1], 8697)
    o2 = -mul(i[7], 4176) - mul(i[5], 4926) + mul(i[3], 7373) + mul(i[1], 20995)
    return [_descale(x, s) for x in (t10 + o2, t12 + o0, t12 - o0, t10 - o2)]


def T2(i, s, mul=_mul32):
    """eight int32 arrays (i[2], i[4], i[6] are not read) -> two"""
    t10 = i[0] << I32(15)
    o = -mul(i[7], 5906) + mul(i[5], 6967) - mul(i[3], 10426) + mul(i[1], 29692)
    return [_descale(t10 + o, s), _descale(t10 - o, s)]


def range_limit(x):
    t = x & I32(1023)
    return np.where(t < 128, t + 128, np.where(t < 512, 255, np.where(t < 896, 0, t - 896))).astype(I32)


def chroma_n(m, hs, vs):
    n = m
    while n < 8 and (hs * m) % (2 * n) == 0 and (vs * m) % (2 * n) == 0:
        n *= 2
    return n


assert [[chroma_n(8 // d, hs, vs) for d in SCALES] for hs, vs in ((1, 1), (2, 1), (2, 2))] == \
    [[4, 2, 1], [4, 2, 1], [8, 4, 2]]


def sampling(sample_ratio):
    return ((1, 1), (2, 1), (2, 2))[sample_ratio]


def geometry(W, H, sample_ratio, d):
    """the coded frame's block counts and the scaled sizes"""
    hs, vs = sampling(sample_ratio)
    cbw, cbh = -(-W // (8 * hs)), -(-H // (8 * vs))
    m = 8 // d
    n = chroma_n(m, hs, vs)
    return dict(hs=hs, vs=vs, bw=cbw * hs, bh=cbh * vs, cbw=cbw, cbh=cbh, m=m, n=n, ow=-(-W // d), oh=-(-H // d),
                wc=-(-W * n // (8 * hs)), hc=-(-H * n // (8 * vs)))


def samples(blocks, qt, bw, bh, n, m24=False):
    """int16 [bh * bw][64] zig-zag blocks in raster order, uint16 [64] zig-zag table -> int32 [n bh][n bw]
    samples 0..255.  m24: pass 1's products from the 24-bit multiplier"""
    if n == 8:
        return R8.samples(blocks, qt, bw, bh, m24)
    blocks = np.asarray(blocks).reshape(bh * bw, 64).astype(I32)
    q = np.asarray(qt).reshape(64).astype(I32)
    with np.errstate(over="ignore"):
        d = np.zeros((bh * bw, 64), I32)
        for k in range(64):
            d[:, ZZ[k]] = blocks[:, k] * q[k]
        d = d.reshape(-1, 8, 8)                                          # [block][row][column]
        if n == 1:
            s = range_limit(_descale(d[:, 0, 0], 3)).reshape(-1, 1, 1)
        else:
            T, s1, s2 = (T4, 12, 19) if n == 4 else (T2, 13, 20)
            p1 = np.stack(T([d[:, r, :] for r in range(8)], s1, _m24 if m24 else _mul32), axis=1)    # [block][n][8]
            p2 = np.stack(T([p1[:, :, c] for c in range(8)], s2), axis=2)                            # [block][n][n]
            s = range_limit(p2)
    return s.reshape(bh, bw, n, n).transpose(0, 2, 1, 3).reshape(bh * n, bw * n)


def h2v1(p, wc, fancy):
    """a chroma plane's rows, wc real samples each -> 2 wc samples: the triangle filter with the
    neighbour's index clamped to [0, wc - 1], or (not fancy, or wc <= 2) each sample twice"""
    p = p[:, :wc]
    if not fancy or wc <= 2:
        return np.repeat(p, 2, axis=1)
    i = np.arange(wc)
    left, right = p[:, np.maximum(i - 1, 0)], p[:, np.minimum(i + 1, wc - 1)]
    out = np.zeros((p.shape[0], 2 * wc), I32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def pixels(coef, W, H, sample_ratio, qt, d, m24=False):
    """the coded frame's coefficients Y | Cb | Cr and uint16 [2][64] -> uint8 [oh][ow][3]"""
    g = geometry(W, H, sample_ratio, d)
    coef = np.asarray(coef, np.int16).reshape(-1, 64)
    qt = np.asarray(qt, np.uint16).reshape(2, 64)
    nb, nbc = g["bw"] * g["bh"], g["cbw"] * g["cbh"]
    assert coef.shape[0] >= nb + 2 * nbc
    y = samples(coef[:nb], qt[0], g["bw"], g["bh"], g["m"], m24)
    c = [samples(coef[nb + k * nbc:nb + (k + 1) * nbc], qt[1], g["cbw"], g["cbh"], g["n"], m24) for k in (0, 1)]
    if g["hs"] * g["m"] != g["n"]:              # 4:2:2: half the luma's width
        c = [h2v1(p, g["wc"], fancy=g["m"] > 1) for p in c]
    oh, ow = g["oh"], g["ow"]
    return rgb(y[:oh, :ow], c[0][:oh, :ow], c[1][:oh, :ow])


def pixels_gray(coef, W, H, qt, d, channels=1, m24=False):
    """Y [nb][64] and uint16 [64] -> uint8 [oh][ow] or, channels 3, [oh][ow][3] with R = G = B"""
    bw, bh, m = -(-W // 8), -(-H // 8), 8 // d
    coef = np.asarray(coef, np.int16).reshape(-1, 64)
    y = samples(coef[:bw * bh], qt, bw, bh, m, m24)[:-(-H // d), :-(-W // d)].astype(np.uint8)
    return y if channels == 1 else np.repeat(y[:, :, None], 3, axis=2)
