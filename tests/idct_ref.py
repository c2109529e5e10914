"""Test helper: a numpy restatement of the pixel half of the decoder, written from
the contract's text and not from csrc/jx_idct.h: dequantisation, the 13-bit fixed-point 8-point
transform down the columns (shift 11) and along the rows (shift 18), the wrapping range limit, the
triangle-filter chroma upsampling and the 16-bit fixed-point colour conversion.

Everything runs on np.int32 arrays, whose sums, products and left shifts wrap in two's complement
and whose >> is the arithmetic shift -- the contract's arithmetic as it stands.

    pixels(coef, W, H, sample_ratio, qt) -> uint8 [H][W][3]

mul24 is the device's 24-bit multiplier, written from the text of __mul24 (HIP programming guide: "the
low 24 bits of both operands are multiplied as signed integers; the low 32 bits of the product are
returned") and not from csrc/jx_idct.h.  With m24=True pass 1 takes its products from it: the pixels a
kernel would give if it chose that multiplier for a block whatever the block holds.  The contract is
m24=False; where the two differ, a test can tell which multiplier a kernel chose.
"""
import numpy as np

I32 = np.int32


def _zigzag():
    """natural index (row * 8 + column) of zig-zag position k: the walk along the anti-diagonals"""
    order = []
    for s in range(15):
        cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        if s % 2 == 0:
            cells.reverse()              # even diagonals run upwards (the row falls)
        order += [r * 8 + c for r, c in cells]
    return order


ZZ = _zigzag()
assert ZZ[:6] == [0, 1, 8, 16, 9, 2] and ZZ[-3:] == [55, 62, 63] and sorted(ZZ) == list(range(64))

C298, C390, C541, C765, C899, C1175 = (I32(v) for v in (2446, 3196, 4433, 6270, 7373, 9633))
C1501, C1847, C1961, C2053, C2562, C3072 = (I32(v) for v in (12299, 15137, 16069, 16819, 20995, 25172))


def mul24(a, c):
    """int32 arrays a, c -> the 24-bit multiplier's a * c: each operand's low 24 bits read as a signed
    number, the product's low 32 bits"""
    a24 = (np.asarray(a, I32) << I32(8)) >> I32(8)              # << wraps, >> is arithmetic: the sign of bit 23
    c24 = (np.asarray(c, I32) << I32(8)) >> I32(8)
    return (a24.astype(np.int64) * c24.astype(np.int64)).astype(I32)       # |product| < 2^46; the cast keeps the low 32 bits


def _mul32(a, c):
    return a * c


def _T(i, s, mul=_mul32):
    """the 1-D transform of eight int32 arrays; mul: the multiplier its twelve products come from"""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = mul(i2 + i6, C541)
    t2 = z1 - mul(i6, C1847)
    t3 = z1 + mul(i2, C765)
    t0 = (i0 + i4) << I32(13)
    t1 = (i0 - i4) << I32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = mul(z3 + z4, C1175)
    a0, a1, a2, a3 = mul(a0, C298), mul(a1, C2053), mul(a2, C3072), mul(a3, C1501)
    z1, z2 = mul(z1, -C899), mul(z2, -C2562)
    z3 = mul(z3, -C1961) + z5
    z4 = mul(z4, -C390) + z5
    a0, a1, a2, a3 = a0 + (z1 + z3), a1 + (z2 + z4), a2 + (z2 + z3), a3 + (z1 + z4)
    outs = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    half = I32(1) << I32(s - 1)
    return [(x + half) >> I32(s) for x in outs]


def samples(blocks, qt, bw, bh, m24=False):
    """int16 [bh * bw][64] zig-zag blocks in raster order, uint16 [64] zig-zag table ->
    int32 [8 bh][8 bw] samples 0..255.  m24: pass 1's products from the 24-bit multiplier"""
    blocks = np.asarray(blocks).reshape(bh * bw, 64).astype(I32)
    q = np.asarray(qt).reshape(64).astype(I32)
    with np.errstate(over="ignore"):
        d = np.zeros((bh * bw, 64), I32)
        for k in range(64):
            d[:, ZZ[k]] = blocks[:, k] * q[k]
        d = d.reshape(-1, 8, 8)                                          # [block][row][column]
        p1 = np.stack(_T([d[:, r, :] for r in range(8)], 11, mul24 if m24 else _mul32), axis=1)    # down the columns
        p2 = np.stack(_T([p1[:, :, c] for c in range(8)], 18), axis=2)   # along the rows
    t = p2 & I32(1023)
    s = np.where(t < 128, t + 128, np.where(t < 512, 255, np.where(t < 896, 0, t - 896))).astype(I32)
    return s.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h_up(s, c_even, c_odd, shift, edge_even, edge_odd):
    n = s.shape[1]
    out = np.zeros((s.shape[0], 2 * n), I32)
    out[:, 2::2] = (3 * s[:, 1:] + s[:, :-1] + c_even) >> shift
    out[:, 1:-1:2] = (3 * s[:, :-1] + s[:, 1:] + c_odd) >> shift
    out[:, 0] = edge_even(s[:, 0])
    out[:, -1] = edge_odd(s[:, -1])
    return out


def upsample_422(p):
    return _h_up(p, 1, 2, 2, lambda a: a, lambda a: a)


def upsample_420(p):
    hc = p.shape[0]
    rows = np.arange(2 * hc)
    near = rows // 2
    far = np.clip(np.where(rows % 2 == 0, near - 1, near + 1), 0, hc - 1)   # clamped to the plane
    s = 3 * p[near] + p[far]
    return _h_up(s, 8, 7, 4, lambda a: (4 * a + 8) >> 4, lambda a: (4 * a + 7) >> 4)


def pixels(coef, W, H, sample_ratio, qt, m24=False):
    coef = np.asarray(coef, np.int16).reshape(-1, 64)
    qt = np.asarray(qt, np.uint16).reshape(2, 64)
    bw, bh = W // 8, H // 8
    hs, vs = (1, 1) if sample_ratio == 0 else (2, 1) if sample_ratio == 1 else (2, 2)
    cbw, cbh = bw // hs, bh // vs
    nb, nbc = bw * bh, cbw * cbh
    assert coef.shape[0] == nb + 2 * nbc
    y = samples(coef[:nb], qt[0], bw, bh, m24)
    cb = samples(coef[nb:nb + nbc], qt[1], cbw, cbh, m24)
    cr = samples(coef[nb + nbc:], qt[1], cbw, cbh, m24)
    if sample_ratio == 1:
        cb, cr = upsample_422(cb), upsample_422(cr)
    elif sample_ratio == 2:
        cb, cr = upsample_420(cb), upsample_420(cr)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
