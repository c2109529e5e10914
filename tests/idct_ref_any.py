"""Test helper: the pixel contract for a frame of any width and height, restated in
numpy from the contract's text and not from csrc/jx_idct.h or the host twin.

A file of W x H codes every block of its coded frame, W and H rounded up to the MCU.  Whole blocks
are dequantised, transformed and range-limited as for any frame (tests/idct_ref.py's `samples`, which
this file takes as it is).  Of a chroma plane only wc = ceil(W / hs) samples per row and
hc = ceil(H / vs) rows are the component's: the upsampling's neighbour index clamps to [0, wc - 1]
and the 4:2:0 far row to [0, hc - 1]; with wc <= 2 the chroma is replicated (2 x 1 or 2 x 2), with no
filter in either direction.  The output is rows [0, H) and columns [0, W).

    coded(W, H, sample_ratio) -> (coded W, coded H)
    pixels(coef, W, H, sample_ratio, qt) -> uint8 [H][W][3]      coef: the coded frame's blocks

m24: pass 1's products from the 24-bit multiplier's model (tests/idct_ref.py), not the contract.
"""
import numpy as np

from idct_ref import I32, samples


def sampling(sample_ratio):
    return ((1, 1), (2, 1), (2, 2))[sample_ratio]


def coded(W, H, sample_ratio):
    hs, vs = sampling(sample_ratio)
    return -(-W // (8 * hs)) * 8 * hs, -(-H // (8 * vs)) * 8 * vs


def nblocks(W, H, sample_ratio):
    """(nb, nbc) of the coded frame"""
    hs, vs = sampling(sample_ratio)
    cw, ch = coded(W, H, sample_ratio)
    nb = (cw // 8) * (ch // 8)
    return nb, nb // (hs * vs)


def upsample(p, W, H, vs):
    """p: int32 [hc][wc], the component's real extent, sampled 2 x vs -> int32 [H][W]"""
    hc, wc = p.shape
    y, x = np.arange(H), np.arange(W)
    near, i = y // vs, x // 2
    if wc <= 2:                                      # replication, no filter in either direction
        return p[near][:, i]
    if vs == 2:
        far = np.clip(np.where(y % 2 == 0, near - 1, near + 1), 0, hc - 1)
        s = 3 * p[near] + p[far]                     # [H][wc]
        add, shift = np.where(x % 2 == 0, 8, 7), 4
    else:
        s = p[near]
        add, shift = np.where(x % 2 == 0, 1, 2), 2
    j = np.clip(np.where(x % 2 == 0, i - 1, i + 1), 0, wc - 1)
    return (3 * s[:, i] + s[:, j] + add.astype(I32)) >> I32(shift)


def pixels(coef, W, H, sample_ratio, qt, m24=False):
    coef = np.asarray(coef, np.int16).reshape(-1, 64)
    qt = np.asarray(qt, np.uint16).reshape(2, 64)
    hs, vs = sampling(sample_ratio)
    cw, ch = coded(W, H, sample_ratio)
    bw, bh = cw // 8, ch // 8
    cbw, cbh = bw // hs, bh // vs
    nb, nbc = bw * bh, cbw * cbh
    assert coef.shape[0] == nb + 2 * nbc
    y = samples(coef[:nb], qt[0], bw, bh, m24)[:H, :W]
    wc, hc = -(-W // hs), -(-H // vs)
    cb = samples(coef[nb:nb + nbc], qt[1], cbw, cbh, m24)[:hc, :wc]
    cr = samples(coef[nb + nbc:], qt[1], cbw, cbh, m24)[:hc, :wc]
    if sample_ratio:
        cb, cr = upsample(cb, W, H, vs), upsample(cr, W, H, vs)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
