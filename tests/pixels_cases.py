"""Test helper shared by tests/test_pixels.py and tests/test_pixels_gpu.py: the
coefficient frames of the pixel tests, each computed once, and the sanitizer program
tests/c/pixels_san.c, built and run once per session."""
import functools
import os

import numpy as np

import jpgx
import oracle
import san_build
from conftest import PKG
from jfif_inputs import nblocks  # noqa: F401  (the pixel tests use it as P.nblocks)

QUALITIES = (1, 50, 90, 97)
# (W, H) per sample mode: 8x8 (16x16 for 4:2:x) is one lane group; 136x16 is 17 blocks per row, a run
# of 8 + 8 + 1 (272x16: 17 chroma blocks per row); 48x32 in 4:2:0 has chroma planes of 2 block rows,
# whose vertical neighbours are the clamped edge on both sides; 96x64
SIZES = {0: ((8, 8), (16, 16), (136, 16), (48, 32), (96, 64)),
         1: ((16, 16), (272, 16), (48, 32), (96, 64)),
         2: ((16, 16), (272, 16), (48, 32), (96, 64))}
EXTREME = (32767, -32767, -32768)
ENTRY = (1, 255, 65535)


@functools.lru_cache(maxsize=None)
def oracle_coef(kind, W, H, q, sr):
    """int16 [nb + 2 nbc][64]: the oracle's forward transform of a splitmix or a tie frame"""
    rgb = oracle.gen_splitmix(W * 131 + H, W, H) if kind == "splitmix" else oracle.gen_tie(W, H)
    full = oracle.blocks(rgb, q)
    if sr == 0:
        out = full.reshape(-1, 64)
    else:
        out = np.concatenate([full[0], oracle.chroma_sub(rgb, q, sr).reshape(-1, 64)])
    out = np.ascontiguousarray(out, np.int16)
    out.setflags(write=False)
    return out


def hostile_frames(W, H, sr):
    """(coef int16 [n][nblk][64], qt uint16 [n][2][64]): every coefficient +-32767 under a table of
    65535; one extreme coefficient per position (in every block) under table entries 1, 255, 65535;
    an all-zero table"""
    nb, nbc = nblocks(W, H, sr)
    nblk = nb + 2 * nbc
    coefs, qts = [], []
    alt = np.where(np.arange(nblk * 64) % 2 == 1, 32767, -32767).astype(np.int16).reshape(nblk, 64)
    for c in (np.full((nblk, 64), 32767, np.int16), np.full((nblk, 64), -32767, np.int16), alt):
        coefs.append(c)
        qts.append(np.full((2, 64), 65535, np.uint16))
    for k in range(64):
        for v in EXTREME:
            for e in ENTRY:
                c = np.zeros((nblk, 64), np.int16)
                c[:, k] = v
                coefs.append(c)
                qts.append(np.full((2, 64), e, np.uint16))
    rnd = np.random.default_rng(W + H + sr).integers(-32768, 32768, (nblk, 64)).astype(np.int16)
    coefs.append(rnd)
    qts.append(np.zeros((2, 64), np.uint16))
    # both sides of the kernels' table threshold (entries up to 63 choose the 24-bit multiplier for
    # pass 1 whatever the coefficients): the largest magnitudes it has to carry, and one entry above
    for c in (np.full((nblk, 64), -32768, np.int16), rnd):
        for e in (63, 64):
            coefs.append(c)
            qts.append(np.full((2, 64), e, np.uint16))
        one = np.full((2, 64), 63, np.uint16)
        one[1, 63] = 64
        coefs.append(c)
        qts.append(one)
    return np.stack(coefs), np.stack(qts)


def pillow_images():
    """the smooth, noise and 0/255-saturated 96x64 images of the Pillow parity tests"""
    yy, xx = np.mgrid[0:64, 0:96]
    smooth = np.stack([(2 * xx + yy) % 256, 255 - (3 * yy) % 256, (xx + 2 * yy) // 2 % 256], 2).astype(np.uint8)
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    sat = (rng.integers(0, 2, (64, 96, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return dict(smooth=smooth, noise=noise, saturated=sat)


def fits_16_bits(coef, qt, nb):
    """libjpeg-turbo's SIMD multiplies coefficient and divisor in 16 bits: max |coef * qt| < 32768"""
    c = np.asarray(coef, np.int64).reshape(-1, 64)
    q = np.asarray(qt, np.int64).reshape(2, 64)
    return max(np.abs(c[:nb] * q[0]).max(), np.abs(c[nb:] * q[1]).max()) < 32768


def run_san():
    """tests/c/pixels_san.c with csrc/jpgx_pixels_host.cpp under the sanitizers, built and run once per
    session; returns (returncode, stdout, stderr)."""
    return san_build.run("pixels_san", [os.path.join(PKG, "csrc", "jpgx_pixels_host.cpp")], timeout=600)


def qt_of(q):
    return jpgx.jfif_qt(q)
