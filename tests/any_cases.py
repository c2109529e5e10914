"""Test helper shared by tests/test_any_size.py and tests/test_any_size_gpu.py (DESIGN.md 3, 4.8,
4.9): the files of the any-size tests, each made once.

Two kinds of input.  Pillow's files of the sizes below, smooth and noise, q 50 and 90, written with
one MCU row per restart interval, without DRI, and with per-image Huffman tables.  And this project's
own files of 64 x 48 with the SOF's width and height patched down by less than one MCU: such a file
is a valid file of the smaller size, with the project's restart layout and JPGX_JFIF_OPTIMIZE tables.
"""
import functools
import io
import os

import numpy as np

import idct_ref_any as R
import jpgx.compat as C
import pixels_cases as P
import san_build
from conftest import PKG

# the smallest sizes at which each edge case exists, for every sampling: one pixel; the replication
# rule (wc <= 2); 6 x 9; even sizes that are no MCU multiple (the p[wc] and last-row clamps); odd;
# partial in one direction only; a last run of one block; more than one workgroup per block row
SIZES = ((1, 1), (3, 5), (4, 4), (6, 9), (18, 10), (30, 22), (17, 15), (16, 33), (33, 16), (129, 65), (263, 21))
QUALITIES = (50, 90)
KINDS = ("smooth", "noise")
WRITERS = (dict(restart_marker_rows=1), dict(), dict(optimize=True))
# what 64 x 48 is patched down to, per sample_ratio: less than one MCU in each direction
PATCHED = {0: ((57, 41),), 1: ((50, 42), (49, 41)), 2: ((50, 34), (49, 33))}
BASE = (64, 48)


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


def image(kind, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "smooth":
        return np.stack([(2 * xx + yy) % 256, 255 - (3 * yy) % 256, (xx + 2 * yy) // 2 % 256], 2).astype(np.uint8)
    return np.random.default_rng(1000 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pillow_file(kind, W, H, sr, q, writer=0):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(image(kind, W, H)).save(b, "JPEG", quality=q, subsampling=sr, **WRITERS[writer])
    return b.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_files(W, H, sr):
    """the four files of a size, the three writers taken in turn"""
    return [pillow_file(kind, W, H, sr, q, (k + W + H) % 3)
            for k, (kind, q) in enumerate((kind, q) for kind in KINDS for q in QUALITIES)]


def patch_size(data, W, H):
    """the file with the SOF's height and width replaced"""
    b = bytearray(data)
    i = 2
    while b[i + 1] not in (0xC0, 0xC1):
        i += 2 + (b[i + 2] << 8 | b[i + 3])
    b[i + 5:i + 9] = bytes([H >> 8, H & 255, W >> 8, W & 255])
    return bytes(b)


@functools.lru_cache(maxsize=None)
def project_file(sr, q, restart_rows, optimize, W=BASE[0], H=BASE[1]):
    """(coef, file) of this project's writer for the 64 x 48 frame of the oracle's coefficients"""
    coef = P.oracle_coef("splitmix", BASE[0], BASE[1], q, sr)
    data = C.write_jfif_ex(coef, BASE[0], BASE[1], q, sr, restart_rows=restart_rows, nthreads=1, optimize=optimize)
    assert R.coded(W, H, sr) == BASE
    return coef, data if (W, H) == BASE else patch_size(data, W, H)


def project_files(sr):
    """[(W, H, coef, file)]: every patched size, with and without restart intervals and own tables"""
    out = []
    for W, H in PATCHED[sr]:
        for q, rr, opt in ((50, 1, False), (90, 0, True), (50, 2, True)):
            coef, data = project_file(sr, q, rr, opt, W, H)
            out.append((W, H, coef, data))
    return out


def fits_16_bits(r):
    """tests/pixels_cases.py's condition for the comparison with Pillow, on a read_jfif(any_size=True) dict"""
    nb, _ = R.nblocks(r["width"], r["height"], r["sample_ratio"])
    return P.fits_16_bits(r["coef"], r["qt"], nb)


def run_san():
    """tests/c/any_san.c with the host layer, the host decoders and the host pixel routine under the
    sanitizers, built and run once per session; (returncode, stdout, stderr)"""
    libs = san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp"),
                                   os.path.join(PKG, "csrc", "jpgx_pixels_host.cpp")]
    return san_build.run("any_san", libs, timeout=900)
