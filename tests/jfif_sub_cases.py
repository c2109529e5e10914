"""Test helper: the inputs that tests/test_jfif_read_sub.py (the host twin jpgx_read_jfif_sub) and
tests/test_jfif_decode_sub_gpu.py (the kernel behind JFIF_DECODE_SUBINTERVAL) share, so that the GPU
decodes the very bytes the twin has decoded, and tests/c/jfif_sub_san.c, built and run once per
session.

The program's extra file (index BIG: 160x128, 4:4:4, no restart intervals, a scan of three tiles of
the kernel's shape) and its corruptions are regenerated here from the program's seeds, as
jfif_san_cases does for tests/c/jfif_read_san.c."""
import io
import os

import numpy as np

import jfif_san_cases as S
import jpgx
import jpgx.compat as C
import san_build
from conftest import GOLDEN, PKG
from jfif_inputs import lap, stuffing_heavy

SUB, TILE = jpgx.jfif_decode_sub_shape()             # the kernel's S and T
SHAPES = [(16, 2), (16, 4), (32, 3), (0, 0)]         # (0, 0): the kernel's own
BIG, BIG_W, BIG_H, BIG_FLIPS = 200, 160, 128, 400
# The program's line for its file BIG (length, FNV-1a hash) and the corruption late_tile_flip() finds
# in its sweep.  tests/test_jfif_read_sub.py holds the program to these values under the sanitizers;
# tests/test_jfif_decode_sub_gpu.py holds the bytes it uploads to them, and runs no sanitizer itself.
BIG_FILE = (36656, 0x2C040DD59C7E4DCA)
BIG_FLIP = (35862, 151)


def write(coef, W, H, q, sr, rr, optimize=False):
    """rr 0: the writers without restart intervals, else write_jfif_ex (as tests/test_jfif_read.py)"""
    if rr == 0 and not optimize:
        return C.write_jfif(coef.reshape(3, -1, 64), W, H, q) if sr == 0 else C.write_jfif_sub(coef, W, H, q, sr)
    return C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1, optimize=optimize)


def intervals(data):
    """[(begin, end)] of the restart intervals of a file the host decoder accepts"""
    scan = C.jfif_info(data)["scan_offset"]
    b = np.frombuffer(data, np.uint8)
    ff = np.flatnonzero(b[scan:-2] == 0xFF) + scan
    marks = ff[(b[ff + 1] & 0xF8) == 0xD0].tolist()
    return list(zip([scan] + [m + 2 for m in marks], marks + [len(data) - 2]))


def big_file():
    """(bytes, coefficients) of the program's file BIG"""
    nb = (BIG_W // 8) * (BIG_H // 8)
    coef = S.coefficients(BIG, 3 * nb * 64)
    return C.write_jfif(coef.reshape(3, nb, 64), BIG_W, BIG_H, 75), coef


def late_tile_flip():
    """the first of the program's corruptions of its file BIG that lies in the scan's third tile of
    the shape (64, 256) and that the host decoder refuses"""
    data, _ = big_file()
    scan = C.jfif_info(data)["scan_offset"]
    for pos, val in S.flips(BIG, data, BIG_FLIPS):
        if scan + 2 * 64 * 256 <= pos < len(data) - 2:
            try:
                C.read_jfif(S.flipped(data, pos, val), 1)
            except jpgx.JpgxError:
                return data, pos, val
    raise AssertionError("the sweep holds no such corruption")


def pillow_tiger(subsampling=2, quality=90):
    """tiger.bmp as Pillow writes it: no restart intervals, Annex K.3 tables"""
    from PIL import Image
    buf = io.BytesIO()
    Image.open(os.path.join(GOLDEN, "images", "tiger.bmp")).convert("RGB").save(
        buf, "JPEG", quality=quality, optimize=False, subsampling=subsampling)
    return buf.getvalue()


def short_intervals(rows=250):
    """an 8-pixel-wide 4:4:4 frame of `rows` one-MCU intervals, each far shorter than a subsequence"""
    W, H = 8, 8 * rows
    rng = np.random.default_rng(5)
    coef = rng.laplace(0, 0.25, size=(3 * rows, 64)).astype(np.int16)
    coef[:, 0] = rng.integers(-300, 300, size=coef.shape[0])
    return W, H, 0, coef, C.write_jfif_ex(coef, W, H, 50, 0, restart_rows=1, nthreads=1)


def whole_multiple():
    """(W, H, sr, coef, bytes, interval) for the first seed at which an interval of a 64x72 4:2:2 file
    of one MCU row per interval is an exact multiple of the kernel's subsequence long"""
    W, H, sr = 64, 72, 1
    for seed in range(2000):
        coef = lap(W, H, sr, 5000 + seed)
        data = write(coef, W, H, 50, sr, 1)
        for k, (b, e) in enumerate(intervals(data)):
            if e > b and (e - b) % SUB == 0:
                return W, H, sr, coef, data, k
    raise AssertionError("no seed gives an interval that is a multiple of the subsequence")


def mechanism_inputs():
    """{name: (W, H, sr, bytes)}: the inputs that make the mechanism work -- a stuffing-heavy frame
    with and without restart intervals, Pillow's 4:2:0 file, the program's three-tile file, intervals
    shorter than a subsequence and one that is a whole number of subsequences"""
    out = {}
    W, H, q, coef = stuffing_heavy(0, 64, 96)
    out["stuffing, one row per interval"] = (W, H, 0, write(coef, W, H, q, 0, 1))
    out["stuffing, no intervals"] = (W, H, 0, write(coef, W, H, q, 0, 0))
    try:
        t = pillow_tiger()
        i = C.jfif_info(t)
        out["pillow 4:2:0"] = (i["width"], i["height"], i["sample_ratio"], t)
    except ImportError:
        pass
    out["three tiles"] = (BIG_W, BIG_H, 0, big_file()[0])
    W, H, sr, _, data = short_intervals()
    out["short intervals"] = (W, H, sr, data)
    W, H, sr, _, data, _ = whole_multiple()
    out["a whole multiple"] = (W, H, sr, data)
    return out


def run_program():
    """tests/c/jfif_sub_san.c with the host layer and the host decoders under the sanitizers, built and
    run once per session; (returncode, stdout, stderr)"""
    return san_build.run("jfif_sub_san", san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp")])
