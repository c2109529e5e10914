"""Test helper shared by tests/test_pixels_scaled.py and tests/test_pixels_scaled_gpu.py (DESIGN.md
4.9b): the files of the reduced-size tests, their coefficients, Pillow's draft decode and the hostile
frames, each made once.

The sizes: one pixel; smaller than a block; one block; the image's edge inside the first MCU both
ways (9 x 17, 17 x 9); one and two MCUs of 4:2:0; odd sizes of several blocks; a multiple of every MCU;
100 x 75 (an even width that is no multiple of 16: 4:2:2's clamp at wc); 263 x 21, 33 blocks per row: a
second workgroup and a partial last run, and at 1/8 a wave's partial row of 33 pixels.
"""
import functools
import io

import numpy as np

import any_cases as A
import idct_ref_scaled as RS
import jpgx.compat as C

SIZES = ((1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 9), (33, 31), (53, 37), (64, 48), (100, 75), (263, 21))
SCALES = RS.SCALES
SAMPLINGS = (0, 1, 2, "gray")
KINDS_Q = tuple((kind, q) for kind in ("smooth", "noise") for q in (50, 90))
have_pillow = A.have_pillow


def ceil_div(a, b):
    return -(-a // b)


def out_size(W, H, d):
    return ceil_div(W, d), ceil_div(H, d)


@functools.lru_cache(maxsize=None)
def pillow_file(kind, W, H, samp, q):
    if samp != "gray":
        return A.pillow_file(kind, W, H, samp, q, (W + H) % 3)
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(A.image(kind, W, H)[:, :, 1])).save(b, "JPEG", quality=q)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def read(data, gray):
    """the host reader's dict, read-only"""
    r = C.read_jfif_gray(data, 1) if gray else C.read_jfif(data, 1, any_size=True)
    r["coef"].setflags(write=False)
    r["qt"].setflags(write=False)
    return r


def files(W, H, samp):
    """the four Pillow files of a size and sampling"""
    return [pillow_file(kind, W, H, samp, q) for kind, q in KINDS_Q]


def host_pixels(r, gray, d, channels=1):
    """the host twin's pixels of a reader's dict at 1 / d"""
    if gray:
        return C.pixels_host_gray(r["coef"], r["width"], r["height"], r["qt"], channels, nthreads=1, scale=d)
    return C.pixels_host(r["coef"].reshape(-1, 64), r["width"], r["height"], r["sample_ratio"], r["qt"], nthreads=1,
                         scale=d)


def host_raw_d1(r, gray):
    """the C entry points called with scale_denom 1 (jpgx.compat takes the unscaled routine for scale 1)"""
    W, H = r["width"], r["height"]
    coef = np.ascontiguousarray(r["coef"], np.int16)
    qt = np.ascontiguousarray(r["qt"], np.uint16)
    buf = np.zeros((H, W, 1 if gray else 3), np.uint8)
    if gray:
        rc = C.lib.jpgx_pixels_host_gray_scaled(coef.ctypes.data, W, H, 1, qt.ctypes.data, buf.ctypes.data, W, 1, 1)
    else:
        rc = C.lib.jpgx_pixels_host_scaled(coef.ctypes.data, W, H, r["sample_ratio"], 1, qt.ctypes.data, buf.ctypes.data,
                                           3 * W, 1)
    assert rc == 0, rc
    return buf[:, :, 0] if gray else buf


def ref_pixels(r, gray, d, channels=1):
    """the restatement's"""
    if gray:
        return RS.pixels_gray(r["coef"], r["width"], r["height"], r["qt"], d, channels)
    return RS.pixels(r["coef"], r["width"], r["height"], r["sample_ratio"], r["qt"], d)


def fits_16_bits(r, gray):
    """max |coef * qt| < 32768: libjpeg-turbo's SIMD multiplies the two in 16 bits"""
    c = np.asarray(r["coef"], np.int64).reshape(-1, 64)
    if gray:
        return np.abs(c * np.asarray(r["qt"], np.int64).reshape(64)).max() < 32768
    return A.fits_16_bits(r)


def pinned(W, H, d):
    """Pillow's draft() can be made to choose 1 / d for this size"""
    return min(W, H) >= d


def draft_pixels(data, d, mode):
    """Pillow's decode at 1 / d: libjpeg's scale_denom = d.  mode: "RGB" or "L" """
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    W, H = im.size
    im.draft(mode, (max(1, W // d), max(1, H // d)))
    assert im.size == out_size(W, H, d), (im.size, W, H, d)      # the scale Pillow chose is the one under test
    im.load()
    assert im.mode == mode
    return np.asarray(im)


def nblocks(W, H, samp):
    if samp == "gray":
        return ceil_div(W, 8) * ceil_div(H, 8)
    g = RS.geometry(W, H, samp, 2)
    return g["bw"] * g["bh"] + 2 * g["cbw"] * g["cbh"]


HOSTILE_SIZE = (24, 16)         # 3 x 2 blocks


@functools.lru_cache(maxsize=None)
def hostile_frames(samp, W=HOSTILE_SIZE[0], H=HOSTILE_SIZE[1]):
    """(coef int16 [n][nblk][64], qt uint16 [n][2][64] or [n][64]): random full-range coefficients under
    tables of 65535, of random entries up to 65535, of 255 and of 63 (the kernels' threshold for the
    24-bit multiplier), and every coefficient at each extreme under 65535"""
    nblk = nblocks(W, H, samp)
    rng = np.random.default_rng(20 + nblk)
    coefs, qts = [], []
    for top in (65535, None, 255, 63, 64):
        coefs.append(rng.integers(-32768, 32768, (nblk, 64)).astype(np.int16))
        qts.append(np.full((2, 64), top, np.uint16) if top else rng.integers(0, 65536, (2, 64)).astype(np.uint16))
    for v in (32767, -32768):
        coefs.append(np.full((nblk, 64), v, np.int16))
        qts.append(np.full((2, 64), 65535, np.uint16))
    coefs, qts = np.stack(coefs), np.stack(qts)
    if samp == "gray":
        qts = np.ascontiguousarray(qts[:, 0])
    coefs.setflags(write=False)
    qts.setflags(write=False)
    return coefs, qts


MUL_SIZE = (48, 32)
MUL_TABLE = 1024                # above the table threshold: the vote over the run decides
MUL_VALUES = (32767, -32768, 9000)      # times 1024: outside 24 bits


@functools.lru_cache(maxsize=None)
def multiplier_frames(samp, d):
    """Frames on which the 24-bit multiplier in pass 1 gives other pixels than the contract: under a table
    of 1024 a background inside +-31 (every dequantised value inside 16 bits: the vote says small) and, in
    the first or the last block of every component, one large value at zig-zag position 2 (row 1 of
    column 0, input 1 of the column: a factor of every reduced transform).  Each frame is guarded: the
    restatement with the 24-bit multiplier differs from the contract"""
    W, H = MUL_SIZE
    gray = samp == "gray"
    nblk = nblocks(W, H, samp)
    g = None if gray else RS.geometry(W, H, samp, d)
    starts = [0] if gray else [0, g["bw"] * g["bh"], g["bw"] * g["bh"] + g["cbw"] * g["cbh"]]
    ends = [nblk] if gray else starts[1:] + [nblk]
    rng = np.random.default_rng(d)
    coefs = []
    for k, v in enumerate(MUL_VALUES):
        c = rng.integers(-31, 32, (nblk, 64)).astype(np.int16)
        for s, e in zip(starts, ends):
            c[s if k % 2 == 0 else e - 1, 2] = v
        coefs.append(c)
    coefs = np.stack(coefs)
    qts = np.full((len(coefs), 64) if gray else (len(coefs), 2, 64), MUL_TABLE, np.uint16)
    return coefs, qts


def multiplier_tells(samp, d, coef, qt):
    W, H = MUL_SIZE
    if samp == "gray":
        return not np.array_equal(RS.pixels_gray(coef, W, H, qt, d, m24=True), RS.pixels_gray(coef, W, H, qt, d))
    return not np.array_equal(RS.pixels(coef, W, H, samp, qt, d, m24=True), RS.pixels(coef, W, H, samp, qt, d))
