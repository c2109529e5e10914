"""Test helper shared by tests/test_gray.py and tests/test_gray_gpu.py: the
committed one-component files of tests/golden/gray_fixtures/ (tools/make_gray_fixtures.py wrote them with
Pillow), the host's answers for them, each computed once, the damaged files of the sanitizer program
tests/c/gray_san.c, and that program's run."""
import functools
import io
import os

import numpy as np

import jpgx
import jpgx.compat as C
import san_build
from conftest import PKG, REPO

DIR = os.path.join(REPO, "tests", "golden", "gray_fixtures")
# the smallest sizes at which each edge exists: one pixel; partial blocks in both directions; one whole
# block; (64, 8) exactly one run; (65, 17) a last run of one block with one visible column; (263, 21)
# 33 blocks per row, two workgroups per block row; W mod 8 in {0 .. 7} over the set
SIZES = ((1, 1), (7, 9), (8, 8), (12, 30), (21, 13), (35, 18), (64, 8), (65, 17), (129, 65), (263, 21),
         (18, 10), (30, 22))
BIG = (263, 200)                    # one file: its scan crosses the sub-interval kernel's tile five times
PATCHED = (0x22, 0x12, 0x41)        # file 2 of 21 x 13 with SOF's sampling byte replaced
SAN_MAX = 700                       # tests/c/gray_san.c damages the fixtures of at most this many bytes


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def load(name):
    with open(os.path.join(DIR, name), "rb") as f:
        return f.read()


def files_of(W, H):
    """the four files of a size"""
    return [load("g_%dx%d_%d.jpg" % (W, H, k)) for k in range(4)]


def patched_files():
    return [load("g_21x13_2_s%02x.jpg" % s) for s in PATCHED]


def big_file():
    return load("g_%dx%d_noise.jpg" % BIG)


def all_fixtures():
    """[(name, W, H, bytes)] of every committed file"""
    out = [("g_%dx%d_%d.jpg" % (W, H, k), W, H) for W, H in SIZES for k in range(4)]
    out += [("g_%dx%d_noise.jpg" % BIG,) + BIG] + [("g_21x13_2_s%02x.jpg" % s, 21, 13) for s in PATCHED]
    assert sorted(n for n, _, _ in out) == sorted(os.listdir(DIR))
    return [(n, W, H, load(n)) for n, W, H in out]


def nblocks(W, H):
    return -(-W // 8) * -(-H // 8)


@functools.lru_cache(maxsize=None)
def host(data):
    """read_jfif_gray's dict, read-only"""
    r = C.read_jfif_gray(data, 1)
    r["coef"].setflags(write=False)
    r["qt"].setflags(write=False)
    return r


def host_status(data, W, H, reader=None):
    """(status, dict or None) of a host reader for a caller that states W x H, as the device entry
    point's caller does: a header that parses to another size counts as a header error"""
    try:
        info = C.jfif_info_gray(data)
        if (info["width"], info["height"]) != (W, H):
            return jpgx.EJFIF_HEADER, None
        return 0, (reader or C.read_jfif_gray)(data)
    except jpgx.JpgxError as e:
        return e.rc, None


def pillow_pixels(data, mode="L"):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "L"
    return np.asarray(im if mode == "L" else im.convert(mode))


def fits_16_bits(r):
    """tests/pixels_cases.py's condition for the comparison with Pillow, on a read_jfif_gray dict: the
    one component and its table stand in both of its places"""
    import pixels_cases as P
    return P.fits_16_bits(np.concatenate([r["coef"], r["coef"]]), np.stack([r["qt"], r["qt"]]), len(r["coef"]))


def damaged(data):
    """tests/c/gray_san.c's inputs for one file, in its order: every prefix, then every single byte
    replaced by 0x00, by 0xFF and with its low bit flipped"""
    out = [data[:n] for n in range(len(data))]
    for val in (lambda x: 0x00, lambda x: 0xFF, lambda x: x ^ 1):
        for p in range(len(data)):
            b = bytearray(data)
            b[p] = val(b[p])
            out.append(bytes(b))
    return out


def damaged_sample(count=256, seed=0x67726179):
    """a fixed sample of the damaged 21 x 13 files, over the four regular fixtures"""
    pool = [d for f in files_of(21, 13) for d in damaged(f)]
    pick = np.random.default_rng(seed).choice(len(pool), count, replace=False)
    return [pool[k] for k in sorted(pick)]


def hostile_frames(W, H):
    """tests/pixels_cases.py's extreme coefficients and tables for a one-component frame of W x H:
    (coef int16 [n][nb][64], qt uint16 [n][64])"""
    import pixels_cases as P
    coefs, qts = P.hostile_frames(-(-W // 8) * 8, -(-H // 8) * 8, 0)
    nb = nblocks(W, H)
    return np.ascontiguousarray(coefs[:, :nb]), np.ascontiguousarray(qts[:, 0])


def range_limit_ref(coef, qt, W, H):
    """the contract's numpy restatement (tests/idct_ref.py), cropped to the visible frame"""
    import idct_ref
    return idct_ref.samples(coef, qt, -(-W // 8), -(-H // 8))[:H, :W].astype(np.uint8)


def run_san():
    """tests/c/gray_san.c with the host layer, the host decoders and the host pixel routine under the sanitizers, built
    and run once per session; (returncode, stdout, stderr)"""
    libs = san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp"),
                                   os.path.join(PKG, "csrc", "jpgx_pixels_host.cpp")]
    return san_build.run("gray_san", libs, timeout=900)
