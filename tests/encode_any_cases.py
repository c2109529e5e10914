"""Test helper shared by tests/test_encode_any.py and tests/test_encode_any_gpu.py:
the sizes and images of the encode side's any-size tests, the edge rule stated with numpy, and the
sanitizer program tests/c/encode_any_san.c, built and run once per session."""
import functools
import os

import numpy as np

import jpgx
import oracle
import san_build
from conftest import PKG

# the smallest sizes at which each edge case exists: one pixel; rows shorter than a chunk; 8 x 8 (3 cw =
# 24 in 4:4:4: a chunk straddles the two rows of a pair; a size the plain 4:4:4 path takes too); odd in
# both directions; partial in one direction only; even and no MCU multiple; more than one chunk-run per
# row; rows that start on every residue mod 4; an odd source pitch and several workgroups per row
SIZES = ((1, 1), (3, 5), (8, 8), (17, 15), (16, 33), (33, 16), (30, 22), (129, 65), (263, 21), (667, 9))
BOTH = ((8, 8), (16, 16))               # sizes the plain entry points take as well (4:4:4; 16 x 16: all)
QUALITIES = (50, 90)


def coded(W, H, sr):
    mw, mh = (16 if sr else 8), (16 if sr == 2 else 8)
    return (W + mw - 1) // mw * mw, (H + mh - 1) // mh * mh


def pad_edge(rgb, sr):
    """the edge rule"""
    H, W = rgb.shape[:2]
    cw, ch = coded(W, H, sr)
    return np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)), mode="edge")


@functools.lru_cache(maxsize=None)
def image(kind, W, H):
    if kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        out = np.stack([(2 * xx + yy) % 256, 255 - (3 * yy) % 256, (xx + 2 * yy) // 2 % 256], 2).astype(np.uint8)
    else:
        out = oracle.gen_splitmix(W * 131 + H, W, H)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_coef(kind, W, H, q, sr, sub=True):
    """the oracle's forward transform of the padded image: int16 [3][nb][64] in parity mode (sub False:
    the coded frame is still sample ratio sr's), [nb + 2 nbc][64] as FLAG_SUBSAMPLE lays it out otherwise"""
    rgb = pad_edge(image(kind, W, H), sr)
    full = oracle.blocks(rgb, q)
    if sr == 0 or not sub:
        out = full if not sub else full.reshape(-1, 64)
    else:
        out = np.concatenate([full[0], oracle.chroma_sub(rgb, q, sr).reshape(-1, 64)])
    out = np.ascontiguousarray(out, np.int16)
    out.setflags(write=False)
    return out


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


def run_san():
    """tests/c/encode_any_san.c with the host layer (host/*.c, the host plan, the host scan writer) and
    the host reader under the sanitizers; (returncode, stdout, stderr)"""
    return san_build.run("encode_any_san", san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp")],
                         timeout=900)


def flags_of(sr, sub=True):
    return jpgx.FLAG_SUBSAMPLE if sr and sub else 0
