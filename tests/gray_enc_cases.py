"""Test helper shared by tests/test_gray_encode.py and tests/test_gray_encode_gpu.py:
the oracle of the one-channel forward path, built block by block from the pinned oracle's own routines,
and the inputs of both files, each computed once and read-only.

The contract (include/jpgx.h): the frame is ceil(W / 8) x ceil(H / 8) blocks in raster order with
standard tiling, the pixels beyond the image by the edge rule, the sample (double)g - 128, then
dct_block, quantise_block with the scaled luminance table (applied transposed by quantise_block itself),
C round() and zig-zag."""
import ctypes
import functools

import numpy as np

import jpgx
import oracle
from test_oracle import LUM

QUALITIES = (50, 90, 97)
# one pixel; partial blocks both ways; one block; W mod 8 = 4, 5, 1, 7; (2056, 8): 257 blocks, a fifth wave
SIZES = ((1, 1), (7, 9), (8, 8), (12, 30), (21, 13), (65, 17), (263, 21), (2056, 8))
# sign pattern of cos((2x + 1) 4 pi / 16), x = 0 .. 7; u = 0 has all +1
S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
TIE_COEFS = ((0, 4), (4, 0), (4, 4))          # (u, v): column (horizontal), row (vertical) frequency
TIE_SEED, TIE_CANDIDATES, TIE_QUALITY = 0x74696573, 6000, 90
TIE_COUNT = 355                               # the selection's size: 137, 174 and 62 ties per coefficient


def nblocks(W, H):
    return -(-W // 8) * -(-H // 8)


def edge_frame(img):
    """the coded frame: np.pad by the edge rule to 8 bw x 8 bh"""
    H, W = img.shape
    return np.pad(img, ((0, -H % 8), (0, -W % 8)), mode="edge")


def blocks_of(frame):
    """[8 bh][8 bw] -> [nb][8][8] in raster order, standard tiling"""
    H, W = frame.shape
    return frame.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def coefficients(samples, q):
    """the per-block pipeline on level-shifted samples float64 [8 bh][8 bw]: int16 [nb][64]"""
    table = oracle.scale_table(LUM, q)
    out = np.empty((samples.size // 64, 64), np.int16)
    for k, blk in enumerate(blocks_of(samples)):
        out[k] = oracle.zigzag_block(oracle.quantise_block(oracle.dct_block(np.ascontiguousarray(blk)), table))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_cached(shape, data, q):
    img = np.frombuffer(data, np.uint8).reshape(shape)
    out = coefficients(edge_frame(img).astype(np.float64) - 128.0, q)
    out.setflags(write=False)
    return out


def gray_oracle(img, q):
    """int16 [nb][64] of a uint8 [H][W] image, read-only, computed once per image and quality"""
    img = np.ascontiguousarray(img, np.uint8)
    return _oracle_cached(img.shape, img.tobytes(), q)


def _ro(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def noise(W, H, seed=1):
    """splitmix noise"""
    return _ro(oracle.gen_splitmix(seed + 1000 * W + H, W, H)[:, :, 0])


@functools.lru_cache(maxsize=None)
def ramp(W, H):
    """a smooth ramp, 3/4 of a grey level per pixel across and 5/4 down, with a soft ripple"""
    y, x = np.mgrid[0:H, 0:W]
    return _ro((3 * x + 5 * y) // 4 + (np.sin(x / 5.0) * 3).astype(np.int64) & 255)


@functools.lru_cache(maxsize=None)
def flat():
    """2048 x 8: block k is flat k.  At q 50 all 128 odd values tie in DC, and the oracle rounds them
    toward zero"""
    return _ro(np.repeat(np.arange(256), 8)[None, :].repeat(8, 0))


def image_of_blocks(blocks):
    """[n][8][8] -> an 8 n x 8 image whose block k is blocks[k]"""
    return _ro(np.asarray(blocks).transpose(1, 0, 2).reshape(8, -1))


@functools.lru_cache(maxsize=None)
def extremes():
    """1040 x 8: the 128 sign patterns of the basis functions (0 / 255: the largest coefficients a block
    can have), then all 0 and all 255"""
    cos = np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)      # [u][x]
    blocks = []
    for v in range(8):
        for u in range(8):
            pos = np.outer(cos[v], cos[u]) > 0                                          # [y][x]
            blocks += [np.where(pos, 255, 0), np.where(pos, 0, 255)]
    blocks += [np.zeros((8, 8), np.int64), np.full((8, 8), 255)]
    return image_of_blocks(blocks)


def tie_numerators(blocks):
    """I [n][4] for TIE_COEFS and (0, 0): the real value of coefficient (u, v) in {0, 4}^2 is I / 8 exactly, I = sum of
    (g - 128) s_u(x) s_v(y) with s_0 = 1 and s_4 = S4 (a(0) a(0) = a(0) C4 = C4 C4 = 1/2)"""
    X = np.asarray(blocks, np.int64) - 128                                             # [n][y][x]
    s = {0: np.ones(8, np.int64), 4: S4.astype(np.int64)}
    return np.stack([np.einsum("nyx,x,y->n", X, s[u], s[v]) for u, v in TIE_COEFS] +
                    [np.einsum("nyx->n", X)], axis=1)


def exact_ties(blocks, q):
    """bool [n][4]: coefficient TIE_COEFS[k] (k = 3: (0, 0)) of the block is an exact rounding tie at
    quality q in real arithmetic: I / (8 Q) = n + 1/2, i.e. I mod 8 Q == 4 Q, Q = Qs[u][v]; integers only"""
    table = oracle.scale_table(LUM, q).astype(np.int64)
    Q = np.array([table[u][v] for u, v in TIE_COEFS] + [table[0][0]])
    return np.mod(tie_numerators(blocks), 8 * Q) == 4 * Q


@functools.lru_cache(maxsize=None)
def ties4():
    """uint8 [n][8][8]: the blocks among TIE_CANDIDATES random ones (numpy's PCG64 seeded with TIE_SEED) that
    have an exact tie at q 90 in at least one of (0, 4), (4, 0), (4, 4).  Selected with exact integer
    arithmetic, never with the code under test."""
    cand = np.random.default_rng(TIE_SEED).integers(0, 256, (TIE_CANDIDATES, 8, 8), dtype=np.uint8)
    pick = cand[exact_ties(cand, TIE_QUALITY)[:, :3].any(axis=1)]
    assert len(pick) == TIE_COUNT, len(pick)
    pick.setflags(write=False)
    return pick


def ties4_image():
    return image_of_blocks(ties4())


# ---- the kernel's restatement on the host (csrc/jx_gray.h through csrc/jpgx_gray_host.cpp) ---------
def host_blocks(img, q, force=False, pitch=None):
    """jx_gray_host_blocks: k_gray lane by lane on the host"""
    img = np.asarray(img)
    H, W = img.shape
    if pitch is None:
        img = np.ascontiguousarray(img, np.uint8)
        pitch = W
    out = np.empty((nblocks(W, H), 64), np.int16)
    fn = jpgx.lib.jx_gray_host_blocks
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p]
    rc = fn(img.ctypes.data, W, H, pitch, q, int(force), out.ctypes.data)
    assert rc == 0, rc
    return out


def selftest_blocks(blocks, q):
    """jx_selftest_gray_blocks: (unflagged coefficients that differ from the exact value, flagged
    coefficients, bool [n][8][8] flags at [v][u])"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 64)
    fn = jpgx.lib.jx_selftest_gray_blocks
    fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong),
                   ctypes.c_void_p]
    fn.restype = ctypes.c_longlong
    flagged = ctypes.c_longlong()
    mask = np.zeros(len(blocks), np.uint64)
    bad = fn(blocks.ctypes.data, len(blocks), q, ctypes.byref(flagged), mask.ctypes.data)
    bits = (mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return int(bad), int(flagged.value), bits.astype(bool).reshape(-1, 8, 8)
